"""ctypes binding of liblaff_hip.so, derived from include/laff_hip.h at import.  No fallback: a missing library is an error.

The header is the one description of the ABI: its structs become ctypes.Structure classes (laff_fc_problem -> FcProblem), its
prototypes the SIGNATURES table, its enums and #defines the constants.  A declaration the parser does not understand raises at
import and is named; nothing is guessed."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('LAFF_HIP_LIB') or os.path.join(_HERE, 'lib', 'liblaff_hip.so')   # env override: debug builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'laff_hip.h')

_SCALARS = {'int': C.c_int, 'unsigned': C.c_uint, 'float': C.c_float, 'double': C.c_double, 'long': C.c_long,
            'long long': C.c_longlong, 'unsigned long long': C.c_ulonglong, 'size_t': C.c_size_t, 'int32_t': C.c_int32,
            'int64_t': C.c_int64, 'uint8_t': C.c_uint8}
_POINTEES = ('void', 'char', 'unsigned char')          # further types that occur behind a pointer only


def _declarator(decl, where):
    """'const float* const* x' -> ('float', 2 stars, 'x', None, const);  'int32_t reserved[2]' -> ('int32_t', 0, 'reserved', 2, False)."""
    m = re.fullmatch(r'(.*[\s*])(\w+)\s*(?:\[(\d+)\])?', decl.strip(), flags=re.S)
    if not m:
        raise ValueError('laff_hip.h: cannot parse %r in %r' % (decl.strip(), where))
    words = m.group(1).replace('*', ' * ').split()
    base = ' '.join(w for w in words if w not in ('const', '*'))
    return base, words.count('*'), m.group(2), m.group(3) and int(m.group(3)), words[0] == 'const'


def _ctype(base, stars, count, const, structs, opaque, where, field):
    """The ctypes type of a struct field (field=True) or of a parameter / return value.  Pointer rule: every pointer is c_void_p, but
    `const char*` is c_char_p outside structs and a struct's pointer to another struct of the header is typed."""
    if base not in _SCALARS and base not in _POINTEES and base not in structs and base not in opaque:
        raise ValueError('laff_hip.h: unknown type %r in %r' % (base, where))
    if stars or (count and not field):
        if field and count:
            raise ValueError('laff_hip.h: array of pointers in %r' % where)
        if field:
            return C.POINTER(structs[base]) if base in structs and stars == 1 else C.c_void_p
        return C.c_char_p if (base, stars, count, const) == ('char', 1, None, True) else C.c_void_p
    if base not in _SCALARS:
        raise ValueError('laff_hip.h: %r passed by value in %r' % (base, where))
    return _SCALARS[base] * count if count else _SCALARS[base]


def _struct(name, body, structs, opaque):
    fields = []
    for decl in body.split(';')[:-1]:
        first, *more = decl.split(',')                  # `int N, Dk, ldx;`: one type, several names
        base, stars, field, count, const = _declarator(first, decl.strip())
        if more and (stars or count or not all(re.fullmatch(r'\s*\w+\s*', n) for n in more)):
            raise ValueError('laff_hip.h: cannot parse %r in struct %s' % (decl.strip(), name))
        ctype = _ctype(base, stars, count, const, structs, opaque, decl.strip(), True)
        fields += [(n.strip(), ctype) for n in [field] + more]
    if body.split(';')[-1].strip() or not fields:
        raise ValueError('laff_hip.h: cannot parse the end of struct %s' % name)
    # _as_parameter_: an instance handed to a c_void_p parameter goes by reference, as POINTER(cls) would take it
    return type(''.join(w.capitalize() for w in name.split('_')[1:]), (C.Structure,),
                {'_fields_': fields, '_as_parameter_': property(C.byref)})


def parse_header(text):
    """(structs by C name, signatures by C name, enum constants and integer #defines by C name) of a header in laff_hip.h's style."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    declared = set(re.findall(r'\b(laff_[a-z0-9_]+)\s*\(', text))
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define (LAFF_\w+) (-?\d+)\s*$', text, flags=re.M)}
    text = re.sub(r'^\s*#[^\n]*', '', text, flags=re.M)                     # guards, includes and the #defines read above
    m = re.fullmatch(r'\s*extern "C" \{(.*)\}\s*', text, flags=re.S)
    if not m:
        raise ValueError('laff_hip.h: the declarations are not inside one extern "C" { } block')
    bodies = []
    text = re.sub(r'\{([^{}]*)\}', lambda b: bodies.append(b.group(1)) or '{%d}' % (len(bodies) - 1), m.group(1))
    structs, opaque, sigs = {}, set(), {}
    *statements, rest = text.split(';')
    for stmt in statements + ([rest] if rest.strip() else []):
        stmt = ' '.join(stmt.split())
        e = re.fullmatch(r'enum \{(\d+)\}', stmt)
        o = re.fullmatch(r'typedef struct (laff_\w+) (laff_\w+)', stmt)
        s = re.fullmatch(r'typedef struct (?:(laff_\w+) )?\{(\d+)\} (laff_\w+)', stmt)
        f = re.fullmatch(r'(.*[\s*])(laff_\w+) ?\((.*)\)', stmt)
        if e:
            for item in bodies[int(e.group(1))].split(','):
                kv = re.fullmatch(r'\s*(LAFF_\w+)\s*=\s*(-?\d+)\s*', item)
                if not kv:
                    raise ValueError('laff_hip.h: cannot parse the enumerator %r' % item.strip())
                consts[kv.group(1)] = int(kv.group(2))
        elif o and o.group(1) == o.group(2):
            opaque.add(o.group(1))
        elif s and s.group(1) in (None, s.group(3)):
            structs[s.group(3)] = _struct(s.group(3), bodies[int(s.group(2))], structs, opaque)
        elif f and '{' not in stmt:
            params = [] if f.group(3).strip() == 'void' else [_declarator(p, stmt) for p in f.group(3).split(',')]
            base, stars, _, _, const = _declarator(f.group(1) + ' _', stmt)
            sigs[f.group(2)] = (_ctype(base, stars, None, const, structs, opaque, stmt, False),
                                [_ctype(b, n, c, k, structs, opaque, stmt, False) for b, n, _, c, k in params])
        else:
            whole = re.sub(r'\{(\d+)\}', lambda b: '{%s}' % bodies[int(b.group(1))], stmt)
            raise ValueError('laff_hip.h: cannot parse the declaration %r' % whole)
    if declared != set(sigs):
        raise ValueError('laff_hip.h: function names without a parsed prototype: %s' % sorted(declared ^ set(sigs)))
    return structs, sigs, consts


with open(HEADER_PATH) as _f:
    STRUCTS, SIGNATURES, K = parse_header(_f.read())
globals().update({cls.__name__: cls for cls in STRUCTS.values()})          # Plane, RankSide, FcProblem, ... AssembleJob

ABI_VERSION = K['LAFF_ABI_VERSION']
ASSEMBLE_MAX_JOBS, ASSEMBLE_MAX_BATCH = K['LAFF_ASSEMBLE_MAX_JOBS'], K['LAFF_ASSEMBLE_MAX_BATCH']
ACT = {None: K['LAFF_ACT_NONE'], False: K['LAFF_ACT_NONE'], '': K['LAFF_ACT_NONE'], 'none': K['LAFF_ACT_NONE'],
       'tanh': K['LAFF_ACT_TANH'], 'relu': K['LAFF_ACT_RELU'], 'sigmoid': K['LAFF_ACT_SIGMOID']}
ATT_WITH_AVE, ATT_MUL, ATT_L2NORM_EACH_HEAD, ATT_NO_SPLIT_HEAD, ATT_JUST_AVERAGE = (
    K['LAFF_ATT_' + n] for n in ('WITH_AVE', 'MUL', 'L2NORM_EACH_HEAD', 'NO_SPLIT_HEAD', 'JUST_AVERAGE'))
GRU_POOLING = {n: K['LAFF_GRU_' + n.upper()] for n in ('mean', 'last', 'mean_last')}
OPT_KIND = {n: K['LAFF_OPT_' + n.upper()] for n in ('adam', 'rmsprop')}
PREC = {n: K['LAFF_PREC_' + n.upper()] for n in ('fp32', 'fp16', 'bf16', 'fp16x3', 'bf16x3')}
ASSEMBLE_KIND = {n: K['LAFF_ASSEMBLE_' + n.upper()] for n in ('rows', 'ragged', 'csr')}


def enum_names(prefix):
    """The enumerators that start with prefix, without it, as a tuple indexed by value (the values must run 0, 1, 2, ...)."""
    found = sorted((v, k[len(prefix):]) for k, v in K.items() if k.startswith(prefix))
    if [v for v, _ in found] != list(range(len(found))):
        raise ValueError('laff_hip.h: the %s* values are not 0 .. %d' % (prefix, len(found) - 1))
    return tuple(n for _, n in found)


_lib = None


def load():
    """Load the library once; raises if it has not been built (python -m laff_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('liblaff_hip.so is missing (%s): build it with `python -m laff_amd.build`; '
                               'laff_amd has no CPU fallback' % LIB_PATH)
        # torch bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  It must be in the process BEFORE
        # liblaff_hip.so is loaded so that both resolve to ONE HIP runtime (shared streams / allocations); loaded
        # the other way round the second runtime sees no device.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if lib.laff_abi_version() != ABI_VERSION:
            raise RuntimeError('liblaff_hip.so ABI %d != binding ABI %d: rebuild' % (lib.laff_abi_version(), ABI_VERSION))
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError('liblaff_hip: %s (rc=%d)' % (load().laff_last_error().decode(), rc))
