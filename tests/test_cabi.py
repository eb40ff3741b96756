"""The C-ABI library loads on a CPU-only host and exports every symbol include/laff_hip.h declares."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(laff_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for s in ('laff_ctx_create', 'laff_fc_act_bn', 'laff_fc_route', 'laff_fuse', 'laff_frame_fuse', 'laff_frame_fuse_grouped_mask', 'laff_pack_rows', 'laff_sim_gemm',
              'laff_rank_count', 'laff_v2t_count', 'laff_v2t_count_exact', 'laff_rank_metrics', 'laff_last_error'):
        assert s in syms


def test_library_exports_every_declared_symbol():
    from laff_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from laff_amd.build import build_library
        build_library(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared_symbols():
        assert hasattr(lib, s), 'liblaff_hip.so does not export %s' % s
    assert lib.laff_abi_version() == _lib.ABI_VERSION


def test_binding_covers_every_declared_symbol():
    from laff_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()
    _lib.load()


def test_argument_errors_do_not_need_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.laff_packed_bytes(10, 512, 3, ctypes.byref(n)) == 0 and n.value == 10 * 512 * 2 * 2
    assert lib.laff_packed_bytes(10, 512, 99, ctypes.byref(n)) == -1
    assert b'precision' in lib.laff_last_error()
    assert lib.laff_fuse(None, None, 1, 1, 1, 4, None, None, None, 0, None, None) == -1
    # the collectives and the exact V2T count refuse null handles before touching RCCL or the GPU
    assert lib.laff_comm_init(None, 0, 1, None, None) == -1 and b'laff_comm_init' in lib.laff_last_error()
    assert lib.laff_allgather_rows(None, None, None, 16) == -1
    assert lib.laff_allreduce_i32_sum(None, None, 4) == -1 and lib.laff_allreduce_f64_max(None, None, 4) == -1
    assert lib.laff_comm_destroy(None) == 0
    assert lib.laff_v2t_count_exact(None, None, 1, 1, 1, None, None, 1, None, None, 1, 4, None, None, None, None, None, 4) == -1


# ---- the binding is derived from the header (laff_amd/_lib.py): the C++ compiler checks the derivation -----------------------------
_PROBE = r'''
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "laff_hip.h"
template <class T> void one() {
    if constexpr (std::is_void_v<T>) std::printf(" v0");
    else std::printf(" %c%zu", std::is_pointer_v<T> ? 'p' : std::is_floating_point_v<T> ? 'f' : std::is_signed_v<T> ? 'i' : 'u', sizeof(T));
}
template <class F> struct sig;
template <class R, class... A> struct sig<R(A...)> {
    static void print(const char* name) { std::printf("%s", name); one<R>(); std::printf(" <-"); (one<A>(), ...); std::printf("\n"); }
};
int main() {
@BODY@
    return 0;
}
'''


def _kind(ctype):
    """'p8', 'f4', 'i4', 'u8', ...: class and size of a ctypes type, as the probe prints them for the C type."""
    code = ctype._type_ if isinstance(ctype._type_, str) else 'P'            # POINTER(struct): a pointer
    cls = 'p' if code in 'Pz' else 'f' if code in 'fd' else 'i' if code in 'bhilq' else 'u' if code in 'BHILQ' else '?'
    return '%s%d' % (cls, ctypes.sizeof(ctype))


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    """What the host C++ compiler says about every declaration of the header: {function: 'i4 <- p8 i4 ...'} and {struct or struct.field:
    numbers}.  Nothing of the library is referenced: the program is built from the header alone and is not linked against it."""
    import shutil
    import subprocess
    from laff_amd import _lib, build
    lines = ['    sig<decltype(%s)>::print("%s");' % (s, s) for s in sorted(_lib.SIGNATURES)]
    for cname, cls in _lib.STRUCTS.items():
        lines.append('    std::printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['    std::printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (cname, f, cname, f, cname, f)
                  for f, _ in cls._fields_]
    out = tmp_path_factory.mktemp('probe')
    src, exe = str(out / 'probe.cpp'), str(out / 'probe')
    with open(src, 'w') as fh:
        fh.write(_PROBE.replace('@BODY@', '\n'.join(lines)))
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    cmd = [cxx] if cxx else [build.hipcc(), '-x', 'c++']                     # hipcc's host side when there is no system compiler
    r = subprocess.run(cmd + ['-std=c++17', '-I' + os.path.join(ROOT, 'include'), src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(line.split(' ', 1) for line in r.stdout.splitlines())


def test_signatures_agree_with_the_compiler(probe):
    """Return type and every parameter of every entry point: class (pointer, floating, signed, unsigned) and size, as the C++ compiler
    reads the header against what the binding passes.  A dropped, swapped or mis-sized argument shows here."""
    from laff_amd import _lib
    assert len(_lib.SIGNATURES) >= 115
    for name, (res, args) in _lib.SIGNATURES.items():
        assert probe[name] == ' '.join([_kind(res), '<-'] + [_kind(a) for a in args]), name


def test_structures_agree_with_the_compiler(probe):
    """sizeof, and offset and size of every field, of every struct of the header against the ctypes classes (a lost field shows as a
    sizeof mismatch)."""
    from laff_amd import _lib
    assert len(_lib.STRUCTS) >= 20
    for cname, cls in _lib.STRUCTS.items():
        assert probe[cname] == '%d' % ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert probe['%s.%s' % (cname, f)] == '%d %d' % (getattr(cls, f).offset, getattr(cls, f).size), (cname, f)


def test_pointer_rule_and_typed_struct_pointers():
    """Every pointer parameter is c_void_p, `const char*` is c_char_p; inside structs a pointer to another struct of the header is typed
    (the encoders assign ctypes arrays to `blocks` / `segments`).  A struct instance given for a pointer parameter goes by reference."""
    from laff_amd import _lib
    for name, (res, args) in _lib.SIGNATURES.items():
        assert res in (ctypes.c_int, ctypes.c_char_p), name
        assert all(a in (ctypes.c_void_p, ctypes.c_char_p) or _kind(a)[0] in 'fiu' for a in args), name
    assert _lib.SIGNATURES['laff_last_error'] == (ctypes.c_char_p, [])
    assert _lib.SIGNATURES['laff_match_ids'][1] == [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int,
                                                    ctypes.c_void_p]
    assert _lib.SIGNATURES['laff_comm_init'][1][3] is ctypes.c_void_p                       # const unsigned char*: bytes, not a string
    assert _lib.SIGNATURES['laff_device_info'][1] == [ctypes.c_void_p, ctypes.c_void_p]      # int out[4]
    assert dict(_lib.ClipText._fields_)['blocks'] is ctypes.POINTER(_lib.ClipBlock)
    assert dict(_lib.ClipVisual._fields_)['blocks'] is ctypes.POINTER(_lib.ClipBlock)
    assert dict(_lib.BertText._fields_)['blocks'] is ctypes.POINTER(_lib.BertBlock)
    assert dict(_lib.FcConcatProblem._fields_)['segments'] is ctypes.POINTER(_lib.FcConcatSegment)
    assert dict(_lib.FrameDesc._fields_)['reserved'] is ctypes.c_int32 * 2
    assert all(t is ctypes.c_void_p for n, t in _lib.Plane._fields_ if n in ('src', 'indptr', 'wt', 'row_scale'))
    lib = _lib.load()
    side = _lib.RankSide(2, None, 0, None, 0, None, 4096, None, None, None, None, None)
    assert lib.laff_fuse_packed_rank(None, None, 1, 1, 1, 4, None, None, None, 0, None, None, None, 1, 1.0, side) == -1
    assert b'null ctx' in lib.laff_last_error()


def test_public_values_are_pinned():
    """The derivation renames and renumbers nothing: the constants the package publishes, as literals."""
    from laff_amd import _lib, ops
    assert _lib.ACT == {None: 0, False: 0, '': 0, 'none': 0, 'tanh': 1, 'relu': 2, 'sigmoid': 3}
    assert _lib.PREC == {'fp32': 0, 'fp16': 1, 'bf16': 2, 'fp16x3': 3, 'bf16x3': 4} and ops.PREC is _lib.PREC
    assert _lib.GRU_POOLING == {'mean': 0, 'last': 1, 'mean_last': 2}
    assert _lib.OPT_KIND == {'adam': 0, 'rmsprop': 1}
    assert _lib.ASSEMBLE_KIND == {'rows': 0, 'ragged': 1, 'csr': 2}
    assert (_lib.ATT_WITH_AVE, _lib.ATT_MUL, _lib.ATT_L2NORM_EACH_HEAD, _lib.ATT_NO_SPLIT_HEAD, _lib.ATT_JUST_AVERAGE) == (1, 2, 4, 8, 16)
    assert (_lib.ASSEMBLE_MAX_JOBS, _lib.ASSEMBLE_MAX_BATCH) == (16, 4096)
    assert ops.LOSS_FLAGS == {'max_violation': 1, 'mean': 2, 'i2t': 4, 't2i': 8}
    assert ops.FC_ROUTES == ('F32_REG', 'F32_TAIL', 'F32_GLDS', 'F16_128', 'X3', 'X3_FUSED', 'STRIP', 'GATHER', 'CONCAT')
    assert ops.SIM_ROUTES == ('TILED128_REG', 'TILED128_TAIL', 'TILED128', 'TILED256', 'TILED256_LONGK', 'X3', 'STRIP')
    assert ops._FC_FAMILIES == {'fp32': 0, 'split': 1, 'fused': 2}
    names = ['FcProblem', 'FcConcatSegment', 'FcConcatProblem', 'FcSplitProblem', 'FcFusedProblem', 'FcShape', 'FcLaunch', 'FcStripProblem',
             'ClipBlock', 'ClipText', 'ClipVisual', 'FrameDesc', 'BertBlock', 'BertText', 'Plane', 'OptimTensor', 'OptimHyper', 'RankSide',
             'RerankProblem', 'AssembleJob']
    assert [cls.__name__ for cls in _lib.STRUCTS.values()] == names                        # in the header's order
    assert all(getattr(_lib, n) is cls and issubclass(cls, ctypes.Structure) for n, cls in zip(names, _lib.STRUCTS.values()))
    assert _lib.STRUCTS['laff_fc_concat_segment'] is _lib.FcConcatSegment and _lib.STRUCTS['laff_plane'] is _lib.Plane
    assert _lib.HEADER_PATH in __import__('laff_amd.build', fromlist=['HEADERS']).HEADERS       # the file the library is built from


_MINI = 'typedef struct laff_ctx laff_ctx;\nint laff_ok(laff_ctx* ctx, const float* x /*device*/, size_t n);\n%s\n'


@pytest.mark.parametrize('decl, named', [
    ('int laff_f(laff_ctx* ctx, short x);', "unknown type 'short'.*laff_f"),                       # an unknown type word
    ('typedef struct { int a; wchar_t* b; } laff_s;', "unknown type 'wchar_t'.*wchar_t\\* b"),
    ('int laff_f(laff_other* p);', "unknown type 'laff_other'.*laff_f"),                            # neither a struct nor opaque
    ('int (*laff_cb)(int);', r'cannot parse the declaration.*laff_cb'),                             # not a declaration of the header's kinds
    ('typedef union { int a; float b; } laff_u;', r'cannot parse the declaration.*laff_u'),
    ('static inline int laff_g(int a) { return a; }', r'cannot parse the declaration.*laff_g'),
    ('typedef struct { int* a, b; } laff_s;', r'cannot parse.*int\* a, b'),
    ('enum { LAFF_X = 1, LAFF_Y };', r"cannot parse the enumerator 'LAFF_Y'"),
    ('int laff_f(laff_ctx*);', r'laff_f'),                                                          # a parameter without a name
    ('#define laff_m(x) laff_ok(0, x, 1)', r'without a parsed prototype.*laff_m'),                  # a name the symbol regex sees
])
def test_parser_refuses_what_it_does_not_understand(decl, named):
    from laff_amd import _lib
    wrap = 'extern "C" {\n%s}\n'
    structs, sigs, consts = _lib.parse_header(wrap % (_MINI % 'enum { LAFF_A = -3 };\n#define LAFF_N 7'))
    assert sigs == {'laff_ok': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t])} and consts == {'LAFF_A': -3, 'LAFF_N': 7}
    with pytest.raises(ValueError, match=named):
        _lib.parse_header(wrap % (_MINI % decl))
    with pytest.raises(ValueError, match='extern "C"'):
        _lib.parse_header(_MINI % '')


# ---- one table for what every feature's host test used to assert one copy each: the entry point is in the header, the library and the
# binding, with this many arguments, at an ABI version of at least this ------------------------------------------------------------
ENTRY_POINTS = [          # (symbol, argument count or None where none was asserted, minimum ABI or 0)
    ('laff_dropout_bn_train_plan', 4, 41), ('laff_dropout_bn_train', 19, 41), ('laff_dropout_bn_train_backward', 18, 41),
    ('laff_batch_assemble', None, 45),
    ('laff_bert_workspace_bytes', None, 0), ('laff_bert_encode', None, 0), ('laff_clip_pack_weight', None, 0),
    ('laff_frame_fuse_backward_plan', None, 38), ('laff_frame_fuse_backward', None, 38),
    ('laff_rerank_workspace_bytes', None, 32), ('laff_rerank_run', None, 32), ('laff_rerank_tkb', None, 32),
    ('laff_sim_hist', 12, 33),
    ('laff_fc_gather_backward', 16, 40),
    ('laff_expert_stage_train_plan', 4, 43), ('laff_expert_stage_train', 13, 43), ('laff_expert_stage_train_backward', 18, 43),
    ('laff_gru_pack_whh_t', None, 0), ('laff_gru_gather_rows', None, 0), ('laff_gru_train_reserve_bytes', None, 0),
    ('laff_gru_encode_train', None, 0), ('laff_gru_backward_plan', None, 0), ('laff_gru_backward_workspace_bytes', None, 0),
    ('laff_gru_backward', None, 0),
    ('laff_clip_workspace_bytes', None, 0), ('laff_clip_encode', None, 0),
    ('laff_netvlad_train_reserve_bytes', None, 44), ('laff_netvlad_backward_workspace_bytes', None, 44),
    ('laff_netvlad_encode_train', None, 44), ('laff_netvlad_backward', None, 44),
    ('laff_clip_pack_weight_padded', None, 26), ('laff_clip_image_kpad', None, 26), ('laff_clip_image_workspace_bytes', None, 26),
    ('laff_clip_image_encode', None, 26),
    ('laff_dsl_loss_workspace_bytes', None, 0), ('laff_dsl_loss', None, 0), ('laff_margin_loss_scores', None, 0),
    ('laff_netvlad_workspace_bytes', None, 28), ('laff_netvlad_encode', None, 28),
    ('laff_fc_concat_act_bn', None, 29), ('laff_fc_concat_act_bn_grouped', None, 29),
    ('laff_tile_bn_train_plan', 4, 42), ('laff_tile_bn_train', 18, 42), ('laff_tile_bn_train_backward', 17, 42),
]


@pytest.mark.parametrize('name, nargs, min_abi', ENTRY_POINTS)
def test_entry_point_in_header_library_and_binding_at_the_header_abi(name, nargs, min_abi):
    from laff_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r'^int %s\(' % name, header, flags=re.M) and re.search(r'\b%s\s*\(' % name, header)
    assert hasattr(raw, name) and getattr(raw, name) is not None              # AttributeError if the built library does not export it
    assert name in _lib.SIGNATURES
    if nargs is not None:
        assert len(_lib.SIGNATURES[name][1]) == nargs
    fn = getattr(_lib.load(), name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    abi = re.findall(r'^#define LAFF_ABI_VERSION (\d+)$', header, flags=re.M)
    assert len(abi) == 1 and raw.laff_abi_version() == _lib.load().laff_abi_version() == _lib.ABI_VERSION == int(abi[0]) >= min_abi


def test_coalesce_batches_concatenates_what_a_loader_yields():
    """model.retrieve() runs each tower once over the concatenated batches of any loader (laff_amd/model/model.py, coalesce_batches)."""
    import numpy as np
    import torch
    from laff_amd.model.model import coalesce_batches
    b1 = {'vis_feat_dict': {'a': torch.ones(2, 3), 'b': np.zeros((2, 1), np.float32)}, 'idxs': [0, 1], 'vis_ids': ('v0', 'v1'),
          'vis_frame_feat_dict': {}, 'extra': None}
    b2 = {'vis_feat_dict': {'a': 2 * torch.ones(1, 3), 'b': np.ones((1, 1), np.float32)}, 'idxs': [2], 'vis_ids': ('v2',),
          'vis_frame_feat_dict': {}, 'extra': None}
    out = coalesce_batches([b1, b2])
    assert out['idxs'] == [0, 1, 2] and out['vis_ids'] == ['v0', 'v1', 'v2'] and out['extra'] is None and out['vis_frame_feat_dict'] == {}
    assert out['vis_feat_dict']['a'].shape == (3, 3) and float(out['vis_feat_dict']['a'][2, 0]) == 2.0
    assert out['vis_feat_dict']['b'].tolist() == [[0.0], [0.0], [1.0]]
    assert coalesce_batches([]) is None
    with pytest.raises(ValueError):
        coalesce_batches([{'a': None}, {'b': None}])
    with pytest.raises(ValueError):
        coalesce_batches([None, torch.ones(1)])
    with pytest.raises(TypeError):
        coalesce_batches([3.0, 4.0])
    with pytest.raises(RuntimeError):
        coalesce_batches([torch.ones(2, 3), torch.ones(2, 4)])          # frame tensors padded to different lengths


def test_cpu_tensors_are_refused():
    import torch
    from laff_amd import ops
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fc_act_bn(torch.zeros(4, 8), torch.zeros(16, 8))


def test_missing_library_fails_loudly(tmp_path):
    """No CPU fallback: with the shared library absent the first op raises (checked in a child process)."""
    import subprocess
    import sys
    code = ("import os, sys; os.environ['LAFF_HIP_LIB'] = %r; sys.path.insert(0, %r); "
            "from laff_amd import _lib\n"
            "try:\n    _lib.load()\nexcept RuntimeError as e:\n    assert 'no CPU fallback' in str(e); print('RAISED')\n"
            % (str(tmp_path / 'nope.so'), ROOT))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert 'RAISED' in out.stdout, out.stderr


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under laff_amd/ may import or execute it (tier rule 3)."""
    import glob
    for f in glob.glob(os.path.join(ROOT, 'laff_amd', '**', '*.py'), recursive=True):
        src = open(f).read()
        assert 'import oracle' not in src and 'from oracle' not in src and 'laff_oracle' not in src, f
    for f in glob.glob(os.path.join(ROOT, 'laff_amd', 'csrc', '*')):
        assert 'oracle' not in open(f).read().lower(), f


def test_fc_strip_kernels_keep_out_of_the_accumulator_registers(tmp_path):
    """fc_strip.hip names all 256 accumulator registers literally (the stationary strip).  hipcc must not have put anything of its own
    there -- neither a parked value (v_accvgpr_* outside the asm statements) nor a spill -- and must not have gone to scratch: compile
    the file with -save-temps and audit the ISA of its kernels (tools/debug/isa_audit.py)."""
    import re
    import subprocess
    import sys
    from laff_amd import build
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'fc_strip.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'fc_strip.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'fc_strip_kernel', quiet=True)
    assert len(stats) == 3                                    # the three epilogue kinds
    for name, st in stats.items():
        assert st['acc_outside'] == 0 and st['scratch'] == 0, (name, st)
        assert st['mfma'] == 12 * 48, (name, st)           # the plain loop's four bodies + two tails of four (fc_strip.hip)
    text = open(asm[0]).read()
    for name in stats:
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0


def test_compiler_scheduled_kernels_keep_their_loads_in_flight(tmp_path):
    """Round 6 found hipcc waiting for every load by itself in the C++ kernels (a `global_load` + `s_waitcnt vmcnt(0)` per plane chunk in
    the fusion kernel, per pair of row pieces in the exact re-score) and compiling `__shfl_xor` reductions to the LDS crossbar.  The
    sources are written so that it cannot (raw loads into arrays first; lane swaps + DPP rotations): this holds the ISA to it.
      * fuse_reg_kernel<4, 2>: its eight whole-head plane loads (scalar base, `nt`) come with no vector-memory wait between them;
      * rank_resolve_kernel: somewhere eight 16-byte row loads are issued back to back, no spill;
      * their reductions are DPP row rotations (row_ror), not ds_bpermute_b32."""
    import re
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    from laff_amd import build

    def asm_of(name):
        out = str(tmp_path / (name + '.s'))
        flags = [f for f in build.FLAGS if f != '-fPIC']
        r = subprocess.run([build.hipcc()] + flags + ['--cuda-device-only', '-S', os.path.join(build.CSRC, name + '.hip'), '-o', out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return open(out).read()

    with ThreadPoolExecutor(max_workers=2) as ex:
        fuse, rank = ex.map(asm_of, ['fuse', 'rank'])

    def body(text, mangled_prefix):
        m = re.search(r'^(%s\S*):' % re.escape(mangled_prefix), text, re.M)
        assert m, mangled_prefix
        rest = text[m.end():]
        return [ln.split(';')[0].strip() for ln in rest[:rest.index('.amdhsa_kernel')].split('\n')]

    f42 = [i for i in body(fuse, '_ZN4laff15fuse_reg_kernelILi4ELi2E') if i and not i.startswith('.')]
    # the longest run of nt plane loads with a scalar base that no `s_waitcnt vmcnt` interrupts
    best = run = 0
    for ins in f42:
        if re.match(r'global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\].* nt', ins):
            run += 1
            best = max(best, run)
        elif ins.startswith('s_waitcnt') and 'vmcnt' in ins:
            run = min(run, int(re.search(r'vmcnt\((\d+)\)', ins).group(1)))      # vmcnt(n): the n youngest requests stay in flight
    assert best >= 8, 'fuse_reg_kernel<4, 2>: at most %d plane loads in flight' % best
    assert sum(i.startswith('ds_bpermute') for i in f42) <= 1              # (the several-heads ticket broadcast of the rank side)
    assert sum('row_ror' in i for i in f42) >= 16                          # the reductions' DPP rotations
    res = [i for i in body(rank, '_ZN4laff19rank_resolve_kernel') if i and not i.startswith('.')]
    best = run = 0
    for ins in res:
        if ins.startswith('global_load_dwordx4'):
            run += 1
            best = max(best, run)
        elif ins.startswith('s_waitcnt') and 'vmcnt' in ins:
            run = min(run, int(re.search(r'vmcnt\((\d+)\)', ins).group(1)))
    assert best >= 8, 'rank_resolve_kernel: at most %d row loads issued together' % best
    assert sum(i.startswith('v_mov_b32_dpp') and 'row_ror' in i for i in res) >= 16     # the fp64 group sums travel by DPP
    meta = rank[rank.index('.name:           _ZN4laff19rank_resolve_kernel'):]
    assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0
    meta = fuse[fuse.index('.name:           _ZN4laff15fuse_reg_kernelILi4ELi2E'):]
    assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0


def _build_c_host(out_dir):
    """tests/c_host/laff_host.c: plain C11 against include/laff_hip.h, built with gcc (no hipcc, no torch) and linked to the library."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'tests', 'c_host', 'laff_host.c')
    exe = os.path.join(str(out_dir), 'laff_host')
    libdir = os.path.join(root, 'laff_amd', 'lib')
    cmd = ['gcc', '-std=c11', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include', '-I' + os.path.join(root, 'include'), src,
           '-o', exe, '-L' + libdir, '-llaff_hip', '-L/opt/rocm/lib', '-lamdhip64', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_c_host_builds_against_the_header(tmp_path):
    """The C ABI is bindable from plain C: the host program of tests/c_host compiles with gcc -std=c11 -Werror against the header alone and
    links to liblaff_hip.so (it runs in the GPU suite: test_gpu_kernels.py::test_c_host_runs_the_exact_rank_tail)."""
    from laff_amd import build
    build.build_library(verbose=False)
    exe = _build_c_host(tmp_path)
    assert os.path.exists(exe)
