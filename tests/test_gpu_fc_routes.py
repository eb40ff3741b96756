"""Every FC projection route of the library, element by element against float64 (tests/fc_ref.py).

Part A -- split_rows_kernel<NCH> (fuse.hip) behind laff_split_rows / laff_split_rows_grouped / laff_row_scales_grouped, bit for bit
against fc_ref.split_ref: the hi and lo planes, padding included, and the row scales, read back as raw bits from buffers that held a
poison pattern; every instantiation (NCH = 1, 2, 4, 8, 16 and the generic 0) is named by a case of SPLIT_CASES.

Part B -- the GEMMs behind fc_act_bn_grouped ('fp32'), fc_act_bn_split_grouped ('split') and fc_act_bn_fused_grouped ('fused'), from
the CASES table.  laff_fc_route names the launches an entry point is about to make without making them, so each case first proves
which kernels it checks.  Per case:
  1. Y has row pitch D + pad and is NaN everywhere before the launch; afterwards the pad columns still are, and [N, D] is finite
     except on the planted inf / NaN rows, whose non-finite pattern is the reference's own;
  2. activation None (and relu, which only passes its argument's error on): e = |Y - fc_exact64| / (2^-24 absdot) <=
     EXACT_TOL[route], fc_exact64 being the float64 sum of exactly the products the kernel forms on its operands;
  3. tanh / sigmoid: |Y - fc_exact64| <= ACT_TOL[activation] wherever the pre-activation's absdot is at most ACT_ABSDOT_MAX (every row but
     the planted x 3e4 one, whose unsaturated outputs get ACT_TOL + EXACT_TOL 2^-24 absdot |bn_scale|: slope <= 1);
     and under every activation, None included: |Y - fc_contract64| / (2^-24 absdot_act) <= CONTRACT_TOL[family], fc_contract64 being
     float64 from the fp32 x and W and absdot_act the absdot an activation of slope <= 1 (1/4) leaves, at least the size of its result;
  4. `pair` cases: the fused launch equals the materialised split bit for bit, after the reporter says both run whole big tiles;
  5. a group equals its problems launched one by one bit for bit wherever the reporter gives both the same kernel (whole big tiles
     for X3: a quarter tile is another kernel's tile); the table states per case how many problems that must be (`solo`).
The tail split of X3 depends on the CU count: the x3_* cases build their shapes from laff_device_info and confirm the regime through
the reporter's nbig / quarters.  X3 needs 512 tiles, so the regime 'all tiles in one round' (tiles <= CUs) exists only on a device of
at least 512 CUs; x3_one_round asserts that arithmetic and checks the smallest X3 group in whichever regime it falls.

launch_gemm_nt_grouped_f16 also has a one-plane 256 x 256 branch (LAFF_FC_KERNEL_F16_256).  No FC entry point reaches it: the only
caller, laff_fc_act_bn_split_grouped, builds every problem with three segments, so a big group is always X3 (the fused entry point has
its own launcher).  ops.FC_ROUTES therefore does not list it and ops.fc_route raises if the library ever reports it.
STRIP, GATHER and CONCAT (fc_act_bn_strip_grouped, fc_gather_act_bn, fc_concat_act_bn_grouped) have their own float64 suites
(test_gpu_fc_strip.py, test_gpu_w2vvpp.py); test_other_families_are_named checks the reporter names them."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

import fc_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- Part A ------------------------------------------------------------------------------------------------------------------------
# a matrix: (N, K, view).  view: 'c' contiguous; 'wide' a column window of a wider matrix (row pitch K + 12, window at column 4);
# 'ldodd' row pitch K + 1 (ldx % 4 != 0: generic kernel); 'off' base pointer 4 bytes past a 16-byte boundary (generic kernel).
# NCH is chosen from the largest K of the launch: K <= 256 NCH; anything unaligned or K % 4 != 0 or K > 4096: the generic kernel.
M = namedtuple('M', 'N K view')
SPLIT_CASES = [
    ('nch1_k4_n1', 1, [M(1, 4, 'c')]),
    ('nch1_k256', 1, [M(1003, 256, 'c')]),
    ('nch1_k4_wide', 1, [M(5, 4, 'wide')]),
    ('nch2_k260', 2, [M(5, 260, 'c')]),
    ('nch2_k512_wide', 2, [M(1003, 512, 'wide')]),
    ('nch4_k516', 4, [M(3, 516, 'c')]),
    ('nch4_k1024', 4, [M(1003, 1024, 'wide')]),
    ('nch8_k2048', 8, [M(1003, 2048, 'c')]),
    ('nch16_k2052', 16, [M(5, 2052, 'c')]),
    ('nch16_k4096', 16, [M(1003, 4096, 'wide')]),
    ('gen_k4100', 0, [M(1003, 4100, 'c')]),
    ('gen_k77', 0, [M(1003, 77, 'c')]),
    ('gen_k3981', 0, [M(4, 3981, 'c')]),
    ('gen_ldodd_k512', 0, [M(1003, 512, 'ldodd')]),
    ('gen_off_k256', 0, [M(5, 256, 'off')]),
    # grouped: NCH from the largest K; 9 matrices = a launch of 8 and a launch of 1
    ('group8_nch16', 16, [M(1003, 4, 'c'), M(3, 256, 'wide'), M(1, 260, 'c'), M(5, 512, 'c'), M(4, 1024, 'c'), M(1003, 2052, 'c'),
                          M(3, 4096, 'wide'), M(1, 516, 'c')]),
    ('group8_nch2', 2, [M(1003, 512, 'c'), M(3, 4, 'c'), M(1, 256, 'c'), M(5, 260, 'wide'), M(4, 64, 'c'), M(1003, 96, 'c'),
                        M(3, 32, 'c'), M(1, 512, 'c')]),
    ('group9_generic_then_nch1', 0, [M(1003, 512, 'c'), M(3, 77, 'c'), M(1, 256, 'c'), M(5, 260, 'c'), M(4, 1024, 'c'),
                                     M(1003, 2048, 'c'), M(3, 4100, 'c'), M(1, 516, 'c'), M(1003, 256, 'wide')]),
]


def _matrix(m, seed):
    """The fp32 matrix of M on the device (a view, as M says) with the six planted rows when it has room for them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m.N, m.K, generator=g)
    if m.N >= 6:
        R.plant_rows(x, R.plant_positions(m.N))
    if m.view == 'c':
        return x.to(DEV)
    if m.view == 'wide':
        big = torch.full((m.N, m.K + 12), 7.0, device=DEV)
        v = big[:, 4:4 + m.K]
    elif m.view == 'ldodd':
        big = torch.full((m.N, m.K + 1), 7.0, device=DEV)
        v = big[:, :m.K]
    else:
        flat = torch.full((m.N * m.K + 4,), 7.0, device=DEV)
        v = flat[1:1 + m.N * m.K].view(m.N, m.K)
        assert v.data_ptr() % 16 == 4
    v.copy_(x)
    return v


def _split_launch(ops, xs, scales_only):
    """laff_split_rows_grouped (or laff_row_scales_grouped) on poisoned buffers -> [(planes int16 (2, N, Kp) | None, rscale int32 (N,))]"""
    lib, h = ops._context(torch.device(DEV))
    n = len(xs)
    X, N, K, LD, O, Rs = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    keep = []
    for i, x in enumerate(xs):
        n_, k_ = x.shape
        kp = -(-k_ // 64) * 64
        nbytes = C.c_size_t()
        ops.check(lib.laff_split_rows_bytes(n_, k_, C.byref(nbytes)))
        assert nbytes.value == 2 * n_ * kp * 2
        buf = torch.full((max(nbytes.value, 16),), 0xFD, device=DEV, dtype=torch.uint8)          # 0xFDFD: an fp16 NaN
        rs = torch.full((max(n_, 1),), float('nan'), device=DEV)
        ld = x.stride(0) if n_ > 1 else max(x.stride(0), k_)
        X[i], N[i], K[i], LD[i] = (x.data_ptr() if n_ else None), n_, k_, ld
        O[i], Rs[i] = buf.data_ptr(), (rs.data_ptr() if n_ else None)
        keep.append((buf, rs, n_, kp))
    if scales_only:
        ops.check(lib.laff_row_scales_grouped(h, n, X, N, K, LD, Rs))
    else:
        ops.check(lib.laff_split_rows_grouped(h, n, X, N, K, LD, O, Rs))
    torch.cuda.synchronize()
    out = []
    for buf, rs, n_, kp in keep:
        planes = None if scales_only else buf[:2 * n_ * kp * 2].view(torch.int16).view(2, n_, kp).cpu().numpy()
        if scales_only:
            assert bool((buf == 0xFD).all()), 'the scales-only launch wrote planes'
        out.append((planes, rs[:n_].view(torch.int32).cpu().numpy()))
    return out


def _same_bits(got16, ref):
    nan = np.isnan(ref)
    g = got16.view(np.float16)
    return bool(np.array_equal(np.isnan(g), nan) and np.array_equal(got16[~nan], ref.view(np.int16)[~nan]))


@pytest.mark.parametrize('name,nch,mats', SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_kernel_bit_for_bit(name, nch, mats):
    from laff_amd import ops
    # the instantiation the case is named after (launch_split_rows_grouped's rule, per launch of up to 8 matrices)
    first = mats[:8]
    vec = all(m.K % 4 == 0 and m.view in ('c', 'wide') for m in first)
    kmax = max(m.K for m in first)
    assert nch == (0 if not vec or kmax > 4096 else next(n for n in (1, 2, 4, 8, 16) if kmax <= 256 * n))
    xs = [_matrix(m, 31 * i + len(name)) for i, m in enumerate(mats)]
    got = _split_launch(ops, xs, False)
    # the scales-only form, with an empty matrix (null pointers) among the others
    empty = torch.empty((0, 64), device=DEV)
    scales = _split_launch(ops, xs[:1] + [empty] + xs[1:], True)
    scales = scales[:1] + scales[2:]
    for i, (m, x) in enumerate(zip(mats, xs)):
        hi, lo, rs, _ = R.split_ref(x.cpu().numpy())
        planes, rs_got = got[i]
        assert np.array_equal(rs_got, rs.view(np.int32)), '%s: matrix %d: rscale bits' % (name, i)
        assert _same_bits(planes[0], hi), '%s: matrix %d: hi plane' % (name, i)
        assert _same_bits(planes[1], lo), '%s: matrix %d: lo plane' % (name, i)
        assert np.array_equal(scales[i][1], rs_got), '%s: matrix %d: laff_row_scales_grouped differs' % (name, i)
    # and the single-matrix entry point on the first one
    lib, h = ops._context(torch.device(DEV))
    x = xs[0]
    kp = -(-x.shape[1] // 64) * 64
    buf = torch.full((2 * x.shape[0] * kp * 2,), 0xFD, device=DEV, dtype=torch.uint8)
    rs1 = torch.full((x.shape[0],), float('nan'), device=DEV)
    ld = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])
    ops.check(lib.laff_split_rows(h, C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], ld, C.c_void_p(buf.data_ptr()), C.c_void_p(rs1.data_ptr())))
    assert np.array_equal(buf.view(torch.int16).view(2, x.shape[0], kp).cpu().numpy(), got[0][0])
    assert np.array_equal(rs1.view(torch.int32).cpu().numpy(), got[0][1])


# ---- Part B ------------------------------------------------------------------------------------------------------------------------
# a problem: N, Dk, D, activation, bias / BatchNorm present, the view x is ('c', 'wide': pitch Dk + 8, 'ldodd': pitch Dk + 1, 'off':
# base 4 bytes off, 'span4g': rows 2^18 + 64 floats apart so that N ldx 4 >= 2^32 from 4096 rows on).  The split and fused problems of
# at least fc_ref.PLANT_MIN_ROWS rows carry the six planted rows of Part A.
P = namedtuple('P', 'N Dk D act bias bn view', defaults=(None, True, True, 'c'))
Case = namedtuple('Case', 'name family route problems regime pair solo')


def _c(name, family, route, problems, regime=None, pair=False, solo=0):
    """solo: how many problems of a group check 5 must find comparable with their single launch (the same kernel, whole tiles)."""
    return Case(name, family, tuple(route), problems if callable(problems) else (lambda cus, p=problems: p), regime, pair, solo)


def _x3_rows(cus, rounds_rem):
    """N for D = 512 (two tile columns) such that the group has rounds_rem(cus) tiles of 256 x 256."""
    tiles = rounds_rem(cus)
    assert tiles % 2 == 0 and tiles >= 512
    return tiles // 2 * 256


def _full_rounds(cus):
    return -(-512 // cus) * cus           # the smallest multiple of the CU count that X3 takes


CASES = [
    # ---- fp32 grouped: the staging kind of each problem picks the kernel; launches go kind 2, 1, 0
    _c('f32_reg_dk', 'fp32', ['F32_REG'], [P(300, 514, 260, 'tanh')]),                                      # Dk % 4 != 0
    _c('f32_reg_ldx', 'fp32', ['F32_REG'], [P(1003, 512, 96, None, view='ldodd')]),                        # ldx % 4 != 0
    _c('f32_reg_base', 'fp32', ['F32_REG'], [P(257, 96, 130, 'relu', view='off')]),                        # misaligned base
    _c('f32_tail_k', 'fp32', ['F32_TAIL'], [P(1003, 516, 260, 'sigmoid')]),                                # 2064 bytes % 128 != 0
    _c('f32_tail_span4g', 'fp32', ['F32_TAIL'], [P(4100, 512, 260, None, view='span4g')]),                 # N ldx 4 >= 2^32
    _c('f32_glds_many', 'fp32', ['F32_GLDS'], [P(16384, 512, 2048, 'tanh')]),                              # 128 x 16 = 2048 tiles
    _c('f32_glds_ragged', 'fp32', ['F32_GLDS'], [P(2049, 2048, 260, None, bias=False, bn=False)]),
    _c('f32_glds_n1_d1', 'fp32', ['F32_GLDS'], [P(1, 512, 1, None, bn=False), P(1, 4096, 260, 'relu'), P(1003, 32, 1, None, bias=False)],
       solo=3),
    _c('f32_mixed11', 'fp32', ['F32_GLDS', 'F32_TAIL', 'F32_REG'],
       [P(300, 512, 96, 'tanh'), P(129, 516, 64, None), P(0, 512, 32), P(64, 514, 33, 'relu'), P(1003, 96, 260, 'sigmoid'),
        P(5, 100, 7, None, bias=False), P(200, 77, 40, None, bn=False), P(257, 2080, 128, None), P(1, 36, 5, 'tanh'),
        P(300, 512, 96, None, view='ldodd'), P(130, 4096, 32, None, view='wide')], solo=10),
    _c('f32_glds_9', 'fp32', ['F32_GLDS', 'F32_GLDS'], [P(200 + 31 * i, 512, 64 + 4 * i, (None, 'tanh', 'relu')[i % 3]) for i in range(9)],
       solo=9),
    # ---- split grouped: 128 x 128 tiles below 512 big tiles, the X3 tile from there on
    _c('f16_small', 'split', ['F16_128'], [P(300, 512, 260, 'tanh')]),
    _c('f16_ragged_k77', 'split', ['F16_128'], [P(1003, 77, 130, None)]),
    _c('f16_ragged_k1030', 'split', ['F16_128'], [P(2049, 1030, 520, 'sigmoid', bias=False), P(5, 1030, 33, None, bn=False)],
       solo=2),
    _c('f16_relu_4096', 'split', ['F16_128'], [P(1500, 4096, 512, 'relu')]),
    _c('x3_one_round', 'split', ['X3'], lambda cus: [P(_x3_rows(cus, lambda c: max(512, c)), 512, 512, None)],
       regime='one_round_or_smallest'),
    _c('x3_rem0', 'split', ['X3'], lambda cus: [P(_x3_rows(cus, _full_rounds), 512, 512, 'tanh')], regime='rem0'),
    _c('x3_tail_split', 'split', ['X3'], lambda cus: [P(_x3_rows(cus, lambda c: _full_rounds(c) + c // 2) - 100, 512, 512, None)],
       regime='split'),
    _c('x3_tail_kept', 'split', ['X3'], lambda cus: [P(_x3_rows(cus, lambda c: _full_rounds(c) + c // 8 * 7) - 3, 512, 512, 'relu')],
       regime='kept'),
    _c('x3_d260_k96', 'split', ['X3'], [P(65536, 96, 260, None, bias=False, bn=False)]),
    _c('x3_d520_k2080', 'split', ['X3'], [P(43777, 2080, 520, 'sigmoid')]),
    _c('x3_n1_inside', 'split', ['X3'], [P(40000, 512, 512, None), P(1, 512, 512, 'tanh'), P(30001, 512, 260, None, bn=False),
                                         P(5, 96, 33, 'relu')]),
    _c('x3_9_problems', 'split', ['X3', 'F16_128'], [P(15000 + 7 * i, 512, 512 if i % 2 else 260, (None, 'tanh')[i % 2]) for i in range(9)],
       solo=1),
    # x3_n1_inside: every single launch is F16_128; x3_9_problems: only the trailing one-problem launch is comparable.  X3's share of
    # check 5 is x3_pair_groups: two problems of whole rounds each, X3 alone and together.
    _c('x3_pair_groups', 'split', ['X3'], lambda cus: [P(_x3_rows(cus, _full_rounds), 96, 512, None), P(_x3_rows(cus, _full_rounds), 96, 512, 'tanh')],
       solo=2),
    # ---- fused grouped: always the X3 tile, the input split on its way into LDS; Dk % 32 == 0, so Kp > Dk at 32, 96, 2080
    _c('fused_small_300', 'fused', ['X3_FUSED'], [P(300, 96, 260, 'tanh')]),
    _c('fused_dk32_d32', 'fused', ['X3_FUSED'], [P(1003, 32, 32, None)]),
    _c('fused_dk2080_wide', 'fused', ['X3_FUSED'], [P(2049, 2080, 1024, 'relu', view='wide')]),
    _c('fused_dk4096', 'fused', ['X3_FUSED'], [P(1500, 4096, 512, 'sigmoid')]),
    _c('fused_dk512_group', 'fused', ['X3_FUSED'], [P(1003, 512, 512, None, bias=False, bn=False), P(300, 512, 260, None, bn=False),
                                                    P(1, 512, 32, 'tanh'), P(2000, 32, 1024, None, bias=False)],
       solo=4),
    _c('fused_big_dk2048', 'fused', ['X3_FUSED'], lambda cus: [P(_x3_rows(cus, _full_rounds), 2048, 512, None)], pair=True),
    _c('fused_big_dk96_d260', 'fused', ['X3_FUSED'], lambda cus: [P(_x3_rows(cus, _full_rounds), 96, 260, 'tanh', view='wide')], pair=True),
    _c('fused_big_dk2080_d1024', 'fused', ['X3_FUSED'], lambda cus: [P(_x3_rows(cus, _full_rounds) // 2, 2080, 1024, None)], pair=True),
]


def test_table_covers_every_route():
    from laff_amd import ops
    assert {r for c in CASES for r in c.route} == set(ops.FC_ROUTES) - {'STRIP', 'GATHER', 'CONCAT'}
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.regime for c in CASES if c.regime} == {'one_round_or_smallest', 'rem0', 'split', 'kept'}
    for fam in ('fp32', 'split', 'fused'):          # every activation, and the three partial epilogues, on every family
        ps = [p for c in CASES if c.family == fam for p in c.problems(256)]
        assert {p.act for p in ps} == set(R.ACTS)
        assert {(p.bias, p.bn) for p in ps} >= {(False, False), (True, False), (False, True), (True, True)}
    assert set(R.EXACT_TOL) == {r for c in CASES for r in c.route}
    assert set(R.CONTRACT_TOL) == {c.family for c in CASES}


def test_other_families_are_named():
    from laff_amd import ops
    for fam, k in (('strip', 'STRIP'), ('gather', 'GATHER'), ('concat', 'CONCAT')):
        assert ops.fc_route(fam, [dict(N=8, Dk=512, D=32)]).kernels == [k]


def _cus(ops):
    lib, h = ops._context(torch.device(DEV))
    info = (C.c_int * 4)()
    ops.check(lib.laff_device_info(h, info))
    return int(info[0])


def _x_view(p, x):
    N, Dk = p.N, p.Dk
    if p.view == 'c' or N == 0:
        return x.to(DEV)
    if p.view == 'off':
        flat = torch.zeros((N * Dk + 4,), device=DEV)
        v = flat[1:1 + N * Dk].view(N, Dk)
    else:
        pitch = {'wide': Dk + 8, 'ldodd': Dk + 1, 'span4g': (1 << 18) + 64}[p.view]
        v = torch.empty((N, pitch), device=DEV)[:, :Dk]
    v.copy_(x)
    return v


def _shape(p, x):
    return dict(N=p.N, Dk=p.Dk, D=p.D, ldx=(x.stride(0) if p.N > 1 else max(x.stride(0), p.Dk)), ldw=p.Dk,
                x_aligned=x.data_ptr() % 16 == 0 or p.N == 0)


def _nan_out(p, i):
    pad = 4 if i % 2 == 0 else 1
    full = torch.full((max(p.N, 1), p.D + pad), float('nan'), device=DEV)
    return full, full[:p.N, :p.D]


def _decode(so):
    kp = -(-so.K // 64) * 64
    h = so.buf.view(torch.float16)
    return h[:so.N * kp].view(so.N, kp), h[so.N * kp:2 * so.N * kp].view(so.N, kp), so.rscale[:so.N]


def _launch(ops, family, items):
    """items: dicts with x, w, ws (SplitOperand of w), xs (SplitOperand of x, split family), b, sc, sh, act, out."""
    if family == 'fp32':
        ops.fc_act_bn_grouped([dict(x=q['x'], weight=q['w'], bias=q['b'], bn_scale=q['sc'], bn_shift=q['sh'], activation=q['act'],
                                    out=q['out']) for q in items])
    elif family == 'split':
        ops.fc_act_bn_split_grouped([dict(x=q['xs'], weight_split=q['ws'], bias=q['b'], bn_scale=q['sc'], bn_shift=q['sh'],
                                          activation=q['act'], out=q['out']) for q in items])
    else:
        ops.fc_act_bn_fused_grouped([dict(x=q['x'], weight_split=q['ws'], bias=q['b'], bn_scale=q['sc'], bn_shift=q['sh'],
                                          activation=q['act'], out=q['out']) for q in items])
    torch.cuda.synchronize()


def _same(a, b):
    return bool(torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0)))


def _regime(cus, tiles):
    rem = tiles % cus
    if tiles <= cus:
        return 'one_round'
    if rem == 0:
        return 'rem0'
    return 'split' if rem * 4 <= 3 * cus else 'kept'


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_fc_route_vs_float64(c):
    from laff_amd import ops
    cus = _cus(ops)
    probs = c.problems(cus)
    split = c.family != 'fp32'
    items = []
    for i, p in enumerate(probs):
        plant = split and p.N >= R.PLANT_MIN_ROWS
        x, w, b, sc, sh = R.make_problem(p.N, p.Dk, p.D, 17 * i + p.N + p.Dk + p.D, p.bias, p.bn, plant)
        q = dict(p=p, x=_x_view(p, x), w=w.to(DEV), b=None if b is None else b.to(DEV), sc=None if sc is None else sc.to(DEV),
                 sh=None if sh is None else sh.to(DEV), act=p.act)
        items.append(q)
    if split:
        for q, so in zip(items, ops.split_rows_grouped([q['w'] for q in items])):
            q['ws'] = so
    if c.family == 'split':
        for q, so in zip(items, ops.split_rows_grouped([q['x'] for q in items])):
            q['xs'] = so

    # which kernels are about to run
    shapes = [_shape(q['p'], q['x']) for q in items]
    route = ops.fc_route(c.family, shapes)
    assert tuple(route.kernels) == c.route, route.launches
    assert route.kernels == ops.fc_route(c.family, [dict(x=q['x'], weight=q['w']) for q in items]).kernels      # from the tensors
    for i, p in enumerate(probs):
        assert (route.launch_of[i] is None) == (p.N == 0)
    assert all(len(l['problems']) <= 8 for l in route.launches)
    if c.family == 'fp32':
        assert [route.kinds[i] for i, p in enumerate(probs) if p.N] == \
            [{'F32_REG': 0, 'F32_TAIL': 1, 'F32_GLDS': 2}[route.launches[route.launch_of[i]]['kernel']] for i, p in enumerate(probs) if p.N]
    if c.regime:
        l = route.launches[0]
        assert l['tiles'] >= 512
        want = _regime(cus, l['tiles'])
        if c.regime == 'one_round_or_smallest':
            assert (want == 'one_round') == (cus >= 512)        # 512 tiles never fit one round of fewer than 512 CUs
            assert l['tiles'] == max(512, cus)
        else:
            assert want == c.regime
        rem = l['tiles'] % cus
        assert (l['nbig'], l['quarters']) == ((l['tiles'] - rem, 4 * rem) if want == 'split' else (l['tiles'], 0))

    outs = [_nan_out(q['p'], i) for i, q in enumerate(items)]
    for q, (full, view) in zip(items, outs):
        q['out'] = view
    _launch(ops, c.family, items)

    for i, (q, (full, Y)) in enumerate(zip(items, outs)):
        p = q['p']
        if p.N == 0:
            assert bool(full.isnan().all())
            continue
        kernel = route.launches[route.launch_of[i]]['kernel']
        assert bool(full[:, p.D:].isnan().all()), 'problem %d: a pad column of Y was written' % i
        if c.family == 'split':
            xo, wo = _decode(q['xs']), _decode(q['ws'])
        elif c.family == 'fused':
            xo, wo = R.split_ref_t(q['x']), _decode(q['ws'])
        e_exact = e_contract = a_err = a_big = 0.0
        for a in range(0, p.N, 8192):
            b_ = min(a + 8192, p.N)
            xa = q['x'][a:b_]
            if split:
                ref = R.fc_exact64(tuple(t[a:b_] for t in xo), wo, q['b'], p.act, q['sc'], q['sh'])
            else:
                ref = R.fc_exact64(xa, q['w'], q['b'], p.act, q['sc'], q['sh'])
            got = Y[a:b_]
            fin = torch.isfinite(ref)
            assert torch.equal(torch.isfinite(got), fin), 'problem %d: finite pattern differs from the reference' % i
            assert torch.equal(got.isnan(), ref.isnan()) and torch.equal(got[~fin & ~ref.isnan()].double(), ref[~fin & ~ref.isnan()])
            if not split:
                assert bool(fin.all())
            # the contract, whatever the activation: tanh / sigmoid pass the pre-activation's error on through a slope <= 1 (1/4)
            con = R.fc_contract64(xa, q['w'], q['b'], p.act, q['sc'], q['sh'])
            adc = R.absdot_act(xa, q['w'], q['b'], p.act, q['sc'], q['sh'])
            e_contract = max(e_contract, R.norm_err(got, torch.where(fin, con, torch.full_like(con, float('nan'))), adc))
            if p.act in (None, 'relu'):         # relu passes its argument's error on (or drops it): the same normalised bounds
                e_exact = max(e_exact, R.norm_err(got, ref, adc))
            else:
                # tanh / sigmoid: absolute, where the pre-activation's absdot is of ordinary size; on a row of huge entries (the planted
                # x 3e4 row) an unsaturated output carries the pre-activation's error, which scales with absdot (slope <= 1)
                adp = R.absdot(xa, q['w'], q['b'])
                err = (got.double() - ref).abs()
                small = fin & (adp <= R.ACT_ABSDOT_MAX)
                if bool(small.any()):
                    a_err = max(a_err, float(err[small].max()))
                big = fin & ~small
                if bool(big.any()):
                    lim = R.ACT_TOL[p.act] + R.EXACT_TOL[kernel] * R.U * (adp if q['sc'] is None else adp * q['sc'].double().abs()[None, :])
                    a_big = max(a_big, float((err[big] / lim[big]).max()))
        print('FCMEASURE case=%s problem=%d kernel=%s family=%s N=%d K=%d D=%d act=%s exact=%.4g contract=%.4g act_abs=%.4g act_big=%.4g' % (
            c.name, i, kernel, c.family, p.N, p.Dk, p.D, p.act, e_exact, e_contract, a_err, a_big))
        q['e'] = (kernel, e_exact, e_contract, a_err, a_big)
    for q in items:
        if q['p'].N == 0:
            continue
        kernel, e_exact, e_contract, a_err, a_big = q['e']
        assert e_exact <= R.EXACT_TOL[kernel]
        assert e_contract <= R.CONTRACT_TOL[c.family]
        assert a_err <= R.ACT_TOL.get(q['p'].act, 0.0)
        assert a_big <= 1.0

    # 4. fused == materialised split, bit for bit, where both run whole big tiles
    if c.pair:
        sr = ops.fc_route('split', shapes)
        assert sr.kernels == ['X3'] and sr.launches[0]['quarters'] == 0 and route.kernels == ['X3_FUSED']
        twin = [dict(q, xs=so, out=_nan_out(q['p'], i)[1]) for i, (q, so) in
                enumerate(zip(items, ops.split_rows_grouped([q['x'] for q in items])))]
        _launch(ops, 'split', twin)
        for q, t in zip(items, twin):
            assert _same(q['out'], t['out']), 'fused and materialised split differ'

    # 5. the group == its problems one by one, bit for bit, where the reporter gives both the same kernel
    if len([p for p in probs if p.N]) > 1:
        compared = 0
        for i, q in enumerate(items):
            if q['p'].N == 0:
                continue
            one = ops.fc_route(c.family, [shapes[i]]).launches[0]
            grp = route.launches[route.launch_of[i]]
            if one['kernel'] != grp['kernel'] or one['quarters'] or grp['quarters']:
                continue
            solo = dict(q, out=_nan_out(q['p'], i)[1])
            _launch(ops, c.family, [solo])
            assert _same(solo['out'], q['out']), 'problem %d: grouped and single launches differ' % i
            compared += 1
        print('FCMEASURE case=%s grouped == single on %d problems' % (c.name, compared))
        assert compared == c.solo, 'check 5 compared %d problems, the table says %d' % (compared, c.solo)
    else:
        assert c.solo == 0
    items.clear()
    del outs
    torch.cuda.empty_cache()                # the 4 GiB-span input goes back at once
