"""Every kernel behind laff_fuse / laff_fuse_packed_rank / laff_frame_fuse, element by element against float64 (tests/fuse_ref.py).

launch_fuse_L (laff_amd/csrc/fuse.hip) picks fuse_reg_kernel<L, 1> for d <= 256, <L, 2> for d <= 512 and fuse_stream_kernel<L> above,
for L = 1..8; inside fuse_reg_kernel whole heads (d == 256 NCH) and ragged heads take different load paths, for dense and for gather
planes; gather planes switch the grid to head-major.  launch_frame_fuse picks frame_fuse_kernel<1 | 2 | 4>, whose waves fold their
frames in batches of 8 / NCH.  Every case below names the kernel and load path the dispatch gives it, and test_table_covers_every_kernel
proves that the table reaches all of them.  Per case:
  1. E against the float64 restatement (unit-norm outputs absolutely; JUST_AVERAGE rows relative to their magnitude), the softmax
     weights where requested;
  2. the packed 16-bit operand bit for bit: round to nearest of the kernel's own E times the prescale;
  3. with rank_side (laff_rank_prepare's work riding in the fuse launches): s_gt64 bit-equal to laff_rank_prepare's, the bands no
     narrower than its bands and equal to rounding, the count / list header cleared, the float64 counts after the banded pipeline.
Every output buffer is NaN before its launch: a row the kernel skipped cannot pass on what an earlier launch left there."""
from collections import namedtuple

import pytest
import torch

import fuse_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# Bounds against float64, set from the maxima measured on the MI355X (in brackets).
TOL_UNIT = 1.5e-6    # unit-norm E [1.11e-6]
TOL_JAVG = 2e-7      # JUST_AVERAGE E, relative to the l2 norm of its (row, head) [1.17e-7]
TOL_WEIGHTS = 1e-6   # softmax weights [8.6e-7]
TOL_FRAMES = 4e-7    # frame attention output, unit norm [2.5e-7]
# Weights next to logits of ~100 carry the fp32 rounding of the logit itself: one ulp there is 7.6e-6, and a weight a moves by up to
# a (1 - a) times it (2.0e-6 measured over 4097 rows).  So the big-logit cases with thousands of rows check E only, and those that
# check weights have a few rows.

Case = namedtuple('Case', 'name kernel L H d N planes flags prec')
# planes, one letter per plane:
#   D  dense, split heads (or the shared row without split heads), a strided view (ld > width)
#   T  tiled over the heads (one d-wide row) with a folded affine over the H * d columns, strided
#   A  dense with a deferred activation (tanh / relu / sigmoid, by plane index) and a folded affine, strided
#   G  gather CSR through its FC (bias, activation, affine); rows of 0 .. ~200 ids, out-of-range ids among them
# flags: ave (WITH_AVE), mul (MUL), l2h (L2NORM_EACH_HEAD), javg (JUST_AVERAGE), nosplit (NO_SPLIT_HEAD), rownorm (l2norm_planes),
#   big (logits above 90: the softmax needs its max subtraction), w (return and check the softmax weights)
# kernel: what launch_fuse_L picks -- reg1 / reg2 (fuse_reg_kernel<L, 1 | 2>) with its load path (whole: d == 256 NCH, lane: the
#   per-lane col < d path), or stream (fuse_stream_kernel<L>)
CASES = [
    Case('r1_L1_d4', 'reg1/lane', 1, 1, 4, 1, 'D', {'ave', 'w'}, 'fp16'),
    Case('r1_L2_d256_gather', 'reg1/whole', 2, 2, 256, 4097, 'GT', {'mul', 'big'}, 'bf16'),
    Case('r1_L3_d36_gather', 'reg1/lane', 3, 3, 36, 2, 'ADG', {'ave', 'mul', 'l2h', 'w'}, 'fp16'),
    Case('r1_L4_d252_javg', 'reg1/lane', 4, 8, 252, 3, 'TADG', {'javg'}, None),
    Case('r1_L5_d256_nosplit', 'reg1/whole', 5, 3, 256, 4097, 'DADAD', {'nosplit', 'l2h', 'ave', 'rownorm'}, 'fp16'),
    Case('r1_L6_d36_40k_items', 'reg1/lane', 6, 2, 36, 20001, 'GDADTD', {'ave', 'w'}, 'bf16'),          # 40002 items, % 4 == 2
    Case('r1_L7_d252_big', 'reg1/lane', 7, 2, 252, 1, 'DTAGDTA', {'mul', 'big', 'w'}, 'fp16'),
    Case('r1_L8_d4_javg', 'reg1/lane', 8, 3, 4, 3, 'DADADADA', {'rownorm', 'l2h', 'javg'}, None),
    Case('r2_L1_d512_gather', 'reg2/whole', 1, 8, 512, 3, 'G', {'ave', 'w'}, 'fp16'),
    Case('r2_L2_d260_javg', 'reg2/lane', 2, 1, 260, 4097, 'DA', {'javg', 'rownorm'}, None),
    Case('r2_L3_d384_big', 'reg2/lane', 3, 2, 384, 1, 'TGD', {'mul', 'big', 'w'}, 'bf16'),
    Case('r2_L4_d508', 'reg2/lane', 4, 3, 508, 2, 'ADTG', {'ave', 'mul', 'l2h', 'w'}, 'fp16'),
    Case('r2_L5_d512_nosplit_big', 'reg2/whole', 5, 2, 512, 3, 'DADAD', {'nosplit', 'big', 'ave', 'w'}, 'bf16'),
    Case('r2_L6_d508_gather', 'reg2/lane', 6, 1, 508, 4097, 'GADTDA', {'l2h'}, 'fp16'),
    Case('r2_L7_d260_rownorm', 'reg2/lane', 7, 8, 260, 2, 'DADTDAD', {'rownorm', 'ave', 'mul', 'w'}, 'bf16'),
    Case('r2_L8_d512_javg_gather', 'reg2/whole', 8, 2, 512, 1, 'GDTADTAD', {'javg', 'l2h'}, None),
    Case('s_L1_d516', 'stream', 1, 2, 516, 3, 'A', {'mul', 'l2h', 'w'}, 'fp16'),
    Case('s_L2_d2048_big', 'stream', 2, 1, 2048, 4097, 'DT', {'ave', 'big'}, 'bf16'),
    Case('s_L3_d1000_javg_nosplit', 'stream', 3, 3, 1000, 1, 'DAD', {'nosplit', 'javg', 'l2h'}, None),
    Case('s_L4_d516_rownorm', 'stream', 4, 8, 516, 2, 'TADT', {'rownorm', 'mul', 'w'}, 'fp16'),
    Case('s_L5_d1000_javg', 'stream', 5, 1, 1000, 4097, 'ADTDA', {'javg'}, None),
    Case('s_L6_d2048', 'stream', 6, 3, 2048, 3, 'DTADTA', {'ave', 'mul', 'l2h', 'big', 'w'}, 'bf16'),
    Case('s_L7_d1000_rownorm', 'stream', 7, 2, 1000, 2, 'DADTDAD', {'l2h', 'rownorm', 'ave', 'w'}, 'fp16'),
    Case('s_L8_d516_nosplit_big', 'stream', 8, 2, 516, 1, 'DADADADA', {'nosplit', 'big', 'w'}, 'fp16'),
]

# laff_fuse_packed_rank: videos first, then texts whose first plane is a gather plane ('G') or dense ('D')
RankCase = namedtuple('RankCase', 'name kernel H d text prec')
RANK_CASES = [
    RankCase('rank_r1_whole_h8_gather', 'reg1/whole', 8, 256, 'G', 'fp16'),
    RankCase('rank_r1_lane_h1_dense', 'reg1/lane', 1, 252, 'D', 'bf16'),
    RankCase('rank_r2_whole_h1_gather', 'reg2/whole', 1, 512, 'G', 'bf16'),
    RankCase('rank_r2_lane_h8_dense', 'reg2/lane', 8, 260, 'D', 'fp16'),
    RankCase('rank_r1_lane_h8_gather', 'reg1/lane', 8, 36, 'G', 'bf16'),
]

# frame_fuse_kernel<NCH>: mode lens / mask (a view of a (B, Fmax + 5) buffer) / full; count features in one grouped launch
FrameCase = namedtuple('FrameCase', 'name nch Fmax d mode attention count')
FRAME_CASES = [
    FrameCase('f1_d36_lens', 1, 1, 36, 'lens', 'attention_noAveNoAverageMul', 1),
    FrameCase('f5_d516_mask', 4, 5, 516, 'mask', 'average_AverageMul_noAve', 2),
    FrameCase('f31_d384_full', 2, 31, 384, 'full', 'attention_noAverageMul_Ave', 3),
    FrameCase('f32_d256_lens', 1, 32, 256, 'lens', 'attention_averageMul', 4),
    FrameCase('f33_d4_mask', 1, 33, 4, 'mask', 'attention_averageMul', 1),
    FrameCase('f33_d508_lens', 2, 33, 508, 'lens', 'attention_noAveNoAverageMul', 2),
    FrameCase('f65_d1000_lens', 4, 65, 1000, 'lens', 'attention_noAverageMul_Ave', 1),
    FrameCase('f65_d252_full', 1, 65, 252, 'full', 'average_AverageMul_noAve', 3),
    FrameCase('f100_d512_mask', 2, 100, 512, 'mask', 'attention_averageMul', 4),
    FrameCase('f100_d36_lens_big', 1, 100, 36, 'lens', 'attention_noAverageMul_Ave', 2),
    FrameCase('f33_d1000_full', 4, 33, 1000, 'full', 'attention_noAveNoAverageMul', 1),
    FrameCase('f100_d260_full', 2, 100, 260, 'full', 'average_AverageMul_noAve', 2),
]

GATHER_COUNTS = (0, 1, 3, 63, 64, 65, 203)      # ids per caption, cycled over the rows (the 64-id loop: one trip, two, four)
ACTS = ('tanh', 'relu', 'sigmoid')


def _dispatch(d):
    """launch_fuse_L's pick (fuse.hip), with fuse_reg_kernel's load path."""
    if d <= 512:
        nch = 1 if d <= 256 else 2
        return 'reg%d/%s' % (nch, 'whole' if d == 256 * nch else 'lane')
    return 'stream'


def _frame_nch(d):
    return 1 if d <= 256 else 2 if d <= 512 else 4


def _frame_lengths(c, B):
    """Per video: 0, 1, 3, 4, Fmax - 1, Fmax, then a spread (clamped to [0, Fmax])."""
    base = [0, 1, 3, 4, c.Fmax - 1, c.Fmax] + [(7 * i + 3) % (c.Fmax + 1) for i in range(B - 6)]
    return [max(0, min(c.Fmax, v)) for v in base]


def _gather_counts(N, salt):
    return [GATHER_COUNTS[(n + salt) % len(GATHER_COUNTS)] for n in range(N)]


def test_table_covers_every_kernel():
    names = [c.name for c in CASES + RANK_CASES + FRAME_CASES]
    assert len(set(names)) == len(names)
    for c in CASES + RANK_CASES:
        assert c.kernel == _dispatch(c.d), c.name
    pairs = {(c.L, c.kernel.split('/')[0]) for c in CASES}
    assert pairs == {(L, k) for L in range(1, 9) for k in ('reg1', 'reg2', 'stream')}
    assert {c.kernel for c in CASES} == {'reg1/whole', 'reg1/lane', 'reg2/whole', 'reg2/lane', 'stream'}
    # both load paths of both reg widths with dense planes only and with a gather plane
    for k in ('reg1/whole', 'reg1/lane', 'reg2/whole', 'reg2/lane'):
        assert any(c.kernel == k and 'G' in c.planes for c in CASES), k
        assert any(c.kernel == k and 'G' not in c.planes for c in CASES), k
    ids = set()
    for c in CASES:
        if 'G' in c.planes:
            ids |= set(_gather_counts(c.N, c.L))
    assert ids == set(GATHER_COUNTS)
    for f in ('ave', 'mul', 'l2h', 'javg', 'nosplit', 'rownorm', 'big'):
        assert any(f in c.flags for c in CASES), f
    assert {c.kernel[:4] for c in CASES if {'big', 'w'} <= c.flags} == {'reg1', 'reg2', 'stre'}
    assert any('javg' in c.flags and c.kernel == 'stream' for c in CASES)
    assert {c.d for c in CASES} == {4, 36, 252, 256, 260, 384, 508, 512, 516, 1000, 2048}
    assert {c.H for c in CASES if 'nosplit' not in c.flags} >= {1, 2, 3, 8} and any(c.H > 1 for c in CASES if 'nosplit' in c.flags)
    assert {1, 2, 3, 4097} <= {c.N for c in CASES}
    assert any(c.N * c.H >= 10000 and c.N * c.H % 4 for c in CASES)
    # rank_side: NCH 1 and 2, whole and ragged, H 1 and 8, dense and gather text planes
    assert {c.kernel for c in RANK_CASES} == {'reg1/whole', 'reg1/lane', 'reg2/whole', 'reg2/lane'}
    assert {c.H for c in RANK_CASES} == {1, 8} and {c.text for c in RANK_CASES} == {'G', 'D'}
    for k in ('reg1', 'reg2'):
        assert {c.text for c in RANK_CASES if c.kernel.startswith(k)} == {'G', 'D'}
    # frames: every width, each with a video that takes more than one batch trip of 4 waves x (8 / NCH) frames
    from oracle import laff_oracle as O
    for c in FRAME_CASES:
        assert c.nch == _frame_nch(c.d), c.name
    for nch in (1, 2, 4):
        trip = 4 * (8 // nch)
        assert any(c.nch == nch and max(_frame_lengths(c, 37)) > trip for c in FRAME_CASES), nch
    assert {c.Fmax for c in FRAME_CASES} == {1, 5, 31, 32, 33, 65, 100}
    assert {c.mode for c in FRAME_CASES} == {'lens', 'mask', 'full'}
    assert {c.attention for c in FRAME_CASES} == set(O.FRAME_ATTENTION_FLAGS)
    assert {c.count for c in FRAME_CASES} == {1, 2, 3, 4}


def _strided(g, N, width, scale=1.0):
    """An (N, width) view into a wider buffer: row pitch width + 8, first column 4 floats in (16-byte aligned)."""
    buf = torch.randn(N, width + 8, generator=g, device=DEV) * scale
    return buf[:, 4:4 + width]


def _gather(g, N, H, d, salt):
    """A CSR of GATHER_COUNTS ids per row over a vocabulary of Dk; every row of 3 or more ids holds out-of-range ids too.  The FC's
    weight_t is a view with a wider pitch."""
    Dk = 3000
    counts = _gather_counts(N, salt)
    crow = torch.zeros(N + 1, dtype=torch.int32)
    crow[1:] = torch.cumsum(torch.tensor(counts), 0)
    nnz = int(crow[-1])
    idx = torch.randint(0, Dk, (nnz,), generator=torch.Generator().manual_seed(salt))
    for n, k in enumerate(counts):
        if k >= 3:
            p = int(crow[n])
            idx[p], idx[p + k // 2], idx[p + k - 1] = -1, Dk, Dk + 17
    val = torch.rand(nnz, generator=g, device=DEV) * 2 + 0.25
    csr = torch.sparse_csr_tensor(crow.to(DEV), idx.to(torch.int32).to(DEV), val, size=(N, Dk))
    wt = (torch.randn(Dk, H * d + 12, generator=g, device=DEV) * 0.1)[:, :H * d]
    bias = torch.randn(H * d, generator=g, device=DEV) * 0.1
    return csr, wt, bias, (crow, idx, val)


def _planes(c, g):
    """ops.fuse planes of case c and their float64 restatement (N, L, H, d)."""
    split = 'nosplit' not in c.flags
    H, d, N = c.H, c.d, c.N
    width = H * d if split else d
    planes, ref = [], []
    for l, k in enumerate(c.planes):
        act = ACTS[l % 3]
        if k == 'D':
            x = _strided(g, N, width)
            planes.append((x, False, None, None))
            ref.append(R.dense_plane(x, H, d, split_head=split))
        elif k == 'T':
            x = _strided(g, N, d)
            sc = torch.rand(H * d, generator=g, device=DEV) + 0.5
            sh = torch.randn(H * d, generator=g, device=DEV) * 0.1
            planes.append((x, True, sc, sh))
            ref.append(R.dense_plane(x, H, d, tile=True, scale=sc, shift=sh))
        elif k == 'A':
            x = _strided(g, N, width, 1.5)
            sc = torch.rand(width, generator=g, device=DEV) + 0.5
            sh = torch.randn(width, generator=g, device=DEV) * 0.1
            planes.append((x, False, sc, sh, act))
            ref.append(R.dense_plane(x, H, d, split_head=split, scale=sc, shift=sh, act=act))
        else:
            csr, wt, bias, (crow, idx, val) = _gather(g, N, H, d, c.L + l)
            sc = torch.rand(H * d, generator=g, device=DEV) + 0.5
            sh = torch.randn(H * d, generator=g, device=DEV) * 0.1
            planes.append((None, False, sc, sh, act, (csr, wt, bias)))
            ref.append(R.gather_plane(crow, idx, val, wt, H, d, bias, sc, sh, act))
    if 'rownorm' in c.flags:
        ref = [p * R.row_scale(p, split) for p in ref]
    return planes, torch.stack(ref, 1)


def _attention_params(g, H, d, big):
    w = torch.randn(H, d, generator=g, device=DEV) / d ** 0.5
    b = torch.randn(H, generator=g, device=DEV) * 0.3
    if big:                                    # logits of 90 .. 110: exp() of them overflows fp32 without the max subtraction
        w = w * 4.0
        b = b + 100.0
    gw = torch.rand(H, generator=g, device=DEV)
    return w, b, gw


def _nan(shape):
    return torch.full(shape, float('nan'), device=DEV)


def _packed_bits_equal(E, P, prec):
    """The operand is round to nearest of (E * prescale), bit for bit."""
    dt = torch.float16 if prec == 'fp16' else torch.bfloat16
    n = E.numel()
    got = P.buf[:2 * n].view(torch.int16)
    want = (E.reshape(-1) * P.prescale).to(dt).view(torch.int16)
    return torch.equal(got, want)


def _flags(ops, c):
    return ops.attention_flags('ave' in c.flags, 'mul' in c.flags, 'l2h' in c.flags, 'nosplit' not in c.flags, 'javg' in c.flags)


def _check_E(E, ref, javg):
    assert bool(torch.isfinite(E).all()), 'an element the kernel did not write'
    diff = (E.double() - ref).abs().amax(2)
    if javg:
        return float((diff / (ref.pow(2).sum(2).sqrt() + 1e-30)).max())
    return float(diff.max())


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_fuse_vs_float64(c):
    from laff_amd import ops
    g = torch.Generator(device=DEV).manual_seed(1000 * c.L + c.d + c.N)
    planes, X = _planes(c, g)
    w, b, gw = _attention_params(g, c.H, c.d, 'big' in c.flags)
    javg = 'javg' in c.flags
    want_w = 'w' in c.flags
    E = _nan((c.N, c.H, c.d))
    aw = _nan((c.N, c.H, c.L)) if want_w else None
    pk = torch.full((c.N * c.H * c.d * 2 + 16,), 0xff, dtype=torch.uint8, device=DEV) if c.prec else None
    out = ops.fuse(planes, c.H, c.d, None if javg else w, None if javg else b, gw, _flags(ops, c), return_weights=want_w,
                   packed_precision=c.prec, l2norm_planes='rownorm' in c.flags, out=E, weights_out=aw, packed_out=pk)
    out = out if isinstance(out, tuple) else (out,)
    assert out[0] is E
    ref, a_ref = R.attention(X, w, b, gw, 'ave' in c.flags, 'mul' in c.flags, 'l2h' in c.flags, javg)
    if 'big' in c.flags:             # every (row, head) has a logit above 90: exp() of it is beyond fp32
        assert float(R.logits(X, w, b, 'mul' in c.flags, 'l2h' in c.flags).amax(2).min()) > 90.0
    err = _check_E(E, ref, javg)
    err_w = 0.0
    if want_w:
        assert out[1] is aw and bool(torch.isfinite(aw).all())
        err_w = float((aw.double() - a_ref).abs().max())
    if c.prec:
        assert out[-1].buf is pk
        assert _packed_bits_equal(E, out[-1], c.prec), 'the packed operand is not round-to-nearest of E * prescale'
        assert bool((pk[c.N * c.H * c.d * 2:] == 0xff).all()), 'written past the operand'
    print('%s: %s  max|E - f64| %.3e%s  max|w - f64| %.3e' % (c.name, c.kernel, err, ' (relative)' if javg else '', err_w))
    assert err <= (TOL_JAVG if javg else TOL_UNIT)
    assert err_w <= TOL_WEIGHTS


def _count_f64(Et, Ev, gt):
    """Float64 ranks of the fp32 embeddings: videos scoring above the ground truth (per-head cosine, mean over heads)."""
    H = Et.shape[1]
    t, v = Et.double(), Ev.double()
    t = t / (t.pow(2).sum(-1, keepdim=True).sqrt() + R.NORM_EPS)
    v = v / (v.pow(2).sum(-1, keepdim=True).sqrt() + R.NORM_EPS)
    S = torch.einsum('thd,vhd->tv', t, v) / H
    rows = torch.arange(S.shape[0], device=DEV)
    above = S > S[rows, gt.long()][:, None]
    above[rows, gt.long()] = False
    return above.sum(1).to(torch.int32)


@pytest.mark.parametrize('c', RANK_CASES, ids=[c.name for c in RANK_CASES])
def test_fused_prepare_vs_rank_prepare_and_float64(c):
    from laff_amd import ops
    Nt, Nv, L, H, d = 3001, 1103, 3, c.H, c.d
    g = torch.Generator(device=DEV).manual_seed(77 * H + d)
    z = torch.randn(Nv, 32, generator=g, device=DEV)
    gt = (torch.arange(Nt, device=DEV) * 31 % Nv).to(torch.int32)
    w, b, gw = _attention_params(g, H, d, False)
    flags = ops.attention_flags(True, False)
    assert ops.fused_prepare_eligible(Nt, Nv, H, d, c.prec)

    def latent(n, lat):
        x = lat @ torch.randn(32, H * d, generator=g, device=DEV) + 2.0 * torch.randn(n, H * d, generator=g, device=DEV)
        return (x, False, None, None), R.dense_plane(x, H, d)
    vp = [latent(Nv, z) for _ in range(L)]
    tp = [latent(Nt, z[gt.long()]) for _ in range(L - 1)]
    if c.text == 'G':
        csr, wt, bias, (crow, idx, val) = _gather(g, Nt, H, d, d)
        tp = [((None, False, None, None, 'tanh', (csr, wt, bias)), R.gather_plane(crow, idx, val, wt, H, d, bias, act='tanh'))] + tp
    else:
        tp = [latent(Nt, z[gt.long()])] + tp
    fp = ops.FusedPrepare(Nt, Nv, gt, heads=H)
    fp.count.fill_(7)
    fp.pairs[:4] = 9
    for t in (fp.s_gt64, fp.band_t, fp.band_v):
        t.fill_(float('nan'))
    Ev_out, Et_out = _nan((Nv, H, d)), _nan((Nt, H, d))
    pv = torch.full((Nv * H * d * 2,), 0xff, dtype=torch.uint8, device=DEV)
    pt = torch.full((Nt * H * d * 2,), 0xff, dtype=torch.uint8, device=DEV)
    Ev, V = ops.fuse([p for p, _ in vp], H, d, w, b, gw, flags, packed_precision=c.prec, rank_side=fp.video, out=Ev_out, packed_out=pv)
    Et, T = ops.fuse([p for p, _ in tp], H, d, w, b, gw, flags, packed_precision=c.prec, rank_side=fp.text, out=Et_out, packed_out=pt)
    err = 0.0
    for E, P, X in ((Ev, V, [r for _, r in vp]), (Et, T, [r for _, r in tp])):
        ref, _ = R.attention(torch.stack(X, 1), w, b, gw, with_ave=True)
        err = max(err, _check_E(E, ref, False))
        assert _packed_bits_equal(E, P, c.prec)
    st = fp.state()
    ref = ops.rank_prepare(Et, Ev, T, V, gt)
    assert torch.equal(st.s_gt64, ref.s_gt64), 's_gt64 differs from laff_rank_prepare'
    assert int(st.count.abs().sum()) == 0 and st.pairs[:4].tolist() == [0, 0, 0, 0]
    nb = ((Nv + 3) & ~3) + (Nv + 63) // 64
    for a, r in ((st.band_t[:Nt], ref.band_t[:Nt]), (st.band_v[:Nv], ref.band_v[:Nv]), (st.band_v[(Nv + 3) & ~3:nb], ref.band_v[(Nv + 3) & ~3:nb])):
        assert bool(torch.isfinite(a).all())
        assert float(((a - r).abs() / r).max()) < 1e-5 and bool((a >= r * (1 - 1e-6)).all()), 'band differs from laff_rank_prepare'
    S = ops.sim_gemm_banded(st, True)
    ops.rank_resolve(st, S)
    assert not st.listed_pairs()[1]
    want = _count_f64(Et, Ev, gt)
    assert int(want.max()) > 0
    print('%s: %s  max|E - f64| %.3e' % (c.name, c.kernel, err))
    assert torch.equal(st.count, want), 'counts after resolve != float64 counts'
    assert err <= TOL_UNIT


@pytest.mark.parametrize('c', FRAME_CASES, ids=[c.name for c in FRAME_CASES])
def test_frame_fuse_vs_float64(c):
    from laff_amd import ops
    from oracle import laff_oracle as O
    B, Fmax, d = 37, c.Fmax, c.d
    g = torch.Generator(device=DEV).manual_seed(31 * Fmax + d)
    with_ave, mul = O.FRAME_ATTENTION_FLAGS[c.attention]
    lens = torch.tensor(_frame_lengths(c, B), dtype=torch.int32, device=DEV)
    big = c.name.endswith('_big')
    # frames past a video's length hold garbage: the kernel must never fold them in (the reference pads with zeros)
    frames = [torch.randn(B, Fmax, d, generator=g, device=DEV) for _ in range(c.count)]
    params = []
    for _ in range(c.count):
        w = torch.randn(d, generator=g, device=DEV) / d ** 0.5 * (4.0 if big else 1.0)
        b = torch.randn(1, generator=g, device=DEV) * 0.3 + (100.0 if big else 0.0)
        params.append((w, b, torch.rand(1, generator=g, device=DEV)))
    mask = None
    if c.mode == 'mask':
        wide = torch.zeros((B, Fmax + 5), device=DEV)
        wide[:, :Fmax] = (torch.arange(Fmax, device=DEV)[None, :] < lens[:, None]).float()
        mask = wide[:, :Fmax]
    flags = ops.attention_flags(with_ave, mul)
    outs = [_nan((B, d)) for _ in range(c.count)]
    if c.count == 1 and c.mode != 'mask':
        got = [ops.frame_fuse(frames[0], lens if c.mode == 'lens' else None, *params[0], flags, out=outs[0])]
    else:
        got = ops.frame_fuse_grouped(frames, lens if c.mode == 'lens' else None, params, flags, mask=mask, out=outs)
    err = 0.0
    for V, fr, (w, b, gw), o in zip(got, frames, params, outs):
        assert V is o and bool(torch.isfinite(V).all()), 'an element the kernel did not write'
        ref = R.frame_attention(fr, w, b, gw, with_ave, mul, lens=lens if c.mode != 'full' else None)
        err = max(err, float((V.double() - ref).abs().max()))
    print('%s: frame_fuse_kernel<%d>  max|V - f64| %.3e' % (c.name, c.nch, err))
    assert err <= TOL_FRAMES
