"""Every kernel behind laff_sim_gemm / laff_sim_gemm_banded, element by element against float64.

launch_gemm_nt (laff_amd/csrc/gemm_nt.hip) picks one of seven routes from the shape, the K bytes, the precision and the LAFF_STRIP mode;
laff_sim_gemm_route names the pick without launching, so every case below first proves which kernel it is about to check.  Per case:
  1. the scores against float64 sums of exactly the products the kernel forms on its packed operands (hi*hi + hi*lo + lo*hi for the
     split formats), times the scale: the only error left is fp32 accumulation of exact products;
  2. the scores against the float64 cosine of the fp32 embeddings, within the precision's contract (PREC_TOL of test_gpu_kernels.py);
  3. the approximate fused count (row_dot_gt + gt_col / s_gt): S[t, gt] == s_gt[t] bit for bit, the count recounted from that S, the
     count-only launch;
  4. the banded count (rank_prepare -> sim_gemm_banded -> rank_resolve): the scores bit-identical to the scores-only launch away from the
     ground truth, the pre-resolve counts bracketing the float64 counts, the re-scored entries, the final counts equal to float64's.
Every score buffer is NaN, padding included, before each launch: a tile the kernel skipped cannot pass on what a previous launch left."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import laff_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'

PREC_TOL = {'fp32': 2e-6, 'fp16x3': 2e-6, 'bf16x3': 5e-6, 'fp16': 1e-4, 'bf16': 2e-3}     # test_gpu_kernels.py
# against the operand-exact float64 reference the only error is fp32 accumulation of exact products.  The 16-bit MFMAs
# (v_mfma_f32_32x32x16_*) round once per 16 products; the fp32 one (v_mfma_f32_32x32x2_f32) once per 2, so K / 2 roundings pile up:
# 1.04e-6 measured at K = 1024 (t128_fp32_ragged), where the bound of the fp32 contract applies instead.
EXACT_TOL = {'fp32': 2e-6, 'fp16x3': 1e-6, 'bf16x3': 1e-6, 'fp16': 1e-6, 'bf16': 1e-6}

Case = namedtuple('Case', 'name Nt Nv H d precision strip pitch route approx_route')


def _c(name, Nt, Nv, H, d, precision, strip, pitch, route, approx_route=None):
    return Case(name, Nt, Nv, H, d, precision, strip, pitch, route, approx_route or route)


# pitch 'pad': alloc_scores' row pitch (Nv rounded up to 32 floats), 'odd': Nv + 1 (rows off 16-byte alignment: no FULL stores).
# Tile counts in the route's own tiles (128 x 128 for the TILED128 family, 256 x 256 for TILED256 / LONGK / X3).
CASES = [
    # K bytes % 16 != 0: operands staged through registers (16-bit d = 516: 1032 bytes; fp32 d = 514: 2056 bytes)
    _c('reg_full_fp16', 1024, 512, 1, 516, 'fp16', 0, 'pad', 'TILED128_REG'),                  # 8 x 4 = 32 tiles
    _c('reg_ragged_bf16', 1025, 513, 1, 516, 'bf16', 0, 'odd', 'TILED128_REG'),                # 9 x 5 = 45
    _c('reg_nt1_bf16', 1, 777, 1, 516, 'bf16', 0, 'odd', 'TILED128_REG'),
    _c('reg_fp32', 640, 384, 1, 514, 'fp32', 0, 'pad', 'TILED128_REG'),
    # K bytes % 128 != 0: LDS-DMA with a K tail (16-bit d = 520: 1040 bytes; fp32 d = 516: 2064 bytes)
    _c('tail_full_fp16', 1024, 1024, 1, 520, 'fp16', 0, 'pad', 'TILED128_TAIL'),               # 64
    _c('tail_ragged_bf16', 1153, 1025, 1, 520, 'bf16', 0, 'odd', 'TILED128_TAIL'),             # 10 x 9 = 90
    _c('tail_nv1_fp16', 257, 1, 1, 520, 'fp16', 0, 'pad', 'TILED128_TAIL'),
    _c('tail_fp32', 700, 900, 1, 516, 'fp32', 0, 'odd', 'TILED128_TAIL'),
    _c('tail_k4128_fp16', 16384, 16384, 8, 516, 'fp16', 0, 'pad', 'TILED128_TAIL'),           # 4096 big tiles, but K = 4128
    # fast LDS-DMA, 128 x 128 tiles: fp32 at any size, 16-bit below 512 big tiles
    _c('t128_fp32_full', 8192, 4096, 1, 512, 'fp32', 0, 'pad', 'TILED128'),                    # 2048
    _c('t128_fp32_ragged', 2049, 1025, 2, 512, 'fp32', 0, 'odd', 'TILED128'),                  # 17 x 9 = 153
    _c('t128_full_fp16', 2048, 1024, 2, 512, 'fp16', 0, 'pad', 'TILED128'),                    # 128
    _c('t128_ragged_fp16', 1153, 2049, 1, 512, 'fp16', 0, 'odd', 'TILED128'),                  # 10 x 17 = 170
    _c('t128_511_fp16', 1792, 18688, 1, 512, 'fp16', 0, 'pad', 'TILED128'),                    # 7 x 73 = 511 big tiles
    _c('t128_511_bf16', 18688, 1792, 2, 512, 'bf16', 0, 'odd', 'TILED128'),
    _c('t128_nt1_bf16', 1, 4096, 1, 512, 'bf16', 0, 'pad', 'TILED128'),
    _c('t128_h8_fp16', 1000, 300, 8, 512, 'fp16', 1, 'pad', 'TILED128'),
    _c('t128_511_fp16x3', 18688, 1792, 1, 512, 'fp16x3', 0, 'pad', 'TILED128'),                # split operands below X3's threshold
    _c('t128_ragged_bf16x3', 1025, 1153, 1, 512, 'bf16x3', 0, 'odd', 'TILED128'),              # 9 x 10 = 90
    # 256 x 256 tiles, 8 waves: 16-bit, >= 512 big tiles
    _c('t256_512_fp16', 8192, 4096, 1, 512, 'fp16', 0, 'pad', 'TILED256'),                     # 32 x 16 = 512
    _c('t256_ragged_bf16', 8193, 4097, 2, 512, 'bf16', 0, 'odd', 'TILED256'),                  # 33 x 17 = 561
    _c('t256_full_bf16', 4096, 8192, 4, 512, 'bf16', 0, 'pad', 'TILED256'),                    # 512, K = 2048
    _c('t256_h4_fp16', 8704, 8448, 4, 512, 'fp16', 0, 'odd', 'TILED256'),                      # 34 x 33 = 1122
    _c('t256_4095_bf16', 16128, 16640, 8, 512, 'bf16', 0, 'pad', 'TILED256'),                  # 63 x 65 = 4095, K = 4096
    _c('t256_k4032_fp16', 16384, 16384, 8, 504, 'fp16', 0, 'pad', 'TILED256'),                 # 4096, K bytes 8064
    # 256 x 256 tiles, 4 waves: one plane, >= 4096 big tiles, K bytes >= 8192 (C5's route)
    _c('longk_4096_bf16', 16384, 16384, 8, 512, 'bf16', 0, 'pad', 'TILED256_LONGK'),          # 64 x 64 = 4096, K bytes 8192
    _c('longk_ragged_fp16', 16641, 16385, 8, 512, 'fp16', 0, 'odd', 'TILED256_LONGK'),        # 66 x 65 = 4290
    # the hi/lo split tile: >= 512 big tiles (predict()'s default precision)
    _c('x3_512_fp16x3', 8192, 4096, 1, 512, 'fp16x3', 0, 'pad', 'X3'),                         # 512
    _c('x3_ragged_bf16x3', 8193, 4097, 1, 512, 'bf16x3', 0, 'odd', 'X3'),                      # 561
    _c('x3_h2_bf16x3', 4096, 8192, 2, 512, 'bf16x3', 0, 'pad', 'X3'),                          # 512
    _c('x3_ragged_fp16x3', 10241, 4097, 2, 512, 'fp16x3', 1, 'odd', 'X3'),                     # 41 x 17 = 697
    # the K = 512 strip kernel (the approximate count is not its epilogue: that launch stays tiled)
    _c('strip_fp16', 4096, 4096, 1, 512, 'fp16', 2, 'pad', 'STRIP', 'TILED128'),
    _c('strip_ragged_bf16', 4097, 4129, 1, 512, 'bf16', 2, 'pad', 'STRIP', 'TILED128'),
    _c('strip_default_fp16', 8192, 6144, 1, 512, 'fp16', 1, 'pad', 'STRIP', 'TILED256'),
]


def test_table_covers_every_route():
    from laff_amd import ops
    assert {c.route for c in CASES} == set(ops.SIM_ROUTES)
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.fixture
def strip_mode():
    from laff_amd import ops

    def set_mode(m):
        os.environ['LAFF_STRIP'] = str(m)
        ops.reset_contexts()
    yield set_mode
    os.environ.pop('LAFF_STRIP', None)
    ops.reset_contexts()


def _inputs(Nt, Nv, H, d, seed, noise=6.0):
    """Clustered embeddings (many near ties), as test_gpu_strip.py makes them, plus an all-zero text row, an all-zero video row and an
    exact duplicate of video 0 (the ground truth of text 0: a true tie)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn(Nv, 48, generator=g, device=DEV)
    P = torch.randn(48, H * d, generator=g, device=DEV)
    gt = (torch.arange(Nt, device=DEV) * 7919 % Nv).to(torch.int32)
    Ev = (z @ P + noise * torch.randn(Nv, H * d, generator=g, device=DEV)).reshape(Nv, H, d).contiguous()
    Et = (z[gt.long()] @ P + noise * torch.randn(Nt, H * d, generator=g, device=DEV)).reshape(Nt, H, d).contiguous()
    if Nt >= 2:
        Et[-1] = 0
    if Nv >= 3:
        Ev[-1] = 0
        Ev[-2] = Ev[0]
    return Et, Ev, gt


def _nan_scores(Nt, Nv, pitch):
    return torch.full((Nt, pitch), float('nan'), device=DEV)[:, :Nv]


def _padding_untouched(S):
    base = S.as_strided((S.shape[0], S.stride(0)), (S.stride(0), 1))
    return bool(base[:, S.shape[1]:].isnan().all())


def _decode(P):
    """The packed operand as float64 (N, K) planes: [x] for one-plane formats, [hi, lo] for the split formats."""
    N, K = P.N, P.K
    if P.precision == 'fp32':
        return [P.buf.view(torch.float32)[:N * K].view(N, K).double()]
    dt = torch.float16 if P.precision.startswith('fp16') else torch.bfloat16
    x = P.buf.view(dt)
    if P.precision.endswith('x3'):
        return [x[:N * K].view(N, K).double(), x[N * K:2 * N * K].view(N, K).double()]
    return [x[:N * K].view(N, K).double()]


def _exact_operands(T, V):
    """Row and column factors whose float64 product is the sum of exactly the products the kernel forms: hi*hi + hi*lo + lo*hi."""
    t, v = _decode(T), _decode(V)
    if len(t) == 1:
        return t[0], v[0]
    return torch.cat([t[0], t[0], t[1]], 1), torch.cat([v[0], v[1], v[0]], 1)


def cosine_f64(E):
    """(N, H, d) fp32 -> (N, H * d) float64, every head normalised as loss.l2norm does (eps 1e-13, + 1e-14)."""
    e = E.double()
    e = e / (e.pow(2).sum(2, keepdim=True).sqrt() + (1e-13 + 1e-14))
    return e.reshape(E.shape[0], -1)


def _ulp32(x):
    a = x.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float('inf'))) - a).double()


def _route(ops, c, K, lds=None, count=None):
    return ops.sim_gemm_route(c.Nt, c.Nv, K, c.precision, lds=lds, count=count)


def test_fp64_helper_matches_the_oracle():
    """cosine_f64 (the contract reference below) is oracle.laff_oracle.txt2vis_matrix_f64, zero rows included."""
    Et, Ev, _ = _inputs(37, 29, 2, 64, 5)
    want = O.txt2vis_matrix_f64(Et.cpu().numpy(), Ev.cpu().numpy())
    got = (cosine_f64(Et) @ cosine_f64(Ev).T / 2).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-14
    assert np.all(got[-1] == 0) and np.all(got[:, -1] == 0)


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_sim_gemm_route_vs_float64(strip_mode, c):
    from laff_amd import ops
    strip_mode(c.strip)
    Nt, Nv, H, d = c.Nt, c.Nv, c.H, c.d
    K = H * d
    pitch = Nv + 1 if c.pitch == 'odd' else (Nv + 31) & ~31
    assert _route(ops, c, K, lds=pitch) == c.route
    Et, Ev, gt = _inputs(Nt, Nv, H, d, Nt * 7 + Nv + K)
    T, V = ops.pack_rows(Et, True, 1e-13, c.precision), ops.pack_rows(Ev, True, 1e-13, c.precision)
    scale = 1.0 / (H * T.prescale * V.prescale)
    S = _nan_scores(Nt, Nv, pitch)
    ops.sim_gemm(T, V, H, out=S)

    approx = c.precision != 'fp32'              # row_dot_gt: 16-bit operands
    if approx:
        assert _route(ops, c, K, lds=pitch, count='approx') == c.approx_route
        assert _route(ops, c, K, count='approx') == c.approx_route
        cnt = torch.full((Nt,), -5, device=DEV, dtype=torch.int32)
        s_gt = ops.row_dot_gt(T, V, gt, heads=H, zero_count=cnt)
        Sa = _nan_scores(Nt, Nv, pitch)
        ops.sim_gemm(T, V, H, out=Sa, gt_col=gt, s_gt=s_gt, count=cnt)
        cnt_only = torch.full((Nt,), -5, device=DEV, dtype=torch.int32)
        ops.row_dot_gt(T, V, gt, heads=H, zero_count=cnt_only)
        ops.sim_gemm(T, V, H, want_scores=False, gt_col=gt, s_gt=s_gt, count=cnt_only)
        assert torch.equal(cnt_only, cnt)
        assert _padding_untouched(Sa)

    banded = d % 4 == 0                         # laff_rank_prepare: d % 4 == 0
    if banded:
        assert _route(ops, c, K, lds=pitch, count='banded') == c.route
        assert _route(ops, c, K, count='banded') == c.route
        st = ops.rank_prepare(Et, Ev, T, V, gt)
        Sb = _nan_scores(Nt, Nv, pitch)
        ops.sim_gemm_banded(st, True, out=Sb)
        Sb_pre, count_pre, pairs = Sb.clone(), st.count.clone(), st.pair_indices()
        assert not st.overflowed()
        ops.rank_resolve(st, Sb)
        assert _padding_untouched(Sb)
        st2 = ops.rank_prepare(Et, Ev, T, V, gt)
        ops.sim_gemm_banded(st2, want_scores=False)
        pairs2 = st2.pair_indices()
        ops.rank_resolve(st2)
        assert not st2.overflowed()
        assert torch.equal(st2.count, st.count)
        assert torch.equal(torch.unique(pairs2[:, 0] * Nv + pairs2[:, 1]), torch.unique(pairs[:, 0] * Nv + pairs[:, 1]))
        listed = torch.bincount(pairs[:, 0], minlength=Nt)
        s_gt64 = st.s_gt64
        diag = (torch.arange(Nt, device=DEV), gt.long())
        if c.route == 'STRIP':          # the strip kernel stores its own score at the ground truth; the resolve writes s_gt64 over it
            assert torch.equal(Sb_pre[diag], S[diag])
        else:
            assert torch.equal(Sb_pre[diag], s_gt64.float())
        assert torch.equal(Sb[diag], s_gt64.float())
        in_list = torch.zeros((Nt, Nv), dtype=torch.bool, device=DEV)
        in_list[pairs[:, 0], pairs[:, 1]] = True

    assert _padding_untouched(S)
    Rt, Rv = _exact_operands(T, V)
    Ct, Cv = cosine_f64(Et), cosine_f64(Ev)
    err_exact = err_contract = err_resolved = 0.0
    want_all = torch.empty((Nt,), dtype=torch.int32, device=DEV)
    for a in range(0, Nt, 4096):
        b = min(a + 4096, Nt)
        rows = torch.arange(b - a, device=DEV)
        g = gt[a:b].long()
        Sblk = S[a:b]
        assert bool(torch.isfinite(Sblk).all()), 'a score the kernel did not write'
        Sd = Sblk.double()
        err_exact = max(err_exact, float((Sd - (Rt[a:b] @ Rv.T) * scale).abs().max()))
        cos = Ct[a:b] @ Cv.T / H
        err_contract = max(err_contract, float((Sd - cos).abs().max()))
        off_gt = torch.ones((b - a, Nv), dtype=torch.bool, device=DEV)
        off_gt[rows, g] = False
        if approx:
            assert torch.equal(Sa[a:b][rows, g], s_gt[a:b]), 'S[t, gt] != s_gt[t]'
            assert torch.equal(Sa[a:b][off_gt], Sblk[off_gt]), 'the fused count changed a score'
            recount = ((Sa[a:b] > s_gt[a:b, None]) & off_gt).sum(1).to(torch.int32)
            assert torch.equal(cnt[a:b], recount), 'fused count != recount from the S it wrote'
        if banded:
            # float64 counts; a difference below 1e-12 is the duplicate video's tie (two float64 evaluations may round it apart)
            sg = cos[rows, g]
            want = ((cos > sg[:, None] + 1e-12) & off_gt).sum(1).to(torch.int32)
            want_all[a:b] = want
            assert torch.equal(Sb_pre[a:b][off_gt], Sblk[off_gt]), 'banded epilogue scores != scores-only launch'
            cp, ls = count_pre[a:b], listed[a:b].to(torch.int32)
            bad = (cp > want) | (want > cp + ls)
            assert not bool(bad.any()), 'pre-resolve count does not bracket the float64 count (%d rows)' % int(bad.sum())
            lst = in_list[a:b]
            assert torch.equal(Sb[a:b][~lst & off_gt], Sblk[~lst & off_gt]), 'the resolve changed an entry it did not list'
            if bool(lst.any()):
                x, ref = Sb[a:b][lst].double(), cos[lst]
                err_resolved = max(err_resolved, float(((x - ref).abs() / (2 * _ulp32(ref) + 1e-15)).max()))
    print('%s: route %s  max|S - exact products| %.3e  max|S - cos64| %.3e  resolved/2ulp %.3f' % (
        c.name, c.route, err_exact, err_contract, err_resolved))
    assert err_exact <= EXACT_TOL[c.precision]
    assert err_contract <= PREC_TOL[c.precision]
    if banded:
        assert err_resolved <= 1.0, 'a re-scored entry is more than 2 ulp from float64'
        assert torch.equal(st.count, want_all), 'final counts != float64 counts'


def test_approx_count_video_shard(strip_mode):
    """A video shard (col0 > 0) of the TILED256 route: texts whose ground truth lies outside the shard get s_gt = -inf and count every
    video of the shard; the others as without shards."""
    from laff_amd import ops
    strip_mode(0)
    Nt, Nv_all, v0, Nv, H, d = 8192, 6000, 1000, 4096, 1, 512
    assert ops.sim_gemm_route(Nt, Nv, H * d, 'fp16', lds=Nv, count='approx') == 'TILED256'
    Et, Ev_all, gt = _inputs(Nt, Nv_all, H, d, 17)
    Ev = Ev_all[v0:v0 + Nv].contiguous()
    T, V = ops.pack_rows(Et, True, 1e-13, 'fp16'), ops.pack_rows(Ev, True, 1e-13, 'fp16')
    S = _nan_scores(Nt, Nv, Nv)
    ops.sim_gemm(T, V, H, out=S)
    cnt = torch.full((Nt,), -5, device=DEV, dtype=torch.int32)
    s_gt = ops.row_dot_gt(T, V, gt, heads=H, col0=v0, zero_count=cnt)
    Sa = _nan_scores(Nt, Nv, Nv)
    ops.sim_gemm(T, V, H, out=Sa, gt_col=gt, s_gt=s_gt, count=cnt, col0=v0)
    local = gt.long() - v0
    inside = (local >= 0) & (local < Nv)
    assert 0 < int(inside.sum()) < Nt
    assert bool(torch.isneginf(s_gt[~inside]).all()) and bool((cnt[~inside] == Nv).all())
    r = torch.nonzero(inside).squeeze(1)
    assert torch.equal(Sa[r, local[r]], s_gt[r])
    off_gt = torch.ones((Nt, Nv), dtype=torch.bool, device=DEV)
    off_gt[r, local[r]] = False
    assert torch.equal(Sa[off_gt], S[off_gt])
    assert torch.equal(cnt, ((Sa > s_gt[:, None]) & off_gt).sum(1).to(torch.int32))
