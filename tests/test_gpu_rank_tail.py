"""The exact-rank tail (pack -> rank_prepare -> banded GEMM -> rank_resolve -> metrics) through every form the host path offers, at sizes
that sit off every alignment its buffers encode: 70 texts x 45 videos (no multiple of 4 or 64; 16 * 70 >= 45, so the fused prepare is
eligible), d = 8, one and two heads, and a gt_col handed in 4 bytes off 16-byte alignment."""
import functools

import numpy as np
import pytest
import torch

from oracle import laff_oracle as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NT, NV, D = 70, 45, 8
CASES = [(H, prec) for H in (1, 2) for prec in ('fp16', 'fp16x3')]


@functools.lru_cache(maxsize=None)
def _problem(H):
    """Unit-norm fp32 embeddings, ground truth, and the ranks / metrics of their float64 scores (numpy).  No two float64 scores of a
    row tie, so the ranks do not depend on how a sum is ordered."""
    g = np.random.default_rng(4500 + H)
    t = g.normal(0, 1, (NT, H, D)).astype(np.float32)
    v = g.normal(0, 1, (NV, H, D)).astype(np.float32)
    t /= np.linalg.norm(t, axis=2, keepdims=True)
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    gt = g.integers(0, NV, NT).astype(np.int32)
    S64 = O.txt2vis_matrix_f64(t, v)
    assert np.diff(np.sort(S64, axis=1), axis=1).min() > 1e-9
    ranks = O.count_ranks(S64, gt)
    assert len(set(ranks.tolist())) > 8
    r = ranks.astype(np.float64)
    metrics = (100.0 * np.mean(r <= 1), 100.0 * np.mean(r <= 5), 100.0 * np.mean(r <= 10), np.floor(np.median(r)), r.mean(),
               (1.0 / r).mean(), (1.0 / r).mean())
    return t, v, gt, ranks, metrics


def _device(H, prec):
    """(Et, Ev, T, V, gt) on the device; gt is a view that starts 4 bytes past a 16-byte boundary."""
    from laff_amd import ops
    t, v, gt, _, _ = _problem(H)
    Et, Ev = torch.as_tensor(t, device=DEV), torch.as_tensor(v, device=DEV)
    holder = torch.zeros(NT + 1, dtype=torch.int32, device=DEV)
    gtd = holder[1:]
    gtd.copy_(torch.as_tensor(gt))
    assert gtd.data_ptr() % 16 == 4 and gtd.is_contiguous()
    return Et, Ev, ops.pack_rows(Et, False, 1e-13, prec), ops.pack_rows(Ev, False, 1e-13, prec), gtd


def _same_prepared(a_sgt, a_bt, a_bv, b):
    blocks = slice((NV + 3) & ~3, ((NV + 3) & ~3) + (NV + 63) // 64)
    assert torch.equal(a_sgt, b.s_gt64) and a_sgt.shape == (NT,)
    assert torch.equal(a_bt[:NT], b.band_t[:NT])
    assert torch.equal(a_bv[:NV], b.band_v[:NV]) and torch.equal(a_bv[blocks], b.band_v[blocks])


@pytest.mark.parametrize('H,prec', CASES)
def test_the_prepare_forms_agree_bit_for_bit(H, prec):
    """s_gt64, band_t and band_v (its columns and its 64-column block maxima) of rank_prepare on given operands, of rank_prepare_text +
    rank_band_video and -- fp16 -- of rank_prepare producing the operands itself, which are the bytes pack_rows(E, normalize=False)
    writes."""
    from laff_amd import ops
    Et, Ev, T, V, gt = _device(H, prec)
    ref = ops.rank_prepare(Et, Ev, T, V, gt)
    assert ref.gt_col.data_ptr() % 16 == 0 and torch.equal(ref.gt_col, gt) and ref.pair_cap == ops.default_pair_cap(NT)
    assert int(ref.count.abs().sum()) == 0 and ref.pairs[:2].tolist() == [0, 0]
    s_gt64, band_t = ops.rank_prepare_text(Et, Ev, T, gt)
    _same_prepared(s_gt64, band_t, ops.rank_band_video(Ev, V), ref)
    if prec == 'fp16':
        st = ops.rank_prepare(Et, Ev, None, None, gt, emit_precision=prec)
        _same_prepared(st.s_gt64, st.band_t, st.band_v, ref)
        nb = NT * H * D * 2, NV * H * D * 2
        assert torch.equal(st.T.buf[:nb[0]], T.buf[:nb[0]]) and torch.equal(st.V.buf[:nb[1]], V.buf[:nb[1]])
        assert int(st.count.abs().sum()) == 0 and st.pairs[:2].tolist() == [0, 0]


@pytest.mark.parametrize('H,prec', CASES)
def test_exact_ranks_are_the_float64_ranks(H, prec):
    from laff_amd import ops
    Et, Ev, T, V, gt = _device(H, prec)
    S, count, st = ops.exact_ranks(Et, Ev, T, V, gt)
    assert not st.overflowed()
    assert np.array_equal(count.cpu().numpy() + 1, _problem(H)[3])
    assert tuple(S.shape) == (NT, NV) and torch.equal(ops.gather_gt(S, gt), st.s_gt64.float())


def _four_ways(H, prec):
    """The seven metrics by resolve + rank_metrics, resolve + rank_metrics_async, and rank_resolve_metrics synchronous and pinned --
    each fused form on a state of its own -- with the ranks every form leaves."""
    from laff_amd import ops
    Et, Ev, T, V, gt = _device(H, prec)

    def counted():
        st = ops.rank_prepare(Et, Ev, T, V, gt)
        return st, ops.sim_gemm_banded(st)

    st, S = counted()
    assert ops.rank_resolve(st, S) is st.count
    ranks = [torch.empty_like(st.count) for _ in range(4)]
    pinned = [torch.full((8,), -1.0, dtype=torch.float64).pin_memory() for _ in range(2)]
    out = [ops.rank_metrics(st.count, base=1, ranks_out=ranks[0])]
    ops.rank_metrics_async(st.count, pinned[0], base=1, ranks_out=ranks[1])
    st3, S3 = counted()
    m3 = ops.rank_resolve_metrics(st3, S3, ranks_out=ranks[2])
    st4, S4 = counted()
    assert ops.rank_resolve_metrics(st4, S4, pinned[1], ranks_out=ranks[3]) is None
    torch.cuda.synchronize()
    assert pinned[0][7].item() == 0.0 and pinned[1][7].item() == 0.0
    assert torch.equal(S3, S) and torch.equal(S4, S)
    out += [tuple(pinned[0][:7].tolist()), m3, tuple(pinned[1][:7].tolist())]
    return out, [r.cpu().numpy() for r in ranks]


@pytest.mark.parametrize('H,prec', CASES)
def test_the_metrics_forms_agree(H, prec):
    """Twice over fresh state: the asynchronous forms take a new metrics slot at every call."""
    _, _, _, want_ranks, want = _problem(H)
    first, ranks = _four_ways(H, prec)
    for m, r in zip(first, ranks):
        np.testing.assert_allclose(m, want, rtol=1e-13, atol=0)
        np.testing.assert_allclose(m, first[0], rtol=1e-13, atol=0)
        assert np.array_equal(r, want_ranks)
    second, ranks = _four_ways(H, prec)
    assert second == first and all(np.array_equal(r, want_ranks) for r in ranks)
