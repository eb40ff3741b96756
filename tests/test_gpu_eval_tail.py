"""The plain evaluation tail -- the kernels that rank whatever score matrix they are handed (laff_gather_gt / laff_rank_count,
laff_v2t_count, laff_topk_rows and its host-side block merge) and the host code on top of them (predictor.v2t_metrics,
retrieval_metrics, topk_lists, txt2video_write_to_file) -- against tests/eval_ref.py on matrices full of exact ties, which is what
the 'hist' measure produces.

Every comparison is exact: counts, indices and values with array_equal, the seven metrics to rtol 1e-13 (float64 means of the same
integers, the bound tests/test_gpu_rank_tail.py holds ops.rank_metrics to).  The cases and what they contain (ties with the ground
truth, sibling and stranger ties, ties across the K-th place and across column blocks) are asserted in tests/test_eval_ref_host.py,
which runs without a GPU on the same bytes.

NaN scores are out of scope: where the reference's sort puts a NaN is an accident of numpy's sort, not a contract."""
import functools

import numpy as np
import pytest
import torch

import eval_ref as R
from oracle import laff_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def pitched(a, pitch, first=0, fill=np.inf):
    """`a` as a row view of a (rows, pitch) buffer that starts at column `first`; everything around it holds `fill`"""
    buf = torch.full((a.shape[0], pitch), fill, dtype=torch.float32, device=DEV)
    view = buf[:, first:first + a.shape[1]]
    view.copy_(torch.as_tensor(a))
    assert view.stride() == (pitch, 1) and view.data_ptr() == buf.data_ptr() + 4 * first
    return view


# ------------------------------------------------------------------------------------------------ gather_gt + rank_count
_t2v_case = functools.lru_cache(maxsize=None)(R.t2v_case)


@functools.lru_cache(maxsize=None)
def _t2v_want(Nv, kind):
    S, gt = _t2v_case(Nv, kind)
    low = R.lowered(R.gathered(S, gt))
    return R.gathered(S, gt), R.t2v_counts(S, gt), low, R.t2v_counts(S, gt, 0, low)


def _layouts(S):
    """The four layouts rank_count_kernel tells apart (float4 loads need lds % 4 == 0 and a 16-byte aligned base), padding = +inf:
    read one column too far and the count is wrong."""
    Nv = S.shape[1]
    up4 = (Nv + 3) & ~3
    out = {'contiguous': dev(S), 'pitch%4==0': pitched(S, up4 + 4), 'odd pitch': pitched(S, (Nv | 1) + 2),
           'base+4': pitched(S, up4 + 4, first=1)}
    c, p, o, b = out.values()
    assert c.is_contiguous() and c.data_ptr() % 16 == 0
    assert p.data_ptr() % 16 == 0 and p.stride(0) % 4 == 0 and p.stride(0) > Nv
    assert o.data_ptr() % 16 == 0 and o.stride(0) % 2 == 1 and o.stride(0) > Nv
    assert b.data_ptr() % 16 == 4 and b.stride(0) % 4 == 0 and b.stride(0) > Nv
    return out


@pytest.mark.parametrize('kind', R.T2V_KINDS, ids=lambda k: 'levels%s' % k if isinstance(k, int) else k)
@pytest.mark.parametrize('Nv', R.T2V_NV)
def test_rank_count_every_layout_equals_the_reference(Nv, kind):
    from laff_amd import ops
    S, gt = _t2v_case(Nv, kind)
    want_sgt, want, low, want_low = _t2v_want(Nv, kind)
    gtd, lowd = dev(gt), dev(low)
    for name, Sd in _layouts(S).items():
        s_gt = ops.gather_gt(Sd, gtd)
        count = ops.rank_count(Sd, gtd, s_gt)
        assert count.dtype == torch.int32
        # bytes, so that -0.0 gathered as +0.0 would show
        assert s_gt.cpu().numpy().tobytes() == want_sgt.tobytes(), name
        assert np.array_equal(count.cpu().numpy(), want), name
        # a threshold below the ground truth's own entry: that entry is above it and must still be left out
        assert np.array_equal(ops.rank_count(Sd, gtd, lowd).cpu().numpy(), want_low), name
    if kind == 1:
        assert int(count.abs().sum()) == 0                        # one score level: everything ties, every rank is 1


@pytest.mark.parametrize('kind', [3, 'special'])
@pytest.mark.parametrize('layout', ['contiguous', 'pitch%4==0'])
def test_rank_count_column_shards_accumulate_to_the_global_count(layout, kind):
    """Three column shards (130, 3 and 126 columns) as views into the matrix: s_gt is the maximum of the shards' gathers (-inf
    where the ground truth lives elsewhere), and the counts accumulated through count= are the global ones -- on zeros and on a
    count that already holds something."""
    from laff_amd import ops
    S, gt = _t2v_case(259, kind)
    want_sgt, want = _t2v_want(259, kind)[:2]
    Sd = _layouts(S)[layout]
    gtd = dev(gt)
    b = R.SHARD_BOUNDS
    parts = [(a, Sd[:, a:z]) for a, z in zip(b[:-1], b[1:])]
    assert min(p.shape[1] for _, p in parts) < 4
    gathers = torch.stack([ops.gather_gt(p, gtd, col0=a) for a, p in parts])
    for (a, p), got in zip(parts, gathers):
        assert got.cpu().numpy().tobytes() == R.gathered(S[:, a:a + p.shape[1]], gt, a).tobytes()
    s_gt = gathers.max(dim=0).values
    assert s_gt.cpu().numpy().tobytes() == want_sgt.tobytes()
    prefill = (np.arange(R.T2V_NT, dtype=np.int32) * 3 + 7)
    for start in (np.zeros(R.T2V_NT, dtype=np.int32), prefill):
        total, want_total = dev(start), start + want
        for a, p in parts:
            alone = ops.rank_count(p, gtd, s_gt, col0=a)
            assert np.array_equal(alone.cpu().numpy(), R.t2v_counts(S[:, a:a + p.shape[1]], gt, a, want_sgt))
            assert ops.rank_count(p, gtd, s_gt, col0=a, count=total) is total
        assert np.array_equal(total.cpu().numpy(), want_total)


# ------------------------------------------------------------------------------------------------ v2t_count
_v2t_case = functools.lru_cache(maxsize=None)(R.v2t_case)
_v2t_want = functools.lru_cache(maxsize=None)(lambda i: R.v2t_counts(*_v2t_case(i)))
V2T_IDS = ['max%d-nv%d-%s' % (max(m), nv, 'distinct' if lv is None else 'levels%d' % lv) for m, nv, lv in R.V2T_CASES]
V2T_FULL = [i for i, (m, _, _) in enumerate(R.V2T_CASES) if len(m) == 1]          # every video has a caption


def _grouping(owner, Nv):
    """(grp_off, grp_idx, max_group) as predictor.v2t_positions builds them"""
    order = np.argsort(owner, kind='stable').astype(np.int32)
    sizes = np.bincount(owner, minlength=Nv)
    off = np.zeros(Nv + 1, dtype=np.int32)
    np.cumsum(sizes, out=off[1:])
    return dev(off), dev(order), int(sizes.max())


@pytest.mark.parametrize('i', range(len(R.V2T_CASES)), ids=V2T_IDS)
def test_v2t_count_equals_the_reference_element_by_element(i):
    from laff_amd import ops
    S, owner = _v2t_case(i)
    Nt, Nv = S.shape
    off, order, biggest = _grouping(owner, Nv)
    assert biggest == max(R.V2T_CASES[i][0])
    for Sd in (dev(S), pitched(S, Nv + 5)):
        count = ops.v2t_count(Sd, off, order, biggest)
        assert count.dtype == torch.int32 and count.shape == (Nt,)
        assert np.array_equal(count.cpu().numpy(), _v2t_want(i))


@pytest.mark.parametrize('i', V2T_FULL, ids=[V2T_IDS[i] for i in V2T_FULL])
def test_metrics_on_tied_scores_equal_the_reference(i):
    from laff_amd import predictor as P
    S, owner = _v2t_case(i)
    Nv = S.shape[1]
    txt_ids, vis_ids = R.ids_of(owner, Nv)
    want_t2v, want_v2t = O.predictor_metrics(S, txt_ids, vis_ids)
    assert R.v2t_metrics(S, owner) == want_v2t
    for Sd in (dev(S), pitched(S, Nv + 5)):
        np.testing.assert_allclose(P.v2t_metrics(Sd, owner), want_v2t, rtol=1e-13, atol=0)
        t2v, v2t = P.retrieval_metrics(Sd, txt_ids, vis_ids)
        np.testing.assert_allclose(t2v, want_t2v, rtol=1e-13, atol=0)
        np.testing.assert_allclose(v2t, want_v2t, rtol=1e-13, atol=0)


def test_metrics_refuse_a_video_without_captions():
    from laff_amd import predictor as P
    i = [len(m) > 1 for m, _, _ in R.V2T_CASES].index(True)
    S, owner = _v2t_case(i)
    assert np.bincount(owner, minlength=S.shape[1]).min() == 0
    with pytest.raises(IndexError):
        P.v2t_metrics(dev(S), owner)
    with pytest.raises(IndexError):
        R.v2t_metrics(S, owner)


# ------------------------------------------------------------------------------------------------ topk_rows
def _same_lists(got, S, K):
    idx, val = got
    want_idx, want_val = R.topk(S, K)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and tuple(idx.shape) == tuple(val.shape) == want_idx.shape
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert val.cpu().numpy().tobytes() == want_val.tobytes()          # bytes: the scores are the matrix's own entries, -0.0 included


@pytest.mark.parametrize('K', R.TOPK_K)
def test_topk_at_the_template_boundaries(K):
    """K on both sides of every KP switch (64 / 512 / 2048 / 4096 / 8192) at Nv = K (everything is selected), Nv = K + 1 (one column
    is left out) and a wide row whose K-th place lies inside a long run of equal values; each with an all-equal, an ascending and a
    descending row or their wide counterparts."""
    from laff_amd import ops
    cap = ops.topk_max_columns(K)
    for Nv, wide in zip(R.topk_sizes(K, cap), (False, False, True)):
        assert K <= Nv <= cap                                     # one kernel call: the merge has tests of its own below
        S = R.topk_case(K, Nv, wide)
        _same_lists(ops.topk_rows(dev(S), K), S, K)


def test_topk_never_selects_the_padding_of_a_pitched_matrix():
    from laff_amd import ops
    S = R.topk_case(65, 1000, False)
    _same_lists(ops.topk_rows(pitched(S, 1024), 65), S, 65)
    _same_lists(ops.topk_rows(pitched(S, 1027, first=3), 1000), S, 1000)


def test_topk_of_infinities_and_signed_zeros(tmp_path):
    """-0.0 and +0.0 are one score (ties by index) and come back with the sign they have in the matrix: the result files print them;
    +-inf sort as numbers.  Single call, column blocks, and the `[0:-1]` list of the writer."""
    from laff_amd import ops, predictor as P
    g = np.random.default_rng(9600)
    S = R.special(g, 4, 300)
    assert np.signbit(S[S == 0]).any() and not np.signbit(S[S == 0]).all() and np.isinf(S).any()
    for K in (1, 150, 299, 300):
        _same_lists(ops.topk_rows(dev(S), K), S, K)
    W = R.special(g, 2, 40000)
    assert W.shape[1] > ops.topk_max_columns(2049)
    _same_lists(ops.topk_rows(dev(W), 2049), W, 2049)
    vis_ids = ['video%d' % v for v in range(300)]
    txt_ids, f = ['video%d#0' % t for t in range(4)], str(tmp_path / 'id.sent.score.txt')
    idx, val = P.txt2video_write_to_file(f, dev(S), vis_ids, txt_ids)
    want_idx, want_val = R.topk(S, 299)
    assert np.array_equal(idx, want_idx) and val.tobytes() == want_val.tobytes()
    lines = R.writer_lines(S, vis_ids, txt_ids, 299)
    assert all(' -0.0' in ln and ' 0.0' in ln and ' inf' in ln and ' -inf' in ln for ln in lines)
    assert open(f).read().split('\n') == lines + ['']


def _merge_precondition():
    from laff_amd import ops
    Nt, Nv, K = R.MERGE_SHAPE
    cap = ops.topk_max_columns(K)
    candidates = sum(min(K, min(Nv, c0 + cap) - c0) for c0 in range(0, Nv, cap))
    # more candidates than one call takes: _topk_blocks has to merge groups of block lists first.  (A larger LDS budget would turn
    # this into a one-level case: then the shape has to grow with it.)
    assert Nv > cap and candidates > cap, (cap, candidates)
    return cap


def test_topk_group_merge_with_ties_planted_across_blocks():
    from laff_amd import ops
    cap = _merge_precondition()
    S = R.merge_case_planted(cap)
    _same_lists(ops.topk_rows(dev(S), R.MERGE_SHAPE[2]), S, R.MERGE_SHAPE[2])


def test_topk_group_merge_on_three_score_levels():
    """3-level scores: every block hands on K candidates of one value, and the winners are the K largest indices of that value over
    all blocks.  Contiguous, and as a pitched view with +inf behind every row."""
    from laff_amd import ops
    _merge_precondition()
    Nt, Nv, K = R.MERGE_SHAPE
    S = R.merge_case_quantised()
    _same_lists(ops.topk_rows(dev(S), K), S, K)
    _same_lists(ops.topk_rows(pitched(S, Nv + 24), K), S, K)


# ------------------------------------------------------------------------------------------------ the result lists
@pytest.mark.parametrize('threshold,K', [(2000, 36), (20, 20), (37, 37)])
def test_result_lists_and_files_on_tied_scores(threshold, K, tmp_path):
    """Nv < Threshold keeps all but the last (the reference's `[0:-1]`), Nv >= Threshold the best Threshold."""
    from laff_amd import predictor as P
    S, vis_ids, txt_ids = R.writer_case()
    want_idx, want_val = R.topk(S, K)
    idx, val = P.topk_lists(dev(S), vis_ids, threshold)
    assert np.array_equal(idx, want_idx) and np.array_equal(val, want_val)
    f = str(tmp_path / 'id.sent.score.txt')
    idx, val = P.txt2video_write_to_file(f, dev(S), vis_ids, txt_ids, Threshold=threshold)
    assert np.array_equal(idx, want_idx) and np.array_equal(val, want_val)
    assert open(f).read().split('\n') == R.writer_lines(S, vis_ids, txt_ids, K) + ['']


# ------------------------------------------------------------------------------------------------ the motivating case
def test_hist_scores_ranked_end_to_end():
    """ops.sim_hist on small integer counts gives a matrix that ties all over; every kernel of the tail on that very matrix equals
    the reference run on its copy on the host."""
    from laff_amd import ops, predictor as P
    T, V, gt = R.hist_case()
    Nt, Nv, _ = R.HIST_SHAPE
    Sd = ops.sim_hist(dev(T), dev(V), eps=1e-8)
    S = Sd.cpu().numpy()
    assert S.shape == (Nt, Nv) and R.rows_tied_with_gt(S, gt) >= 0.25
    assert np.mean([len(np.unique(S[:, v])) < Nt for v in range(Nv)]) == 1.0
    gtd = dev(gt)
    assert np.array_equal(ops.rank_count(Sd, gtd, ops.gather_gt(Sd, gtd)).cpu().numpy(), R.t2v_counts(S, gt))
    off, order, biggest = _grouping(gt, Nv)
    assert np.array_equal(ops.v2t_count(Sd, off, order, biggest).cpu().numpy(), R.v2t_counts(S, gt))
    for K in (10, Nv - 1, Nv):
        _same_lists(ops.topk_rows(Sd, K), S, K)
    txt_ids, vis_ids = R.ids_of(gt, Nv)
    want = O.predictor_metrics(S, txt_ids, vis_ids)
    for got, w in zip(P.retrieval_metrics(Sd, txt_ids, vis_ids), want):
        np.testing.assert_allclose(got, w, rtol=1e-13, atol=0)
