"""tests/eval_ref.py held to the oracle (which tests/golden/eval.npz holds to the original's recorded outputs), the host arithmetic of
predictor.v2t_metrics replayed on reference counts, and the properties of the generated cases that tests/test_gpu_eval_tail.py relies
on.  CPU only."""
import numpy as np
import pytest
import torch

import eval_ref as R
from oracle import laff_oracle as O


def _problem(seed, max_videos=29, max_caps=39, levels=None, pin_max=False):
    """a random grouping (every video at least one caption; pin_max: video 0 has max_caps) and a score matrix of `levels` values, or
    tie-free"""
    g = np.random.default_rng(seed)
    Nv = int(g.integers(1, max_videos + 1))
    sizes = g.integers(1, max_caps + 1, Nv)
    if pin_max:
        sizes[0] = max_caps
    owner = R.groups(g, Nv, sizes)
    S = R.distinct(g, len(owner), Nv) if levels is None else R.quantised(g, len(owner), Nv, levels)
    return S, owner


# ------------------------------------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize('seed', range(8))
def test_reference_equals_the_oracle_without_ties(seed):
    S, owner = _problem(seed, levels=None)
    txt_ids, vis_ids = R.ids_of(owner, S.shape[1])
    assert np.array_equal(R.t2v_counts(S, owner) + 1, O.count_ranks(S, owner))
    t2v, v2t = O.predictor_metrics(S, txt_ids, vis_ids)
    assert R.t2v_metrics(S, owner) == t2v and R.v2t_metrics(S, owner) == v2t
    # video -> text counts are the places in an argsort of the column (no ties: any sort kind)
    for v in range(S.shape[1]):
        place = np.empty(S.shape[0], dtype=np.int64)
        place[np.argsort(-S[:, v])] = np.arange(S.shape[0])
        assert np.array_equal(R.v2t_counts(S, owner)[owner == v], place[owner == v])
    K = max(1, S.shape[1] // 2)
    idx, val = R.topk(S, K)
    assert np.array_equal(idx, np.argsort(S, axis=1)[:, ::-1][:, :K]) and np.array_equal(val, -np.sort(-S, axis=1)[:, :K])


@pytest.mark.parametrize('seed', range(12))
def test_reference_equals_the_oracle_with_ties(seed):
    S, owner = _problem(100 + seed, levels=1 + seed % 5)
    txt_ids, vis_ids = R.ids_of(owner, S.shape[1])
    t2v, v2t = O.predictor_metrics(S, txt_ids, vis_ids)
    assert np.array_equal(R.t2v_counts(S, owner) + 1, O.count_ranks(S, owner))
    assert R.t2v_metrics(S, owner) == t2v and R.v2t_metrics(S, owner) == v2t
    for v, pos in enumerate(R.v2t_positions(S, owner)):
        assert np.array_equal(pos, O.gt_positions(S[:, v], np.nonzero(owner == v)[0]))


def test_shard_contract_of_the_counts():
    """a column outside the shard gathers -inf; with the global s_gt the shard counts add up to the global count"""
    S, gt = R.t2v_case(259, 3)
    b = R.SHARD_BOUNDS
    parts = [(a, S[:, a:z]) for a, z in zip(b[:-1], b[1:])]
    g = np.stack([R.gathered(p, gt, a) for a, p in parts])
    assert np.array_equal(np.isfinite(g).sum(axis=0), np.ones(len(gt)))
    s_gt = g.max(axis=0)
    assert np.array_equal(s_gt, S[np.arange(len(gt)), gt])
    assert np.array_equal(sum(R.t2v_counts(p, gt, a, s_gt) for a, p in parts), R.t2v_counts(S, gt))
    assert min(z - a for a, z in zip(b[:-1], b[1:])) < 4 and b[0] == 0 and b[-1] == 259
    assert all(((gt >= a) & (gt < z)).any() for a, z in zip(b[:-1], b[1:]))      # every shard owns some ground truth


def test_empty_group_raises():
    S, owner = R.v2t_case(2)
    with pytest.raises(IndexError):
        R.v2t_metrics(S, owner)


# ------------------------------------------------------------------------------------------------ predictor's host arithmetic
def _patched_count(S, grp_off, grp_idx, max_group):
    """ops.v2t_count's contract from its own arguments, counted by the reference"""
    off, order = grp_off.numpy(), grp_idx.numpy()
    assert max_group == int(np.diff(off).max())
    owner = np.empty(len(order), dtype=np.int64)
    owner[order] = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return torch.from_numpy(R.v2t_counts(S.numpy(), owner))


@pytest.mark.parametrize('seed', range(40))
def test_predictor_v2t_metrics_on_reference_counts(seed, monkeypatch):
    """The lexsort and the bump loop for tied sibling captions: groups of up to 70 captions, 1-5 score levels."""
    from laff_amd import ops, predictor
    monkeypatch.setattr(ops, 'v2t_count', _patched_count)
    big = seed % 4 == 0
    S, owner = _problem(500 + seed, max_videos=12, max_caps=(70 if big else 39), levels=1 + seed % 5, pin_max=big)
    assert not big or np.bincount(owner).max() == 70
    got = predictor.v2t_metrics(torch.from_numpy(S), owner)
    want = R.v2t_metrics(S, owner)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got, O.predictor_metrics(S, *R.ids_of(owner, S.shape[1]))[1], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ what the GPU cases contain
@pytest.mark.parametrize('Nv', R.T2V_NV)
@pytest.mark.parametrize('kind', R.T2V_KINDS)
def test_t2v_cases_hit_every_component_and_tie_with_the_ground_truth(Nv, kind):
    S, gt = R.t2v_case(Nv, kind)
    S2, gt2 = R.t2v_case(Nv, kind)
    assert S.tobytes() == S2.tobytes() and np.array_equal(gt, gt2)                # the same bytes for the host and the GPU tests
    assert S.shape == (R.T2V_NT, Nv) and S.dtype == np.float32 and gt.dtype == np.int32
    n4 = Nv & ~3
    vec = gt[gt < n4]
    if n4:
        assert set((vec % 4).tolist()) == {0, 1, 2, 3}                            # each float4 component
    assert set(range(n4, Nv)) <= set(gt.tolist()) and Nv - 1 in gt                # the scalar tail, the last column
    # under a lowered threshold the ground truth's own entry would count if it were not excluded: in every component and the tail
    sg = S[np.arange(len(gt)), gt]
    low = R.lowered(sg)
    beats = sg > low
    assert (low <= sg).all() and low.dtype == np.float32 and beats.any()
    assert np.array_equal(R.t2v_counts(S, gt, 0, low) + beats, (S > low[:, None]).sum(axis=1))
    if kind != 'special':
        assert beats.all() and np.isneginf(low[0::2]).all() and np.isfinite(low[1::2]).all()
    tied = R.rows_tied_with_gt(S, gt)
    if R.t2v_tie_heavy(Nv, kind):
        assert tied >= 0.25, tied
    if kind == 1:
        assert (R.t2v_counts(S, gt) == 0).all()                                   # everything ties: rank 1 everywhere
    if kind == 'special' and Nv >= 45:
        sg = S[np.arange(len(gt)), gt]
        assert np.isposinf(sg).any() and np.isneginf(sg).any() and (sg == 0).any()
        zero_rows = np.nonzero(sg == 0)[0]
        assert any(np.signbit(S[t][S[t] == 0]).any() and not np.signbit(S[t][S[t] == 0]).all() for t in zero_rows)
    counts = R.t2v_counts(S, gt)
    if Nv >= 45 and kind != 1:
        assert len(set(counts.tolist())) > 3                                      # and the counts are no constant


@pytest.mark.parametrize('i', range(len(R.V2T_CASES)))
def test_v2t_cases_contain_sibling_and_stranger_ties(i):
    mix, Nv, levels = R.V2T_CASES[i]
    S, owner = R.v2t_case(i)
    sizes = np.bincount(owner, minlength=Nv)
    assert sizes.max() == max(mix) and len(owner) <= 4000 and S.shape == (len(owner), Nv)
    assert (len(mix) == 1) == (sizes.min() > 0)                                   # a mix of several sizes has a video without captions
    if len(mix) > 1:
        assert 0 in mix and Nv > len(mix)
    own = S[np.arange(len(owner)), owner]
    col = S[:, owner].T                                                           # col[t] = the column of t's video
    same = col == own[:, None]
    sibling = same & (owner[None, :] == owner[:, None]) & ~np.eye(len(owner), dtype=bool)
    stranger = same & (owner[None, :] != owner[:, None])
    if levels is None:
        assert len(np.unique(S)) == S.size
    else:
        if max(mix) > 1:
            assert sibling.any(axis=1).mean() >= 0.25
        if Nv > 1:
            assert stranger.any(axis=1).mean() >= 0.25


def test_v2t_cases_cover_every_instantiation_and_pass_count():
    """maxima on both sides of each switch of launch_v2t_count (G = 4 / 8 / 16 / 32) and one, two and three passes of G = 32"""
    maxima = {max(m) for m, _, _ in R.V2T_CASES}
    assert maxima == {1, 4, 5, 8, 9, 16, 17, 32, 33, 70}
    assert {Nv for _, Nv, _ in R.V2T_CASES} == {1, 31, 32, 33, 97}
    assert {lv for _, _, lv in R.V2T_CASES} == {2, 7, None}
    assert sum(len(m) == 1 for m, _, _ in R.V2T_CASES) >= 4


def test_topk_cases_tie_across_the_kth_place():
    from laff_amd import ops
    for K in R.TOPK_K:
        cap = ops.topk_max_columns(K)
        sizes = R.topk_sizes(K, cap)
        assert sizes[0] == K and sizes[1] == K + 1 and K < sizes[2] <= cap
        for Nv, wide in zip(sizes, (False, False, True)):
            S = R.topk_case(K, Nv, wide)
            if Nv == K:
                continue
            srt = -np.sort(-S, axis=1)
            straddle = srt[:, K - 1] == srt[:, K]
            if wide:
                run = (S == srt[:, K - 1][:, None]).sum(axis=1)
                assert straddle.all() or K == 1
                assert straddle[2:].all() and (run[2:] > 2 * K).all()             # a run of equals far longer than K
            else:
                rows = R.TOPK_SPECIAL_ROWS
                assert straddle[rows['equal']] and not straddle[rows['ascending']] and not straddle[rows['descending']]
                assert (np.diff(S[rows['ascending']]) > 0).all() and (np.diff(S[rows['descending']]) < 0).all()
                if K >= 63:
                    assert straddle[rows['levels3']]


def test_merge_cases_need_the_group_merge_and_tie_across_blocks():
    from laff_amd import ops
    Nt, Nv, K = R.MERGE_SHAPE
    cap = ops.topk_max_columns(K)
    nblocks = -(-Nv // cap)
    candidates = sum(min(K, min(Nv, c0 + cap) - c0) for c0 in range(0, Nv, cap))
    assert candidates > cap and nblocks == 4                                      # the `while cand_v.shape[1] > cap` loop runs
    group = max(2, cap // K) * K
    assert -(-candidates // group) >= 2                                           # ... over more than one group
    S = R.merge_case_planted(cap)
    idx, val = R.topk(S, K)
    for r in range(Nt):
        tied = np.nonzero(S[r] == val[r, K - 1])[0]
        taken = np.intersect1d(tied, idx[r])
        assert len(tied) == 7 and len(taken) == 3 and np.array_equal(taken, tied[-3:])
        assert len(set((tied // cap).tolist())) >= 3                              # the tie spans blocks ...
        assert len(set((tied // cap // 2).tolist())) == 2                         # ... and both merge groups
        inside = np.nonzero(S[r] == np.float32(2.5))[0]
        assert len(inside) == 7 and set((inside // cap).tolist()) == {0, 1, 2, 3} and np.isin(inside, idx[r]).all()
    Q = R.merge_case_quantised()
    srt = -np.sort(-Q, axis=1)
    assert (srt[:, K - 1] == srt[:, K]).all() and ((Q == srt[:, K - 1][:, None]).sum(axis=1) > 2 * K).all()


def test_writer_and_hist_cases_are_tie_heavy():
    S, vis_ids, txt_ids = R.writer_case()
    srt = -np.sort(-S, axis=1)
    assert len(vis_ids) == S.shape[1] == 37 and len(txt_ids) == 6
    assert (srt[:, 19] == srt[:, 20]).all() and (srt[:, 35] == srt[:, 36]).any()  # ties across K = 20 and across K = Nv - 1
    assert len(R.writer_lines(S, vis_ids, txt_ids, 20)[0].split()) == 41
    T, V, gt = R.hist_case()
    Nt, Nv, _ = R.HIST_SHAPE
    assert T.shape[0] == Nt and V.shape[0] == Nv and np.bincount(gt, minlength=Nv).min() >= 1
    inter = np.minimum(T[:, None], V[None]).sum(-1)
    union = np.maximum(T[:, None], V[None]).sum(-1)
    assert union.min() >= 1 and union.max() <= 18
    # equal (intersection, union) pairs are equal scores in any arithmetic that is a function of the two integers
    pair = (inter * 64 + union).astype(np.int64)
    assert R.rows_tied_with_gt(pair, gt) >= 0.25
    col_ties = np.mean([len(np.unique(pair[:, v])) < Nt for v in range(Nv)])
    assert col_ties == 1.0
