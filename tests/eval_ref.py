"""The score-matrix evaluation tail (gather_gt / rank_count, v2t_count, topk_rows, predictor.v2t_metrics, the result writers) restated
in plain numpy, and the generators of the tie-heavy inputs its tests share.

Everything is integer counting or exact selection on the float32 values as given; the only floating-point arithmetic is the float64
means of the seven metrics.  The conventions:

    text -> video   count[t] = #{c != gt[t] : S[t, c] >  S[t, gt[t]]}            strictly greater: a tie does not cost a place
    video -> text   count[t] = #{t' : S[t', owner[t]] > S[t, owner[t]]}          all rows, the video's other captions included
                    captions of one video with equal scores take consecutive places
    top-K           score descending, equal scores by LARGER index first          (a stable ascending argsort read backwards)

No torch, no device."""
import numpy as np

from oracle import laff_oracle as O


# ------------------------------------------------------------------------------------------------ reference
def gathered(S, gt, col0=0):
    """s_gt[t] = S[t, gt[t] - col0], -inf where that column is not in [0, Nv): what gather_gt_kernel writes for a column shard"""
    S = np.asarray(S)
    c = np.asarray(gt).astype(np.int64) - col0
    inside = (c >= 0) & (c < S.shape[1])
    out = np.full(S.shape[0], -np.inf, dtype=S.dtype)
    out[inside] = S[np.nonzero(inside)[0], c[inside]]
    return out


def t2v_counts(S, gt, col0=0, s_gt=None):
    """#{c != gt - col0 : S[t, c] > s_gt[t]} per row, int32; s_gt defaults to gathered(S, gt, col0)"""
    S = np.asarray(S)
    if s_gt is None:
        s_gt = gathered(S, gt, col0)
    c = np.asarray(gt).astype(np.int64) - col0
    inside = (c >= 0) & (c < S.shape[1])
    above = S > np.asarray(s_gt)[:, None]
    above[np.nonzero(inside)[0], c[inside]] = False
    return above.sum(axis=1).astype(np.int32)


def v2t_counts(S, owner):
    """#{t' : S[t', owner[t]] > S[t, owner[t]]} for every caption t, int32: strict, over all rows"""
    S, owner = np.asarray(S), np.asarray(owner).astype(np.int64)
    out = np.zeros(S.shape[0], dtype=np.int32)
    for v in np.unique(owner):
        members = np.nonzero(owner == v)[0]
        col = S[:, v]
        out[members] = (col[None, :] > col[members][:, None]).sum(axis=1)
    return out


def v2t_positions(S, owner):
    """Per video, the sorted 1-based places of its captions in its column: count + 1, and captions of one video with equal scores
    behind one another.  An empty array for a video without captions."""
    S, owner = np.asarray(S), np.asarray(owner).astype(np.int64)
    counts = v2t_counts(S, owner).astype(np.int64)
    out = []
    for v in range(S.shape[1]):
        c = np.sort(counts[owner == v])
        # equal counts <=> equal scores (same column, same comparison): the i-th of a run of equals stands i places behind the first
        run_start = np.searchsorted(c, c, side='left')
        out.append(c + 1 + (np.arange(len(c)) - run_start))
    return out


def v2t_metrics(S, owner):
    """(r1, r5, r10, medr, meanr, mir, mAP) of the video -> text direction; IndexError when a video has no caption"""
    return O.eval_from_positions(v2t_positions(S, owner))


def t2v_metrics(S, gt):
    return O.eval_from_positions([[int(c) + 1] for c in t2v_counts(S, gt)])


def topk(S, K):
    """(idx int32 (Nt, K), val (Nt, K)): the K best columns per row, larger index first among equal scores.  NaN is out of scope:
    where numpy's sort puts it is no contract of anybody's."""
    S = np.asarray(S)
    idx = np.argsort(S, axis=1, kind='stable')[:, ::-1][:, :K]
    return idx.astype(np.int32), np.take_along_axis(S, idx, axis=1)


# ------------------------------------------------------------------------------------------------ generators
def quantised(g, Nt, Nv, levels):
    """float32 (Nt, Nv) of values k / levels, k in [0, levels): the matrices of the 'hist' measure -- ratios of small integers, full of
    exact ties.  levels == 1: every entry is 0."""
    return (g.integers(0, levels, (Nt, Nv)) / np.float32(levels)).astype(np.float32)


def distinct(g, Nt, Nv):
    """float32 (Nt, Nv) without two equal entries"""
    n = Nt * Nv
    assert n < 2 ** 24
    return (g.permutation(n).reshape(Nt, Nv) / np.float32(n)).astype(np.float32)


def special(g, Nt, Nv):
    """+inf, -inf, -0.0, +0.0 and +-1 in equal shares: -0.0 == +0.0 must tie, nothing beats +inf, everything else beats -inf"""
    vals = np.array([np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0], dtype=np.float32)
    return vals[g.integers(0, len(vals), (Nt, Nv))]


def groups(g, Nv, sizes):
    """int32 owner vector: video v has sizes[v] captions (0 allowed), the texts in shuffled order"""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.shape == (Nv,) and (sizes >= 0).all()
    return g.permutation(np.repeat(np.arange(Nv), sizes)).astype(np.int32)


def spread(mix, Nv):
    """the caption counts of `mix` dealt over Nv videos in turn (the first, its maximum, always lands on video 0)"""
    return [mix[v % len(mix)] for v in range(Nv)]


# ---- text -> video cases
T2V_NT = 70
T2V_NV = (1, 3, 4, 5, 45, 64, 259)
T2V_KINDS = (1, 3, 50, 'special')          # quantisation levels, or the +-inf / +-0 matrix


def gt_cover(g, Nt, Nv):
    """Ground-truth columns that hit every column of the first and the last float4 of a row, every column of the scalar tail
    (Nv & ~3 .. Nv - 1) and the last column; the other rows at random."""
    must = sorted(set(range(min(4, Nv))) | set(range(max((Nv & ~3) - 4, 0), Nv)))
    assert len(must) <= Nt
    gt = g.integers(0, Nv, Nt)
    gt[g.permutation(Nt)[:len(must)]] = must
    return gt.astype(np.int32)


def t2v_case(Nv, kind):
    """(S float32 (70, Nv), gt int32 (70,)) of one case; the same bytes wherever it is asked for"""
    g = np.random.default_rng(9100 + 10 * Nv + T2V_KINDS.index(kind))
    S = special(g, T2V_NT, Nv) if kind == 'special' else quantised(g, T2V_NT, Nv, kind)
    return S, gt_cover(g, T2V_NT, Nv)


def t2v_tie_heavy(Nv, kind):
    """cases whose rows are expected to tie with the ground truth: few values against many columns.  (One column has nothing to tie
    with; 50 levels over 3-5 columns tie in a few rows in a hundred.)"""
    return Nv >= 3 and (kind in (1, 3, 'special') or Nv >= 45)


def lowered(s_gt):
    """A threshold handed in from elsewhere (a shard, another precision) that lies BELOW the ground truth's own entry: -inf in the even
    rows, the next float32 down in the odd ones.  Only then does `c != gt` decide anything -- the entry itself is never above itself."""
    out = np.nextafter(np.asarray(s_gt, dtype=np.float32), np.float32(-np.inf))
    out[0::2] = -np.inf
    return out


SHARD_BOUNDS = (0, 130, 133, 259)          # three column shards of the Nv = 259 cases; the middle one is 3 columns wide

# ---- video -> text cases: (caption counts dealt over the videos, Nv, score levels or None for a tie-free matrix)
V2T_CASES = [
    ((1,), 1, 2), ((1,), 33, 7), ((4, 0, 1, 3), 31, 2), ((5, 0, 2), 32, 7), ((8, 0, 3, 1), 33, None), ((9, 0, 4), 97, 2),
    ((16, 0, 7), 31, 7), ((17, 0, 1), 32, 2), ((32, 0, 5), 33, 7), ((33, 0, 2, 32), 97, None), ((70, 0, 33, 1), 97, 2),
    ((5,), 31, 2), ((33,), 32, 7), ((70,), 1, 7), ((16,), 97, None), ((8,), 33, 2), ((9,), 32, 7),
]


def v2t_case(i):
    """(S float32 (Nt, Nv), owner int32 (Nt,)) of V2T_CASES[i]"""
    mix, Nv, levels = V2T_CASES[i]
    g = np.random.default_rng(9300 + i)
    owner = groups(g, Nv, spread(mix, Nv))
    Nt = len(owner)
    return (distinct(g, Nt, Nv) if levels is None else quantised(g, Nt, Nv, levels)), owner


def ids_of(owner, Nv):
    """(txt_ids, vis_ids) in the `video#caption` protocol of predictor.gt_columns for an owner vector"""
    return ['vid%d#%d' % (v, t) for t, v in enumerate(owner)], ['vid%d' % v for v in range(Nv)]


# ---- top-K cases
TOPK_K = (1, 63, 64, 65, 512, 513, 2048, 2049, 4096, 4097, 8192)
TOPK_SPECIAL_ROWS = {'normal': 0, 'levels3': 1, 'equal': 2, 'ascending': 3, 'descending': 4}


def topk_matrix(g, Nv):
    """float32 (5, Nv): normal scores of which the first third is rounded to one decimal; 3-level quantised; all equal; strictly
    ascending; strictly descending"""
    S = np.empty((5, Nv), dtype=np.float32)
    S[0] = g.normal(0, 1, Nv)
    S[0, : Nv // 3] = np.round(S[0, : Nv // 3], 1)
    S[1] = quantised(g, 1, Nv, 3)[0]
    S[2] = 0.25
    S[3] = np.arange(Nv, dtype=np.float32) - Nv // 2
    S[4] = S[3, ::-1]
    return S


def topk_wide_matrix(g, Nv):
    """float32 (4, Nv) of long runs of equal values: two 3-level rows, a row that is all equal but for five larger entries, and a
    1-level row"""
    S = np.empty((4, Nv), dtype=np.float32)
    S[0:2] = quantised(g, 2, Nv, 3)
    S[2] = 0.5
    S[2, g.permutation(Nv)[:min(5, Nv)]] = 0.75
    S[3] = 0.0
    return S


def topk_sizes(K, cap):
    """the three widths of one K: K, K + 1, and a wide one (8 K + 37 columns, or as many as one kernel call takes: `cap`)"""
    return K, K + 1, min(8 * K + 37, cap)


def topk_case(K, Nv, wide):
    g = np.random.default_rng(9500 + 3 * K + Nv % 3)
    return topk_wide_matrix(g, Nv) if wide else topk_matrix(g, Nv)


MERGE_SHAPE = (2, 73000, 8192)             # (Nt, Nv, K): more per-block candidates than one call takes, so block lists merge in groups


def merge_case_planted(block):
    """Normal scores, (2, 73000), with equal values planted in different column blocks (of `block` columns) and different merge groups:
    per row, a value well inside the best K at seven places, and the value of the (K - 2)-th place at six more places that were
    below the K-th -- so seven entries tie for the last three places, and the three largest indices must win them."""
    Nt, Nv, K = MERGE_SHAPE
    g = np.random.default_rng(9700)
    S = g.normal(0, 1, (Nt, Nv)).astype(np.float32)
    inside = [5, block - 1, block, 2 * block - 1, 2 * block, 3 * block, Nv - 1]
    edge = [[7, block - 2, block + 1, 2 * block + 3, 3 * block + 1, Nv - 2],              # every block, both merge groups
            [11, 12, 13, block - 3, block - 4, 3 * block + 2]]                            # the low blocks against the last one
    for r in range(Nt):
        S[r, inside] = 2.5
        S[r, edge[r]] = -9.0
        order = np.sort(S[r])[::-1]
        thr = order[K - 3]
        assert order[K - 4] > thr > order[K - 2]
        S[r, edge[r]] = thr
    return S


def merge_case_quantised():
    Nt, Nv, _ = MERGE_SHAPE
    return quantised(np.random.default_rng(9701), Nt, Nv, 3)


# ---- result-writer and end-to-end cases
def writer_case():
    """(S (6, 37) 3-level, vis_ids, txt_ids)"""
    S = quantised(np.random.default_rng(9800), 6, 37, 3)
    return S, ['video%d' % v for v in range(37)], ['video%d#0' % t for t in range(6)]


def writer_lines(S, vis_ids, txt_ids, K):
    """the lines of id.sent.score.txt for the K best of every row: `txt_id vis_id score vis_id score ...`, scores printed as numpy
    float32 (tests/golden/writers.npz holds the format to the original's output)"""
    idx, val = topk(S, K)
    return [t + ' ' + ' '.join('%s %s' % (vis_ids[i], v) for i, v in zip(idx[r], val[r])) for r, t in enumerate(txt_ids)]


HIST_SHAPE = (70, 45, 6)                   # (Nt, Nv, bins)


def hist_case():
    """(T (70, 6), V (45, 6) float32 counts in 0..3, gt int32 (70,) -- every video owns a caption): Jaccard scores of such rows are
    ratios of integers below 19 and tie all over the matrix"""
    Nt, Nv, K = HIST_SHAPE
    g = np.random.default_rng(9900)
    T, V = g.integers(0, 4, (Nt, K)).astype(np.float32), g.integers(0, 4, (Nv, K)).astype(np.float32)
    T[T.sum(axis=1) == 0, 0] = 1.0
    V[V.sum(axis=1) == 0, 0] = 1.0
    gt = g.permutation(np.concatenate([np.arange(Nv), g.integers(0, Nv, Nt - Nv)])).astype(np.int32)
    return T, V, gt


def rows_tied_with_gt(S, gt):
    """fraction of rows in which another column equals the ground truth's score"""
    S = np.asarray(S)
    sg = S[np.arange(S.shape[0]), gt]
    return float((((S == sg[:, None]).sum(axis=1) - 1) > 0).mean())
