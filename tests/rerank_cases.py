"""Generated inputs for the stage-by-stage re-ranking checks, and the table of cases (tests/test_gpu_rerank.py compares the device
with them, tests/test_rerank_host.py holds their conditions without a GPU).

Every generated case sits on no tie BY CONSTRUCTION, because a seed search cannot find one past a few hundred items:
  * every block value is a multiple of 2^-17 in [-1, 1]: 2 - 2 x is then exact in fp32, the column maximum is bit-equal to float64's
    and the division is D's only rounding (<= 6e-8);
  * rerank_ref.neighbour_gap >= 2e-6 in float64, 32 times that rounding, so the fp32 neighbour lists are the float64 lists.
`check_inputs` asserts both; nothing is ever left out of a comparison.
"""
import functools

import numpy as np

import rerank_ref as R

UNIT = 1 << 17                 # block values are integers / 2^17
STEP = 16                      # 2^-13 in those units: the spacing of the repaired list values
MIN_GAP = 2e-6
DIM = 24


def _respace(x, top):
    """x: integer columns.  In every column the `top` largest values are made at least STEP apart, largest first
    (v_t <- min(v_t, v_{t-1} - STEP)), and the rest is clamped below the last of them."""
    s = np.ascontiguousarray(x.T)                           # a column per row: sorted along the contiguous axis
    order = np.argsort(-s, axis=1, kind='stable')
    s = np.take_along_axis(s, order, axis=1)
    top = min(top, s.shape[1])
    for t in range(1, top):
        s[:, t] = np.minimum(s[:, t], s[:, t - 1] - STEP)
    s[:, top:] = np.minimum(s[:, top:], s[:, top - 1:top] - STEP)
    out = np.empty_like(s)
    np.put_along_axis(out, order, s, axis=1)
    out = np.ascontiguousarray(out.T)
    return out


def lattice_blocks(seed, Q, G, k1, per=8, noise=0.45):
    """fp32 blocks (q_g, q_q, g_g) of Q + G cluster-planted unit embeddings (the fixture generator's recipe, in float64), their cosines
    rounded to multiples of 2^-13 and every column of the block matrix repaired so that its k1 + 4 largest values are 2^-13 apart.
    q_g is read in both positions of the block matrix (row j of it is most of query j's column, column g of it is part of gallery
    item g's): it is repaired in the query columns first and query j's values are moved up by (2 j + 1) 2^-17, so that in a gallery
    column they tie with no g_g value (a multiple of 2^-13) and with no other query's; then the g_g columns are repaired alone."""
    assert 2 * Q + 1 < STEP
    g = np.random.default_rng(seed)
    n = Q + G
    centres = g.normal(0, 1, (n // per + 2, DIM))
    e = centres[g.integers(0, len(centres), n)] + noise * g.normal(0, 1, (n, DIM))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    c = np.minimum(np.rint(e @ e.T * (UNIT // STEP)).astype(np.int64) * STEP, UNIT - STEP)
    c[np.arange(n), np.arange(n)] = UNIT
    qq, qg, gg = c[:Q, :Q].copy(), c[:Q, Q:].copy(), c[Q:, Q:].copy()
    cols = _respace(np.concatenate([qq, qg.T], axis=0), k1 + 4)        # column j: q_q[:, j], then q_g[j, :]
    cols += 2 * np.arange(Q)[None, :] + 1
    cols[np.arange(Q), np.arange(Q)] = UNIT
    qq, qg = cols[:Q], np.ascontiguousarray(cols[Q:].T)
    gg = _respace(gg, k1 + 4)
    return tuple(np.ascontiguousarray(a / float(UNIT), dtype=np.float32) for a in (qg, qq, gg))


Q45 = round(0.45 * UNIT) / UNIT


def ring_offsets(k1):
    offs = [0, 100, -100, 200, -200]
    for d in range(1, k1):
        offs += [d, -d]
    return offs[:k1 + 1]


def ring_blocks(G, k1=32, seed=0):
    """One query and G gallery items on a ring, the neighbour lists written down: column i of g_g holds 1 - t 2^-7 at row
    (i + o_t) mod G for the k1 + 1 offsets 0, +100, -100, +200, -200, +1, -1, +2, ... (the first kh + 1 are the half list) and -0.5
    elsewhere; q_g is -0.5 except 40 random columns at 0.45 - t 2^-7.  The far offsets make the expansion sets and the
    query-expanded rows several times as long as clustered embeddings give."""
    assert G >= 402 and k1 + 1 <= 64
    gg = np.full((G, G), -0.5)
    for t, o in enumerate(ring_offsets(k1)):
        gg[(np.arange(G) + o) % G, np.arange(G)] = 1.0 - t / 128.0
    qg = np.full((1, G), -0.5)
    qg[0, np.random.default_rng(seed).choice(G, 40, replace=False)] = Q45 - np.arange(40) / 128.0
    return qg.astype(np.float32), np.ones((1, 1), dtype=np.float32), gg.astype(np.float32)


def plant_ties(blocks, k1):
    """Exact ties in D, in six gallery columns of a lattice case: one list value copied onto another g_g entry of the column, whose
    index is 64 away (the same lane of the arg-min), 1 away (the neighbouring lane) or far away -- each once inside the list
    (positions 4 and 5) and once across its end (positions k1 and k1 + 1, where the lower index must get in).  Returns the blocks
    and the planted (row of D, position of the first of the two equal values)."""
    q_g, q_q, g_g = (np.array(a) for a in blocks)
    Q, G = q_g.shape
    N = Q + G
    assert N >= 130
    order = np.argsort(R.distances(q_g, q_q, g_g), axis=1, kind='stable')[:, :k1 + 4]
    far = N // 2
    while far % 64 in (0, 1, 63):
        far += 1
    planted, g = [], 0
    for t in (4, k1):
        for d in (64, 1, far):
            while True:
                assert g < G, 'no column left to plant a tie in'
                i, a = Q + g, int(order[Q + g, t])
                g += 1
                b = [b for b in (a - d, a + d) if Q <= b < N and b not in order[i]]
                if a >= Q and b:
                    g_g[b[0] - Q, i - Q] = g_g[a - Q, i - Q]
                    planted.append((i, t))
                    break
    return (q_g, q_q, g_g), planted


def check_inputs(blocks, k1, planted=()):
    """the condition every generated case must meet; returns the gap (of all pairs but the planted ones)"""
    for a in blocks:
        assert a.dtype == np.float32 and np.abs(a).max() <= 1.0
        assert np.array_equal(a.astype(np.float64) * UNIT, np.rint(a.astype(np.float64) * UNIT))
    d = np.diff(R.list_head(R.distances(*blocks), k1), axis=1)
    for i, t in planted:
        assert d[i, t] == 0.0, (i, t)
        d[i, t] = np.inf
    gap = float(d.min())
    assert gap >= MIN_GAP, gap
    return gap


#: name -> (Q, G, k1, k2, how the blocks are made)
CASES = {
    # the smallest problems, N = k1 + 1: every list is the whole problem and L1 = N clamps
    'n2': (1, 1, 1, 1, dict(seed=1)),
    'n2_k2': (1, 1, 1, 2, dict(seed=2)),
    'n6': (1, 5, 5, 3, dict(seed=3)),
    'n33': (1, 32, 32, 8, dict(seed=4)),
    'n33_q2': (2, 31, 32, 8, dict(seed=5)),
    # the tail block of the four-items-per-block kernels and the lane edge of the 64-wide scans
    'n63': (3, 60, 20, 6, dict(seed=6)),
    'n64': (3, 61, 20, 6, dict(seed=7)),
    'n65': (3, 62, 20, 6, dict(seed=8)),
    'n66': (3, 63, 20, 6, dict(seed=9)),
    'n67': (3, 64, 20, 6, dict(seed=10)),
    # G around the 64-item block of the Jaccard pass
    'g64_q1': (1, 64, 32, 8, dict(seed=11)),
    'g65_q1': (1, 65, 32, 8, dict(seed=12)),
    'g128_q1': (1, 128, 32, 8, dict(seed=13)),
    'g129_q1': (1, 129, 32, 8, dict(seed=14)),
    'g64_q5': (5, 64, 20, 6, dict(seed=15)),
    'g65_q5': (5, 65, 20, 6, dict(seed=16)),
    'g128_q5': (5, 128, 20, 6, dict(seed=17)),
    'g129_q5': (5, 129, 20, 6, dict(seed=18)),
    # mid sizes at the largest k1
    'n257': (5, 252, 32, 8, dict(seed=19)),
    'n1030': (3, 1027, 32, 8, dict(seed=24, per=8, noise=0.45)),
    'n1030_k2_1': (5, 1025, 32, 1, dict(seed=21, per=100, noise=0.6)),
    # every limit at once
    'n4096': (2, 4094, 32, 8, dict(seed=22)),
    # designed lists: the second trip of the expansion write-out, the second and third of the Jaccard scatter
    'ring': (1, 1028, 32, 8, 'ring'),
    'ring_k2_1': (1, 1028, 32, 1, 'ring'),
    # exact ties
    'ties': (3, 1027, 32, 8, 'ties'),
}
SMALLEST = ['n2', 'n2_k2', 'n6', 'n33', 'n33_q2']
GROUP = ['n33', 'n1030', 'g64_q1', 'n257']        # one launch group of unequal problems at k1 = 32, k2 = 8; N = 33, 1030, 65, 257
LAMBDA_CASE = 'n257'
STAGES = ('val1', 'val2', 'out')


@functools.lru_cache(maxsize=None)
def blocks_of(name):
    Q, G, k1, k2, how = CASES[name]
    if how == 'ring':
        return ring_blocks(G, k1), ()
    if how == 'ties':
        return plant_ties(blocks_of('n1030')[0], k1)
    return lattice_blocks(Q=Q, G=G, k1=k1, **how), ()


def _flat(rows):
    return np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1) for r in rows])


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def bound(e32, want):
    """the project's rule for an fp32 result against float64: max(2 e32, 4 ulp of the largest value)"""
    return max(2.0 * float(e32), 4.0 * ulp32(want))


@functools.lru_cache(maxsize=None)
def case(name, lambda_value=0.3):
    """The inputs of a case, checked, its float64 stages, and per stage e32 = the fp32 rendering's |fp32 - fp64| and the bound that
    follows from it.  Computed once per process; nobody writes to it."""
    Q, G, k1, k2, _ = CASES[name]
    blocks, planted = blocks_of(name)
    assert blocks[0].shape == (Q, G) and blocks[1].shape == (Q, Q) and blocks[2].shape == (G, G)
    gap = check_inputs(blocks, k1, planted)
    s64 = R.stages(*blocks, k1, k2, lambda_value)
    s32 = R.stages(*blocks, k1, k2, lambda_value, dtype=np.float32, sets=s64['sets'])
    # the fp32 lists are the float64 lists, and the column maxima are bit-equal
    assert np.array_equal(s32['rank'], s64['rank']) and np.array_equal(s32['colmax'].astype(np.float64), s64['colmax'])
    assert all(np.array_equal(a, b) for a, b in zip(s32['idx2'], s64['idx2']))
    e32, bnd = {}, {}
    for st in STAGES:
        want = _flat(s64[st])
        e32[st] = float(np.abs(_flat(s32[st]) - want).max())
        bnd[st] = bound(e32[st], want)
    return dict(name=name, Q=Q, G=G, N=Q + G, k1=k1, k2=k2, lambda_value=lambda_value, blocks=blocks, planted=planted, gap=gap,
                s64=s64, e32=e32, bound=bnd, cnt1=max(len(e) for e in s64['idx1']), cnt2=max(len(e) for e in s64['idx2']))
