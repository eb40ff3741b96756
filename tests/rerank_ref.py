"""float64 restatement of k-reciprocal re-ranking (Zhong et al., CVPR 2017) and of the neighbour-count re-ranking, written from
the formulas in include/laff_hip.h -- what the device results are checked against.

    orig = 2 - 2 [[qq, qg], [qg^T, gg]];  D[i, j] = orig[j, i] / max_k orig[k, i]
    rank[i] = the k1 + 1 smallest entries of D[i, :], ascending
    R(i, k) = { j in rank[i][:k+1] : i in rank[j][:k+1] };  kh = round_half_even(k1 / 2)
    E(i) = R(i, k1) + every R(c, kh), c in R(i, k1), with |R(c, kh) & R(i, k1)| > 2/3 |R(c, kh)|
    V[i, e] = exp(-D[i, e]) / sum over E(i);  k2 != 1: V[i] <- mean of V[rank[i][:k2]]
    m[i, j] = sum_k min(V[i, k], V[j, k]);  final[i, g] = (1 - m / (2 - m)) (1 - lambda) + D[i, Q + g] lambda
"""
import numpy as np


def round_half_even(k1):
    h = k1 // 2
    return h if k1 % 2 == 0 else (h + 1 if h % 2 else h)


def overlap_float(n_both, n_set):
    """the overlap test as the reference writes it (float64)"""
    return n_both > 2. / 3 * n_set


def overlap_int(n_both, n_set):
    """... and as the kernel evaluates it"""
    return 3 * n_both > 2 * n_set


def _blocks(q_g, q_q, g_g, dtype):
    return tuple(np.asarray(a, dtype=dtype) for a in (q_g, q_q, g_g))


def _orig(q_g, q_q, g_g, dtype):
    q_g, q_q, g_g = _blocks(q_g, q_q, g_g, dtype)
    two = np.dtype(dtype).type(2)
    return two - two * np.block([[q_q, q_g], [q_g.T, g_g]])


def distances(q_g, q_q, g_g, dtype=np.float64):
    orig = _orig(q_g, q_q, g_g, dtype)
    return np.ascontiguousarray((orig / orig.max(axis=0, keepdims=True)).T)


def neighbour_lists(D, k1):
    return np.argsort(D, axis=1, kind='stable')[:, :k1 + 1]


def list_head(D, k1):
    """the k1 + 2 smallest values of every row of D, ascending"""
    n = min(k1 + 2, D.shape[1])
    return np.sort(np.partition(D, n - 1, axis=1)[:, :n], axis=1)


def neighbour_gap(q_g, q_q, g_g, k1):
    """the smallest difference between two of the k1 + 2 smallest values of a row of D, over all rows: how far every neighbour
    list (and its boundary) is from a tie"""
    return float(np.diff(list_head(distances(q_g, q_q, g_g), k1), axis=1).min())


def reciprocal(rank, i, k):
    return [int(j) for j in rank[i, :k + 1] if i in rank[j, :k + 1]]


def expansion_sets(rank, k1):
    """the definition, item by item (slow: seconds at N = 1000); expansion_sets_fast is held equal to it"""
    kh = round_half_even(k1)
    out = []
    for i in range(rank.shape[0]):
        ri = reciprocal(rank, i, k1)
        e = set(ri)
        for c in ri:
            rc = reciprocal(rank, c, kh)
            if overlap_float(len(set(rc) & set(ri)), len(rc)):
                e.update(rc)
        out.append(sorted(e))
    return out


def _reciprocity(rank, k):
    N = rank.shape[0]
    m = np.zeros((N, N), dtype=bool)
    m[np.arange(N)[:, None], rank[:, :k + 1]] = True
    return m & m.T


def expansion_sets_fast(rank, k1):
    """expansion_sets with the reciprocity test as two boolean N x N matrices: sorted int64 index arrays"""
    r1, rh = _reciprocity(rank, k1), _reciprocity(rank, round_half_even(k1))
    nh = rh.sum(axis=1)
    out = []
    for i in range(rank.shape[0]):
        ri = np.flatnonzero(r1[i])
        sub = rh[ri]
        take = overlap_float((sub & r1[i]).sum(axis=1), nh[ri])
        out.append(np.flatnonzero(r1[i] | sub[take].any(axis=0)))
    return out


def stages(q_g, q_q, g_g, k1, k2, lambda_value, dtype=np.float64, sets=None):
    """Every intermediate the kernels materialise, in `dtype` arithmetic and in the reference's order of operations (np.sum of the
    weights, np.mean over the k2 rows, the minima accumulated in index order, the blend): with dtype=np.float32 this is the
    reference's own fp32 computation, whose distance from the float64 run is what a tolerance is derived from.

    Returns a dict: colmax [N], rank [N, k1+1], D [Q, N] (the query rows), sets (the expansion sets: sorted index arrays),
    idx1 / val1 (the sparse rows of V: here idx1 is sets), idx2 / val2 (the rows after query expansion, membership != 0; the same
    objects as idx1 / val1 at k2 = 1), out [Q, G].  `sets`: expansion sets computed before from the same lists (they depend on
    rank alone)."""
    dt = np.dtype(dtype).type
    Q = np.asarray(q_g).shape[0]
    orig = _orig(q_g, q_q, g_g, dt)
    colmax = orig.max(axis=0)
    D = np.ascontiguousarray((orig / colmax).T)
    del orig
    N = D.shape[0]
    rank = neighbour_lists(D, k1)
    if sets is None:
        sets = expansion_sets_fast(rank, k1)
    V = np.zeros((N, N), dtype=dt)
    idx1, val1 = [], []
    for i, e in enumerate(sets):
        e = np.asarray(e, dtype=np.int64)
        w = np.exp(-D[i, e])
        v = w / np.sum(w)
        V[i, e] = v
        idx1.append(e)
        val1.append(v)
    idx2, val2 = idx1, val1
    if k2 != 1:
        Vq = np.empty_like(V)
        for i in range(N):
            Vq[i] = np.mean(V[rank[i, :k2]], axis=0)
        V = Vq
        idx2 = [np.flatnonzero(V[i]) for i in range(N)]
        val2 = [V[i, e] for i, e in enumerate(idx2)]
    jac = np.empty((Q, N), dtype=dt)
    for i in range(Q):
        m = np.zeros(N, dtype=dt)
        for k in idx2[i]:                                   # index order, as the reference walks np.where(V[i] != 0)
            m += np.minimum(V[i, k], V[:, k])
        jac[i] = dt(1) - m / (dt(2) - m)
    final = jac * dt(1.0 - lambda_value) + D[:Q] * dt(lambda_value)
    return dict(Q=Q, N=N, colmax=colmax, rank=rank, D=D[:Q].copy(), sets=sets, idx1=idx1, val1=val1, idx2=idx2, val2=val2,
                out=np.ascontiguousarray(final[:, Q:]))


def re_ranking(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3):
    return stages(q_g, q_q, g_g, k1, k2, lambda_value)['out']


def workspace_layout(sizes, k1, k2):
    """Where laff_rerank_run keeps what in its workspace (rerank_layout in api.hip): per problem {name: (byte offset, shape, 'i' or
    'f')} in the order rank, colmax, cnt1, idx1, val1 and for k2 != 1 cnt2, idx2, val2 (at k2 = 1 they are the first three again),
    every piece rounded up to 256 bytes, L1 = min(cap, N), L2 = min(k2 cap, N), cap = (k1 + 1)(kh + 2); problems follow one another.
    Returns (the list of these dicts, the total bytes)."""
    cap = (k1 + 1) * (round_half_even(k1) + 2)
    o, out = 0, []
    for Q, G in sizes:
        N = Q + G
        L1, L2 = min(cap, N), min(k2 * cap, N)
        pieces = [('rank', (N, k1 + 1), 'i'), ('colmax', (N,), 'f'), ('cnt1', (N,), 'i'), ('idx1', (N, L1), 'i'), ('val1', (N, L1), 'f')]
        if k2 != 1:
            pieces += [('cnt2', (N,), 'i'), ('idx2', (N, L2), 'i'), ('val2', (N, L2), 'f')]
        d = {}
        for name, shape, kind in pieces:
            d[name] = (o, shape, kind)
            o += (4 * int(np.prod(shape)) + 255) // 256 * 256
        if k2 == 1:
            d.update(cnt2=d['cnt1'], idx2=d['idx1'], val2=d['val1'])
        out.append(d)
    return out, o


def workspace_views(ws, sizes, k1, k2):
    """the workspace of ops.rerank_run (a uint8 tensor) as named int32 / fp32 tensor views, one dict per problem"""
    import torch
    layout, total = workspace_layout(sizes, k1, k2)
    assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() >= total
    return [{name: ws[o:o + 4 * int(np.prod(shape))].view(torch.int32 if kind == 'i' else torch.float32).view(shape)
             for name, (o, shape, kind) in d.items()} for d in layout]


def tkb_counts(g_g, k1):
    """count[v] = 1 + #{u : v among the k1 largest of g_g[u]}"""
    g_g = np.asarray(g_g, dtype=np.float64)
    nn = np.argsort(-g_g, axis=1, kind='stable')[:, :k1]
    return 1 + np.bincount(nn.reshape(-1), minlength=g_g.shape[0])


def re_ranking_tkb_simple(q_g, q_q, g_g, topK=3000, k1=20):
    q_g = np.asarray(q_g, dtype=np.float64)
    count = tkb_counts(g_g, k1)
    out = np.zeros(q_g.shape)
    for r in range(q_g.shape[0]):
        c = np.argsort(-q_g[r], kind='stable')[:topK]
        out[r, c] = np.log(count[c] + 1.0)
    return out / (np.sqrt((out ** 2).sum(axis=1, keepdims=True)) + 1e-13 + 1e-14)


def l2norm_rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x / (np.sqrt((x ** 2).sum(axis=1, keepdims=True)) + 1e-13 + 1e-14)
