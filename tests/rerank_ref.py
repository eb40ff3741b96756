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


def distances(q_g, q_q, g_g):
    q_g, q_q, g_g = (np.asarray(a, dtype=np.float64) for a in (q_g, q_q, g_g))
    orig = 2.0 - 2.0 * np.block([[q_q, q_g], [q_g.T, g_g]])
    return (orig / orig.max(axis=0, keepdims=True)).T


def neighbour_lists(D, k1):
    return np.argsort(D, axis=1, kind='stable')[:, :k1 + 1]


def neighbour_gap(q_g, q_q, g_g, k1):
    """the smallest difference between two of the k1 + 2 smallest values of a row of D, over all rows: how far every neighbour
    list (and its boundary) is from a tie"""
    s = np.sort(distances(q_g, q_q, g_g), axis=1)[:, :k1 + 2]
    return float(np.diff(s, axis=1).min())


def reciprocal(rank, i, k):
    return [int(j) for j in rank[i, :k + 1] if i in rank[j, :k + 1]]


def expansion_sets(rank, k1):
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


def re_ranking(q_g, q_q, g_g, k1=20, k2=6, lambda_value=0.3):
    Q = np.asarray(q_g).shape[0]
    D = distances(q_g, q_q, g_g)
    N = D.shape[0]
    rank = neighbour_lists(D, k1)
    V = np.zeros((N, N))
    for i, e in enumerate(expansion_sets(rank, k1)):
        w = np.exp(-D[i, e])
        V[i, e] = w / w.sum()
    if k2 != 1:
        V = np.stack([V[rank[i, :k2]].mean(axis=0) for i in range(N)])
    m = np.minimum(V[:Q, None, :], V[None, :, :]).sum(axis=2)
    final = (1.0 - m / (2.0 - m)) * (1.0 - lambda_value) + D[:Q] * lambda_value
    return final[:, Q:]


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
