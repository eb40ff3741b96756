"""A float64 numpy restatement of the reference's NetVLAD text encoder (model/Attention.py:862-918 NetVLAD.forward over
W2Vec.raw_encoding rows): the checker of tests/test_netvlad_host.py and tests/test_gpu_netvlad.py."""
import numpy as np


def _normalize(x, axis):
    return x / np.maximum(np.linalg.norm(x, axis=axis, keepdims=True), 1e-12)


def netvlad_row(X, fc1, cent):
    """One caption: X (M, D) its rows (M may be 0) -> (K * D,) float64."""
    X, fc1, cent = (np.asarray(a, np.float64) for a in (X, fc1, cent))
    K, D = cent.shape
    if len(X) == 0:
        return np.zeros(K * D)
    Xh = _normalize(X, 1)
    logit = Xh @ fc1.T
    a = np.exp(logit - logit.max(1, keepdims=True))
    a /= a.sum(1, keepdims=True)
    u = a.T @ Xh - a.sum(0)[:, None] * cent
    return _normalize(_normalize(u, 1).reshape(-1), 0)


def netvlad_features(rows, table, fc1, cent):
    """rows: per caption (ids, token count) as W2Vec.raw_ids returns them; a caption without ids stands for that many zero rows."""
    table = np.asarray(table, np.float64)
    D = table.shape[1]
    return np.stack([netvlad_row(table[ids] if len(ids) else np.zeros((n, D)), fc1, cent) for ids, n in rows]) if rows else \
        np.zeros((0, np.asarray(cent).size))
