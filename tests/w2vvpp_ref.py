"""float64 numpy restatement of the W2VV++ concat towers, written from the formulas:

    vis:  y = BN(tanh(cat_k(X_k) W^T + b))          txt:  y = BN(tanh(cat_e(F_e) W^T + b))
    score = cosine(y_txt, y_vis)                    BN (eval) = (y - running_mean) / sqrt(running_var + 1e-5) * weight + bias
"""
import numpy as np

ACTS = {None: lambda y: y, 'none': lambda y: y, 'tanh': np.tanh, 'relu': lambda y: np.maximum(y, 0.0),
        'sigmoid': lambda y: 1.0 / (1.0 + np.exp(-y))}


def tower(segments, W, bias=None, bn=None, activation='tanh', eps=1e-5):
    """segments: matrices of N rows in column order; W (D, sum widths); bn: None or (weight, bias, running_mean, running_var)."""
    x = np.concatenate([np.asarray(s, np.float64) for s in segments], axis=1)
    y = x @ np.asarray(W, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    y = ACTS[activation](y)
    if bn is not None:
        g, b, m, v = (np.asarray(t, np.float64) for t in bn)
        y = (y - m) / np.sqrt(v + eps) * g + b
    return y


def folded_bn(bn, eps=1e-5):
    """(scale, shift) of the eval-mode BatchNorm in float64."""
    g, b, m, v = (np.asarray(t, np.float64) for t in bn)
    scale = g / np.sqrt(v + eps)
    return scale, b - m * scale


def cosine(t, v):
    t = np.asarray(t, np.float64)
    v = np.asarray(v, np.float64)
    return (t / np.linalg.norm(t, axis=1, keepdims=True)) @ (v / np.linalg.norm(v, axis=1, keepdims=True)).T


def tower_from_sd(sd, prefix, segments, activation='tanh'):
    """sd: {key: array}; prefix 'vis_net.' or 'txt_net.transformer.'."""
    bn = None
    if prefix + 'bn1.weight' in sd:
        bn = tuple(sd[prefix + 'bn1.' + k] for k in ('weight', 'bias', 'running_mean', 'running_var'))
    return tower(segments, sd[prefix + 'fc1.weight'], sd[prefix + 'fc1.bias'], bn, activation)


def ranks_of_gt(S, gt):
    """1-based rank of column gt[i] in row i of S (descending; ties count against the ground truth like a strict '>' count + 1)."""
    s_gt = S[np.arange(S.shape[0]), gt]
    return (S > s_gt[:, None]).sum(axis=1) + 1


def gt_margin(S, gt):
    """min over the other columns of |s - s_gt| per row."""
    d = np.abs(S - S[np.arange(S.shape[0]), gt][:, None])
    d[np.arange(S.shape[0]), gt] = np.inf
    return d.min(axis=1)
