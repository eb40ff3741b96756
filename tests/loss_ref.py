"""float64 restatement, with analytic gradients, of the criteria behind laff_dsl_loss, laff_margin_loss_scores and laff_margin_loss.

Written from the formulas, not from the reference's code:

    M = l2norm(s) . l2norm(im)^T,  n = B,  temperature t
    cal(X):  A = softmax of X / t down each column,  P = n X (.) A,  cal = -sum_i log softmax_row(P)[i][i]
             G = softmax_row(P) - I,   dX = n A G + (n / t) A (X G - colsum(A X G))
    dsl = (cal(M) + cal(M^T)) / 2, summed over heads

    margin on a score matrix: cost_s[i][j] = max(0, margin + score[i][j] - score[i][i]) ('i2t' / 'bidir'),
    cost_im[i][j] = max(0, margin + score[i][j] - score[j][j]) ('t2i' / 'bidir'), diagonal cleared; max_violation keeps the row maximum of
    cost_s and the column maximum of cost_im (first maximum on ties); 'sum' or 'mean' of each, added.

    margin on embeddings (laff_margin_loss): score = l2norm(im) . l2norm(s)^T per head (rows = videos, columns = captions), the loss
    above on it, chained through the two products and the normalisation, summed over heads.
"""
import numpy as np

EPS = 1e-13 + 1e-14      # l2norm: x / (|x| + eps + 1e-14)


def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def cal(X, temp):
    """(cal(X), d cal / dX) in float64."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    A = _softmax(X / temp, 0)
    P = n * X * A
    m = P.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(P - m).sum(axis=1))
    value = -(np.diag(P) - lse).sum()
    G = _softmax(P, 1) - np.eye(n)
    AXG = A * X * G
    dX = n * A * G + (n / temp) * (AXG - A * AXG.sum(axis=0, keepdims=True))
    return value, dX


def dsl_scores(M, temp):
    """(loss, dM) of (cal(M) + cal(M^T)) / 2."""
    l1, g1 = cal(M, temp)
    l2, g2 = cal(np.asarray(M, np.float64).T, temp)
    return 0.5 * (l1 + l2), 0.5 * (g1 + g2.T)


def _l2norm(x):
    r = np.sqrt((x * x).sum(axis=1, keepdims=True))
    return x / (r + EPS), r


def _l2norm_bwd(xh, r, g):
    """dx of x^ = x / (|x| + eps) given g = dL/dx^."""
    return g / (r + EPS) - xh * (xh * g).sum(axis=1, keepdims=True) / r


def dsl(s, im, temp=1000.0):
    """(loss, d_s, d_im) in float64 for s, im (B, d) or (B, H, d): DualSoftmaxLoss per head, summed."""
    s = np.asarray(s, np.float64)
    im = np.asarray(im, np.float64)
    flat = s.ndim == 2
    if flat:
        s, im = s[:, None, :], im[:, None, :]
    temp = float(temp)
    loss = 0.0
    d_s, d_im = np.zeros_like(s), np.zeros_like(im)
    for h in range(s.shape[1]):
        sh, rs = _l2norm(s[:, h])
        ih, ri = _l2norm(im[:, h])
        l, dM = dsl_scores(sh @ ih.T, temp)
        loss += l
        d_s[:, h] = _l2norm_bwd(sh, rs, dM @ ih)
        d_im[:, h] = _l2norm_bwd(ih, ri, dM.T @ sh)
    return (loss, d_s[:, 0], d_im[:, 0]) if flat else (loss, d_s, d_im)


def margin_scores(score, margin, max_violation, cost_style, direction):
    """(loss, d_score) in float64 of the margin ranking loss on a given (B, B) score matrix."""
    S = np.asarray(score, np.float64)
    B = S.shape[0]
    dg = np.diag(S)
    off = ~np.eye(B, dtype=bool)
    loss = 0.0
    dS = np.zeros_like(S)
    for name, ref, axis in (('i2t', dg[:, None], 1), ('t2i', dg[None, :], 0)):
        if direction not in (name, 'bidir'):
            continue
        cost = np.maximum(margin + S - ref, 0.0) * off
        if max_violation:
            w = 1.0 / B if cost_style == 'mean' else 1.0
            arg = cost.argmax(axis=axis)                      # the first maximum, as torch.max
            for q in range(B):
                i, j = (q, arg[q]) if axis == 1 else (arg[q], q)
                if cost[i, j] > 0.0:
                    loss += w * cost[i, j]
                    dS[i, j] += w
                    dS[q, q] -= w
        else:
            w = 1.0 / (B * B) if cost_style == 'mean' else 1.0
            act = cost > 0.0
            loss += w * cost.sum()
            dS += w * act
            dS[np.arange(B), np.arange(B)] -= w * act.sum(axis=axis)
    return loss, dS


def margin_scores_slack(score, margin, max_violation, direction):
    """The smallest distance of any decision of margin_scores from flipping, in float64: |hinge argument| of every off-diagonal pair
    and, under max_violation, the lead of each row's / column's hardest negative over the runner-up (where that maximum is positive)."""
    S = np.asarray(score, np.float64)
    B = S.shape[0]
    dg = np.diag(S)
    off = ~np.eye(B, dtype=bool)
    slack = np.inf
    for name, ref, axis in (('i2t', dg[:, None], 1), ('t2i', dg[None, :], 0)):
        if direction not in (name, 'bidir') or B < 2:
            continue
        arg = margin + S - ref
        slack = min(slack, np.abs(arg[off]).min())
        if max_violation and B > 2:
            cost = np.maximum(arg, 0.0) * off
            top = np.sort(np.where(off, cost, -np.inf), axis=axis)
            first, second = (top[:, -1], top[:, -2]) if axis == 1 else (top[-1, :], top[-2, :])
            lead = (first - second)[first > 0.0]
            if lead.size:
                slack = min(slack, lead.min())
    return slack


def margin_eps(B, d):
    """The relative fp32 rounding of laff_margin_loss's gradient chain on its all-absolute-values majorant (see margin)."""
    return (3 * B + 3 * d + 24) * 2.0 ** -24


def margin(s, im, margin, max_violation, cost_style, direction):
    """(loss, d_s, d_im, b_s, b_im) in float64 for s, im (B, d) or (B, H, d): the margin ranking loss per head, summed.

    b_s and b_im bound, element by element, what fp32 rounding can do to d_s and d_im when the same chain (normalise, scores, hinge
    weights, two products, backward of the normalisation) runs in fp32 and takes every decision as float64 does.  They are the chain
    itself with every term replaced by its absolute value, so nothing cancels, times a relative error eps:

        G_abs = |dS| . |s^|   (resp. |dS|^T . |im^|),   o_abs = G_abs / (r + EPS) + |x^| sum_k(|x^_k| G_abs_k) / r,   b = eps o_abs
        eps   = (3 B + 3 d + 24) u,   u = 2^-24

    eps is first order in u and holds for any summation order (a sum of n terms of one sign, or measured against the sum of the
    absolute values of its terms, is off by at most n u relative, however it is bracketed):
      * x^ = x / (|x| + eps') carries (d/2 + 4) u: the sum of d squares d u on |x|^2, halved by the sqrt, plus the squares' own
        rounding, the sqrt, the add and the divide.
      * an off-diagonal dS entry is the weight w = fl(1 / count) once or twice (added exactly): at most 3 u with the conversion of
        the count; the diagonal is up to 2 (B - 1) additions of -w, all of one sign: at most (2 B + 2) u.
      * a product over K = B terms adds (B + 1) u relative to sum |dS| |x^|, so G carries (2B + 2) + (d/2 + 4) + (B + 1) u at most
        on G_abs: (3 B + d/2 + 7) u.
      * the backward, o = G / n - x^ (x^ . G) / r.  First term: G's error, n's (d/2 + 2) u and the divide: (3 B + d + 10) u.  Second
        term: the d-term dot product adds (d + 1) u and x^'s (d/2 + 4) u to G's: (3 B + 2 d + 12) u; the division by r (r carries
        (d/2 + 2) u) and the product with x^ ((d/2 + 4) u) with their own roundings add (d + 8) u: (3 B + 3 d + 20) u.  The
        subtraction adds one u on at most o_abs.
    Together at most (3 B + 3 d + 21) u on o_abs; eps rounds that up to (3 B + 3 d + 24) u, which leaves room for the second order.
    """
    s = np.asarray(s, np.float64)
    im = np.asarray(im, np.float64)
    flat = s.ndim == 2
    if flat:
        s, im = s[:, None, :], im[:, None, :]
    B, H, d = s.shape
    eps = margin_eps(B, d)
    loss = 0.0
    d_s, d_im, b_s, b_im = (np.zeros_like(s) for _ in range(4))

    def bound(xh, r, G_abs):
        return eps * (G_abs / (r + EPS) + np.abs(xh) * (np.abs(xh) * G_abs).sum(axis=1, keepdims=True) / r)

    for h in range(H):
        sh, rs = _l2norm(s[:, h])
        ih, ri = _l2norm(im[:, h])
        l, dS = margin_scores(ih @ sh.T, margin, max_violation, cost_style, direction)
        loss += l
        d_im[:, h] = _l2norm_bwd(ih, ri, dS @ sh)
        d_s[:, h] = _l2norm_bwd(sh, rs, dS.T @ ih)
        b_im[:, h] = bound(ih, ri, np.abs(dS) @ np.abs(sh))
        b_s[:, h] = bound(sh, rs, np.abs(dS).T @ np.abs(ih))
    out = (d_s, d_im, b_s, b_im)
    return (loss,) + (tuple(a[:, 0] for a in out) if flat else out)
