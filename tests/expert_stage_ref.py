"""float64 restatement of the expert stage of the LAFF towers in numpy (laff_expert_stage_train and its backward):

    v = x_l[n, :] + expert[l, :]     s = |v|     r = 1 / (s + 1e-13 + 1e-14)     Y[n, l, :] = v r     (v without l2norm)
    dv = r g - v (r^2 / s) (v . g), the second term 0 where s == 0;  dv = g without l2norm;  dx_l = dv;  d_expert[l] = sum_n dv

and the absolute-value expressions the device tests' bounds are stated on.  Everything is evaluated in float64 whatever the inputs'
type is."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32
EPS = 1e-13 + 1e-14


def _v(xs, expert):
    v = np.stack([np.asarray(x, np.float64) for x in xs], axis=1)            # (N, L, D)
    return v if expert is None else v + np.asarray(expert, np.float64)[None]


def forward(xs, expert, l2norm):
    """(Y (N, L, D), r (L, N) or None)."""
    v = _v(xs, expert)
    if not l2norm:
        return v, None
    r = 1.0 / (np.sqrt((v * v).sum(2)) + EPS)
    return v * r[:, :, None], r.T.copy()


def backward(xs, expert, l2norm, dY):
    """(dx (N, L, D), d_expert (L, D), mag (N, L, D)): mag = r |g_i| + |v_i| (r^2 / s) sum_j |v_j g_j|, the all-absolute-values
    majorant of dv that the bounds scale (|g| without l2norm)."""
    v, g = _v(xs, expert), np.asarray(dY, np.float64)
    if not l2norm:
        return g.copy(), g.sum(0), np.abs(g)
    s = np.sqrt((v * v).sum(2))
    r = 1.0 / (s + EPS)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(s > 0, r * r / s, 0.0)
    dv = r[:, :, None] * g - v * (q * (v * g).sum(2))[:, :, None]
    mag = r[:, :, None] * np.abs(g) + np.abs(v) * (q * np.abs(v * g).sum(2))[:, :, None]
    return dv, dv.sum(0), mag


def bounds(N, D, l2norm, Y64, mag):
    """(bound of Y, of dx, of d_expert), element by element, from float64 values.  With l2norm: one rounding for v, at most (D + 2) u
    on the sum of squares, halved by the root, three more operations: (D / 2 + 5) u |Y|; dx within (3 D + 16) u mag; d_expert adds the
    N roundings of its sums.  Without: Y is one rounding from the float64 sum, dx is dY itself (bound 0), d_expert N u sum_n |g|."""
    if not l2norm:
        return U * np.abs(Y64), np.zeros_like(mag), N * U * mag.sum(0)
    return (D / 2 + 5) * U * np.abs(Y64), (3 * D + 16) * U * mag, (3 * D + 16 + N) * U * mag.sum(0)
