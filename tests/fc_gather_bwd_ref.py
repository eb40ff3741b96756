"""The backward of the FC projection a = act(x W^T + bias) of a SPARSE x, restated in float64.

The pattern is densified -- an entry that is named twice adds up, an id outside [0, Dk) or a row outside [0, N) is dropped -- and the
formulas and bounds are those of tests/fc_bwd_ref.py:

    dz = da * act'(a)        dw = dz^T x   [D, Dk]        db = sum_n dz[n, :]   [D]        (no dx: counts are not differentiable)
    |dw - ref| <= (N + 4) u |da|^T |x|        |db - ref| <= (N + 4) u sum_n |da|,    u = 2^-24

|x| adds the magnitudes of the entries one by one (equal to |x| for counts, which are positive).  A column's sum has as many terms as
the column has entries: the factor N + 4 covers every column of at most N entries, repeated ones counted.
"""
import numpy as np
import torch

import fc_bwd_ref as R

U = R.U
ACTIVATIONS = R.ACTIVATIONS


def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=dtype)


def dense_from_csr(crow, col, val, N, Dk, magnitude=False):
    """The (N, Dk) float64 matrix of a CSR pattern: repeated entries added, ids outside [0, Dk) dropped.  val None: all ones."""
    crow, col = _np(crow, np.int64), _np(col, np.int64)
    val = np.ones(col.shape[0]) if val is None else _np(val, np.float64)
    x = np.zeros((N, Dk))
    row = np.repeat(np.arange(N), np.diff(crow))
    keep = (col >= 0) & (col < Dk)
    np.add.at(x, (row[keep], col[keep]), np.abs(val[keep]) if magnitude else val[keep])
    return x


def dense_from_csc(colptr, rows, val, N, Dk, magnitude=False):
    """The same matrix from the transposed pattern as laff_fc_gather_backward reads it: column v owns [colptr[v], colptr[v + 1]);
    entries outside every column's range, and rows outside [0, N), are dropped."""
    colptr, rows = _np(colptr, np.int64), _np(rows, np.int64)
    val = np.ones(rows.shape[0]) if val is None else _np(val, np.float64)
    x = np.zeros((N, Dk))
    for v in range(Dk):
        for j in range(colptr[v], colptr[v + 1]):
            if 0 <= rows[j] < N:
                x[rows[j], v] += abs(val[j]) if magnitude else val[j]
    return x


def transpose_plain(crow, col, val, N, Dk):
    """A plain transposition of a CSR pattern, entry by entry: per column the (row, value) pairs in the order the CSR holds them."""
    crow, col = _np(crow, np.int64), _np(col, np.int64)
    val = np.ones(col.shape[0], np.float32) if val is None else _np(val, np.float32)
    cols = [[] for _ in range(Dk)]
    for n in range(N):
        for j in range(crow[n], crow[n + 1]):
            if 0 <= col[j] < Dk:
                cols[col[j]].append((n, val[j]))
    return cols


def backward(x_dense, a, da, activation):
    """(dw, db) in float64 from the densified x (N, Dk), the forward output a (N, D) and its gradient da: fc_bwd_ref's formulas."""
    dz = _np(da, np.float64) * R.act_prime(a, activation)
    return dz.T @ x_dense, dz.sum(0)


def bounds(x_magnitude, da):
    """The element-by-element bounds (for dw, db) of the module docstring; x_magnitude is the densified pattern with magnitude=True."""
    da = np.abs(_np(da, np.float64))
    N = da.shape[0]
    return (N + 4) * U * (da.T @ x_magnitude), (N + 4) * U * da.sum(0)


def column(colptr, rows, val, v, a, da, activation):
    """Column v of dw and of its bound ([D] each) straight from the transposed pattern: for shapes too large to densify."""
    N = a.shape[0]
    lo, hi = int(colptr[v]), int(colptr[v + 1])
    rs = _np(rows[lo:hi], np.int64)
    xs = np.ones(hi - lo) if val is None else _np(val[lo:hi], np.float64)
    keep = (rs >= 0) & (rs < N)
    rs, xs = rs[keep], xs[keep]
    dz = _np(da[rs], np.float64) * R.act_prime(a[rs], activation)
    return xs @ dz, (N + 4) * U * (np.abs(xs) @ np.abs(_np(da[rs], np.float64)))
