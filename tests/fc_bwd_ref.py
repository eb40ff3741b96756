"""The backward of the FC projection a = act(x W^T + bias), written out by hand in float64.

The saved forward output `a` is an INPUT of the formulas, as it is of laff_fc_backward: act' is a function of a for every activation.

    dz = da * act'(a)        tanh: 1 - a^2     sigmoid: a (1 - a)     relu: a > 0     none: 1
    dx = dz W                [N, Dk]
    dw = dz^T x              [D, Dk]
    db = sum_n dz[n, :]      [D]

`bounds` gives the element-by-element error bounds of an fp32 evaluation in any summation order, fma or not:
    |dw - ref| <= (N + 4) u |da|^T |x|     |dx - ref| <= (D + 4) u |da| |W|     |db - ref| <= (N + 4) u sum_n |da|,    u = 2^-24
(a K-term fp32 dot product stays within gamma_K sum |a b|; forming dz from a costs at most three roundings against |act'| <= 1).
"""
import numpy as np
import torch

U = 2.0 ** -24
ACTIVATIONS = (None, 'tanh', 'sigmoid', 'relu')


def _f64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def act_prime(a, activation):
    a = _f64(a)
    if activation == 'tanh':
        return 1.0 - a * a
    if activation == 'sigmoid':
        return a * (1.0 - a)
    if activation == 'relu':
        return (a > 0).astype(np.float64)
    if activation in (None, 'none'):
        return np.ones_like(a)
    raise ValueError(activation)


def backward(x, w, a, da, activation):
    """(dx, dw, db) in float64 numpy from x (N, Dk), w (D, Dk), the forward output a (N, D) and its gradient da (N, D)."""
    x, w, da = _f64(x), _f64(w), _f64(da)
    dz = da * act_prime(a, activation)
    return dz @ w, dz.T @ x, dz.sum(0)


def bounds(x, w, da):
    """The element-by-element bounds (for dx, dw, db) of the module docstring."""
    x, w, da = np.abs(_f64(x)), np.abs(_f64(w)), np.abs(_f64(da))
    N, D = da.shape
    return (D + 4) * U * (da @ w), (N + 4) * U * (da.T @ x), (N + 4) * U * da.sum(0)


def forward_torch(x, w, b, activation):
    z = torch.nn.functional.linear(x, w, b)
    return {None: lambda t: t, 'none': lambda t: t, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}[activation](z)


def rel_err(got, ref):
    """max |got - ref| / max |ref|; a reference that is zero throughout admits only zeros."""
    got, ref = _f64(got).reshape(-1), _f64(ref).reshape(-1)
    if ref.size == 0:
        return 0.0
    top = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    if top == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / top
