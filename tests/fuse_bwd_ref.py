"""A float64 restatement, written out by hand with no autograd, of what laff_fuse_backward (laff_amd/csrc/fuse_bwd.hip) computes: the
gradients of tests/fuse_ref.attention over plain dense planes with respect to the planes, w and b.  Beside it,
autograd_grads() takes the same gradients from torch.autograd through fuse_ref.attention itself, in float64 or float32: the checker of
the closed forms (tests/test_fuse_bwd_ref.py) and of the kernel (tests/test_gpu_fuse_backward.py).

Planes are (N, L, H * d) with split heads (plane l holds x_l[n, h * d + c]) and (N, L, d) without (every head reads the same d columns,
and the gradient of a plane is the sum over the heads).  dE is (N, H, d).

Both normalisations y = v / (n + eps), n = |v|, have the backward dv = (dy - y (y . dy) (n + eps) / n) / (n + eps), as
tests/loss_ref._l2norm_bwd states it.
"""
import numpy as np
import torch

import fuse_ref

F64 = torch.float64
NORM_EPS, OUT_EPS = fuse_ref.NORM_EPS, fuse_ref.OUT_EPS


def _t(a, dtype=F64):
    return a.detach().to('cpu', dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype)


def heads_of(planes, H, d, split_head=True):
    """(N, L, H * d) / (N, L, d) -> the (N, L, H, d) input of fuse_ref.attention (a view: gradients flow back to the planes)."""
    N, L = planes.shape[:2]
    return planes.reshape(N, L, H, d) if split_head else planes[:, :, None, :].expand(N, L, H, d)


def closed_form(planes, H, d, w, b, gw, dE, with_ave=False, mul=False, l2norm_each_head=False, split_head=True, just_average=False):
    """{'dx': (N, L, H d | d), 'dw': (H, d), 'db': (H,), 'dz': (N, H, L), 'g_norm': (N, H), 'raw_norm': (N, L, H)} in float64.
    g_norm and raw_norm are the two lengths the backward divides by (|g|; |raw_l| under the per-head l2norm, else ones)."""
    P = _t(planes)
    N, L = P.shape[:2]
    raw = heads_of(P, H, d, split_head)
    dE = _t(dE).reshape(N, H, d)
    rho = raw.pow(2).sum(3, keepdim=True).sqrt()
    x = raw / (rho + NORM_EPS) if l2norm_each_head else raw
    if just_average:
        dx = (dE / L)[:, None].expand(N, L, H, d)
        dw, db, dz = torch.zeros(H, d, dtype=F64), torch.zeros(H, dtype=F64), torch.zeros(N, H, L, dtype=F64)
        gn = (x.sum(1) / L).pow(2).sum(2).sqrt()
    else:
        w, b = _t(w).reshape(H, d), _t(b).reshape(H)
        ave = _t(gw).reshape(1, H, 1) if with_ave else 0.0
        s = x.sum(1)                                                   # (N, H, d)
        ws = w[None] * s / L if mul else w[None].expand(N, H, d)       # the vector every x_l is dotted with
        a = torch.softmax(torch.einsum('nlhd,nhd->nhl', x, ws) + b[None, :, None], dim=2)
        g = torch.einsum('nhl,nlhd->nhd', a, x) + ave * s
        r = g.pow(2).sum(2, keepdim=True).sqrt()
        E = g / (r + OUT_EPS)
        dg = (dE - E * (E * dE).sum(2, keepdim=True) * (r + OUT_EPS) / r) / (r + OUT_EPS)
        da = torch.einsum('nhd,nlhd->nhl', dg, x)
        dz = a * (da - (a * da).sum(2, keepdim=True))
        q = torch.einsum('nhl,nlhd->nhd', dz, x)
        dx = torch.einsum('nhl,nhd->nlhd', a + ave, dg) + torch.einsum('nhl,nhd->nlhd', dz, ws)
        if mul:
            dx = dx + (w[None] * q / L)[:, None]
        dw = (q * s / L if mul else q).sum(0)
        db = dz.sum((0, 2))
        gn = r[:, :, 0]
    if l2norm_each_head:
        dx = (dx - x * (x * dx).sum(3, keepdim=True) * (rho + NORM_EPS) / rho) / (rho + NORM_EPS)
    dx = dx.reshape(N, L, H * d) if split_head else dx.sum(2)
    return {'dx': dx, 'dw': dw, 'db': db, 'dz': dz, 'g_norm': gn,
            'raw_norm': rho[..., 0] if l2norm_each_head else torch.ones(N, L, H, dtype=F64)}


def autograd_grads(planes, H, d, w, b, gw, dE, with_ave=False, mul=False, l2norm_each_head=False, split_head=True, just_average=False,
                   dtype=F64):
    """(dx, dw, db) of sum(E * dE) from torch.autograd through fuse_ref.attention, every operation in `dtype` on the CPU (results
    returned in float64).  fuse_ref converts its inputs to fuse_ref.F64; for a float32 run that name is pointed at float32 for the
    duration of the call.  just_average: dw and db are zeros."""
    P = _t(planes, dtype).requires_grad_(True)
    N = P.shape[0]
    wt = bt = None
    if not just_average:
        wt, bt = _t(w, dtype).reshape(H, d).requires_grad_(True), _t(b, dtype).reshape(H).requires_grad_(True)
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        with torch.enable_grad():
            E, _ = fuse_ref.attention(heads_of(P, H, d, split_head), wt, bt, None if gw is None else _t(gw, dtype), with_ave=with_ave,
                                      mul=mul, l2norm_each_head=l2norm_each_head, just_average=just_average)
            assert E.dtype == dtype
            (E * _t(dE, dtype).reshape(N, H, d)).sum().backward()
    finally:
        fuse_ref.F64 = keep
    if just_average:
        return P.grad.to(F64), torch.zeros(H, d, dtype=F64), torch.zeros(H, dtype=F64)
    return P.grad.to(F64), wt.grad.to(F64), bt.grad.to(F64)


def rel_err(got, ref):
    """max |got - ref| / max |ref| -- the error measure of the backward's checks.  A reference that is zero throughout (dw at L = 1:
    a softmax over one plane has no gradient) admits nothing but zeros: 0.0 then, inf otherwise."""
    got, ref = _t(got).reshape(-1), _t(ref).reshape(-1)
    if ref.numel() == 0:
        return 0.0
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if not bool(got.any()) else float('inf')
    return float((got - ref).abs().max()) / top
