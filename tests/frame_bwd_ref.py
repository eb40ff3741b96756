"""A float64 restatement, written out by hand with no autograd, of what laff_frame_fuse_backward (laff_amd/csrc/frame_bwd.hip) computes:
the gradients of tests/fuse_ref.frame_attention with respect to the frames and w; b's gradient is zero, gw has
none.  Beside it, autograd_grads() takes the same gradients from torch.autograd through fuse_ref.frame_attention itself, in float64 or
float32: the checker of the closed form (tests/test_frame_bwd_ref.py) and of the kernel (tests/test_gpu_frame_fuse_backward.py).

frames (B, Fmax, d), dV (B, d), lens (B,) or None (every frame real).  Frames at or past a video's length are constants of the problem:
they are read as zeros whatever the buffer holds (NaN included) and their rows of the gradient are zeros.  A video of length 0 has
g = 0 and V = 0: float64 autograd gives NaN there, both functions below set its rows to zero and leave it out of dw.
"""
import numpy as np
import torch

import fuse_ref
from fuse_bwd_ref import rel_err  # noqa: F401  (the error measure of every backward check)

F64 = torch.float64
OUT_EPS = fuse_ref.OUT_EPS


def _t(a, dtype=F64):
    return a.detach().to('cpu', dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype)


def masked(frames, lens, dtype=F64):
    """(the frames with every row at or past its video's length replaced by zeros, the lengths clamped to [0, Fmax], the row mask)"""
    x = _t(frames, dtype)
    B, Fmax, _ = x.shape
    n = fuse_ref.frame_lengths(B, Fmax, None if lens is None else _t(lens, torch.long))
    keep = torch.arange(Fmax)[None, :] < n[:, None]
    return torch.where(keep[:, :, None], x, torch.zeros((), dtype=dtype)), n, keep


def closed_form(frames, w, b, gw, dV, with_ave=False, mul=False, lens=None):
    """{'dx': (B, Fmax, d), 'dw': (d,), 'db': (1,) zeros, 'g_norm': (B,) -- |g|, the length the backward divides by --, 'a': (B, Fmax)}"""
    x, n, keep = masked(frames, lens)
    B, Fmax, d = x.shape
    w, dV = _t(w).reshape(1, d), _t(dV).reshape(B, d)
    bias = float(_t(b).reshape(-1)[0])
    ave = float(_t(gw).reshape(-1)[0]) if with_ave else 0.0
    live = (n > 0)[:, None]
    s = x.sum(1)                                                       # (B, d)
    ws = w * s / Fmax if mul else w.expand(B, d)
    a = torch.softmax(torch.einsum('bfd,bd->bf', x, ws) + bias, dim=1)
    t = torch.einsum('bf,bfd->bd', a, x)
    g = t + ave * s
    r = g.pow(2).sum(1, keepdim=True).sqrt()
    rs = torch.where(live, r, torch.ones_like(r))                      # (a zero-length video: any divisor, its rows are cleared below)
    V = g / (rs + OUT_EPS)
    dg = (dV - V * (V * dV).sum(1, keepdim=True) * (rs + OUT_EPS) / rs) / (rs + OUT_EPS)
    dg = torch.where(live, dg, torch.zeros_like(dg))
    da = torch.einsum('bd,bfd->bf', dg, x)
    c = (a * da).sum(1, keepdim=True)
    dz = a * (da - c)
    q = torch.einsum('bf,bfd->bd', dz * keep, x)
    dx = (a + ave)[:, :, None] * dg[:, None, :] + dz[:, :, None] * ws[:, None, :]
    if mul:
        dx = dx + (w * q / Fmax)[:, None, :]
    dx = dx * keep[:, :, None]
    dw = (q * s / Fmax if mul else q).sum(0)
    return {'dx': dx, 'dw': dw, 'db': torch.zeros(1, dtype=F64), 'g_norm': r[:, 0], 'a': a}


def autograd_grads(frames, w, b, gw, dV, with_ave=False, mul=False, lens=None, dtype=F64):
    """(dx, dw, db) of sum(V * dV) from torch.autograd through fuse_ref.frame_attention, every operation in `dtype` on the CPU (results
    in float64).  fuse_ref converts its inputs to fuse_ref.F64; for a float32 run that name is pointed at float32 for the duration of
    the call.  The padded rows enter as zeros and leave with zero gradient; zero-length videos are left out of the graph.  db is zeros:
    the restatement reads b as a number, and the softmax does not see a shift of its logits."""
    x, n, keep = masked(frames, lens, dtype)
    B, Fmax, d = x.shape
    live = torch.nonzero(n > 0)[:, 0]
    dx = torch.zeros(B, Fmax, d, dtype=F64)
    if live.numel() == 0:
        return dx, torch.zeros(d, dtype=F64), torch.zeros(1, dtype=F64)
    xl = x[live].clone().requires_grad_(True)
    wt = _t(w, dtype).reshape(d).clone().requires_grad_(True)
    saved = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        with torch.enable_grad():
            V = fuse_ref.frame_attention(xl, wt, _t(b, dtype), None if gw is None else _t(gw, dtype), with_ave=with_ave, mul=mul,
                                         lens=n[live])
            assert V.dtype == dtype
            (V * _t(dV, dtype).reshape(B, d)[live]).sum().backward()
    finally:
        fuse_ref.F64 = saved
    dx[live] = xl.grad.to(F64) * keep[live][:, :, None]
    return dx, wt.grad.to(F64), torch.zeros(1, dtype=F64)
