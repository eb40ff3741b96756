"""A float64 torch restatement of what the fuse kernels (laff_amd/csrc/fuse.hip) compute from their fp32 inputs: the planes of
laff_fuse (dense / tiled / deferred activation / folded affine / gather CSR / row norm), the attention fusion over them
(Multi_head_MyApply_Attention, model/Attention.py:508-531, over Attention_1, :78-105; JustAverage, :35-37) and the per-video frame
attention of laff_frame_fuse (model/model.py:2163-2173).  The checker of tests/test_fuse_ref.py (CPU, against the fp32 oracle and the
goldens) and tests/test_gpu_fuse_routes.py (on the device).  Every function takes numpy arrays or tensors and works on their device."""
import numpy as np
import torch

F64 = torch.float64
NORM_EPS = 1e-13 + 1e-14          # loss.l2norm: |x| + eps + 1e-14 (per-head l2norm, the row norm of the expert branch)
OUT_EPS = 1e-14                   # Attention_1's final l2norm(eps=0): |g| + 1e-14


def _t(a, device=None):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(F64) if device is None else a.to(device=device, dtype=F64)
    return torch.as_tensor(np.asarray(a), dtype=F64, device=device)


def activation(y, act):
    if act is None:
        return y
    if act == 'tanh':
        return torch.tanh(y)
    if act == 'relu':
        return torch.clamp(y, min=0.0)
    if act == 'sigmoid':
        return torch.sigmoid(y)
    raise ValueError(act)


def dense_plane(x, H, d, tile=False, split_head=True, scale=None, shift=None, act=None):
    """x: (N, H * d) (split heads), (N, d) (tiled over the heads, or one row shared by every head without split heads)
    -> (N, H, d) float64: activation, then the folded affine (scale / shift over the H * d stacked columns, d without split heads)."""
    x = _t(x)
    N = x.shape[0]
    if tile or not split_head:
        y = activation(x[:, :d], act)[:, None, :].expand(N, H, d)
    else:
        y = activation(x[:, :H * d], act).reshape(N, H, d)
    if scale is not None:
        shp = (1, 1, d) if not split_head else (1, H, d)
        y = y * _t(scale, y.device).reshape(shp) + _t(shift, y.device).reshape(shp)
    return y.contiguous()


def gather_plane(indptr, indices, values, wt, H, d, bias=None, scale=None, shift=None, act=None):
    """A sparse feature through its FC: row n is sum_p values[p] * wt[indices[p]] over indptr[n] <= p < indptr[n + 1] (ids outside
    [0, wt rows) dropped; values None reads as ones), plus bias, then activation and folded affine -> (N, H, d) float64."""
    wt = _t(wt)
    dev = wt.device
    indptr = torch.as_tensor(np.asarray(indptr.cpu() if isinstance(indptr, torch.Tensor) else indptr), dtype=torch.long, device=dev)
    idx = torch.as_tensor(np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices), dtype=torch.long, device=dev)
    N, Dk = indptr.numel() - 1, wt.shape[0]
    val = torch.ones(idx.numel(), dtype=F64, device=dev) if values is None else _t(values, dev).reshape(-1)
    row = torch.repeat_interleave(torch.arange(N, device=dev), indptr[1:] - indptr[:-1])
    keep = (idx >= 0) & (idx < Dk)
    y = torch.zeros((N, H * d), dtype=F64, device=dev)
    y.index_add_(0, row[keep], wt[idx[keep], :H * d] * val[keep, None])
    if bias is not None:
        y = y + _t(bias, dev)[:H * d]
    y = activation(y, act)
    if scale is not None:
        y = y * _t(scale, dev)[:H * d] + _t(shift, dev)[:H * d]
    return y.reshape(N, H, d)


def row_scale(plane, split_head=True):
    """l2norm(local_embs, dim=2) of the expert branch as laff_plane_row_norms computes it: 1 / (|row| + 1e-13 + 1e-14) over the
    stacked row of the plane (H * d columns, or the d shared ones without split heads) -> (N, 1, 1)."""
    rows = plane.reshape(plane.shape[0], -1) if split_head else plane[:, 0, :]
    return (1.0 / (rows.pow(2).sum(1).sqrt() + NORM_EPS))[:, None, None]


def _heads(X, l2norm_each_head):
    X = _t(X)
    return X / (X.pow(2).sum(3, keepdim=True).sqrt() + NORM_EPS) if l2norm_each_head else X


def logits(X, w, b, mul=False, l2norm_each_head=False):
    """The (N, H, L) softmax inputs of attention(): (x_l [* mean_l x]) . w_h + b_h."""
    X = _heads(X, l2norm_each_head)
    N, L, H, d = X.shape
    c = X * (X.sum(1) / L)[:, None] if mul else X
    return torch.einsum('nlhd,hd->nhl', c, _t(w, X.device).reshape(H, d)) + _t(b, X.device).reshape(H)[None, :, None]


def attention(X, w=None, b=None, gw=None, with_ave=False, mul=False, l2norm_each_head=False, just_average=False):
    """X: (N, L, H, d) float64 planes -> (E (N, H, d), softmax weights (N, H, L) or None).
    Per head: optional l2norm of every plane, logits (x_l [* mean_l x]) . w_h + b_h, softmax, sum_l a_l x_l + gw_h sum_l x_l
    (Attention_1 adds gw * mean to each of the L terms), then |.| + 1e-14.  JUST_AVERAGE: the plain mean over the planes."""
    X = _heads(X, l2norm_each_head)
    N, L, H, d = X.shape
    s = X.sum(1)                                                       # (N, H, d)
    if just_average:
        return s / L, None
    a = torch.softmax(logits(X, w, b, mul), dim=2)
    g = torch.einsum('nhl,nlhd->nhd', a, X)
    if with_ave:
        g = g + _t(gw, X.device).reshape(1, H, 1) * s
    return g / (g.pow(2).sum(2, keepdim=True).sqrt() + OUT_EPS), a


def frame_lengths(B, Fmax, lens=None, mask=None):
    """The frames every video folds in: round(sum of its mask row) or lens, clamped to [0, Fmax]; all Fmax without either."""
    if mask is not None:
        return torch.clamp(torch.round(_t(mask)[:, :Fmax].sum(1)).long(), 0, Fmax)
    if lens is not None:
        ln = lens if isinstance(lens, torch.Tensor) else torch.as_tensor(np.asarray(lens))
        return torch.clamp(ln.long(), 0, Fmax)
    return torch.full((B,), Fmax, dtype=torch.long)


def frame_attention(frames, w, b, gw=None, with_ave=False, mul=False, lens=None, mask=None):
    """frames (B, Fmax, d) -> (B, d) float64.  Frames at or past a video's length count as zeros whatever the buffer holds: their
    logit is b, they add nothing to the sums.  mul: w * (sum of the frames / Fmax), padding included in the mean."""
    x = _t(frames)
    B, Fmax, d = x.shape
    n = frame_lengths(B, Fmax, lens, mask).to(x.device)
    x = x * (torch.arange(Fmax, device=x.device)[None, :] < n[:, None])[:, :, None]
    w = _t(w, x.device).reshape(1, 1, d)
    s = x.sum(1)                                                       # (B, d)
    c = x * (s / Fmax)[:, None, :] if mul else x
    a = torch.softmax((c * w).sum(2) + float(_t(b).reshape(-1)[0]), dim=1)
    g = torch.einsum('bf,bfd->bd', a, x)
    if with_ave:
        g = g + float(_t(gw).reshape(-1)[0]) * s
    return g / (g.pow(2).sum(1, keepdim=True).sqrt() + OUT_EPS)
