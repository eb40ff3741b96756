"""Tensor-level wrappers over the C ABI (include/laff_hip.h).

torch is used here for device memory and streams only: every function takes CUDA (ROCm) fp32 tensors,
passes raw pointers to liblaff_hip.so on the current torch stream and returns torch tensors.  There is no
CPU or eager-PyTorch fallback: CPU tensors are rejected.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

from . import _lib
from ._lib import (ACT, GRU_POOLING, ATT_JUST_AVERAGE, ATT_L2NORM_EACH_HEAD, ATT_MUL, ATT_NO_SPLIT_HEAD, ATT_WITH_AVE, PREC,
                   FcProblem, FcSplitProblem, FcStripProblem, Plane, check, FcFusedProblem, RankSide, FcConcatProblem, FcConcatSegment,
                   FcLaunch, FcShape, RerankProblem)

__all__ = ['sim_hist', 'rerank_workspace_bytes', 'rerank_run', 'rerank_tkb', 'frame_preprocess', 'frame_desc_device', 'netvlad_workspace_bytes', 'netvlad_encode', 'netvlad_train_reserve_bytes', 'netvlad_backward_workspace_bytes', 'netvlad_encode_train', 'netvlad_backward', 'bert_workspace_bytes', 'bert_encode', 'clip_pack_weight', 'clip_workspace_bytes', 'clip_encode', 'gru_pack_whh', 'gru_workspace_bytes', 'gru_encode', 'gru_pack_whh_t', 'gru_gather_rows', 'batch_assemble', 'gru_train_reserve_bytes', 'gru_encode_train', 'gru_backward', 'gru_backward_plan', 'gru_backward_workspace_bytes', 'rank_resolve_metrics', 'rank_prepare', 'rank_prepare_text', 'rank_band_video', 'rank_export_pairs', 'rank_resolve_list', 'sim_gemm_banded', 'rank_resolve', 'exact_ranks', 'RankState', 'topk_rows', 'topk_from_operands', 'alloc_scores', 'frame_fuse_grouped', 'fc_act_bn_fused_grouped', 'fused_split_eligible', 'fc_strip_pack', 'fc_strip_eligible', 'fc_act_bn_strip_grouped', 'StripWeights', 'margin_loss', 'dsl_loss', 'margin_loss_scores', 'fc_gather_act_bn', 'fc_act_bn', 'fc_act_bn_grouped', 'fc_act_bn_split_grouped', 'split_rows', 'row_dot_gt', 'rank_metrics_async', 'fuse', 'fuse_backward', 'fc_backward', 'fc_backward_plan', 'csr_transpose', 'fc_gather_backward', 'fc_concat_backward', 'fc_concat_backward_plan', 'dropout_bn_train', 'dropout_bn_train_backward', 'tile_bn_train_plan', 'tile_bn_train', 'tile_bn_train_backward', 'expert_stage_train_plan', 'expert_stage_train', 'expert_stage_train_backward', 'dropout_bn_train_plan', 'optim_plan', 'optim_last_launches', 'grad_sqnorm', 'grad_scale', 'optim_step', 'frame_fuse', 'frame_fuse_backward', 'frame_fuse_backward_plan', 'pack_rows', 'sim_gemm', 'sim_gemm_route', 'SIM_ROUTES', 'fc_route', 'FC_ROUTES', 'FcRoute', 'gather_gt', 'rank_count', 'v2t_count', 'v2t_count_exact', 'reset_contexts', 'FusedPrepare', 'fused_prepare_eligible',
           'rank_metrics', 'attention_flags', 'PREC', 'default_prescale', 'selfattn_fuse', 'selfattn_fuse_backward',
           'selfattn_fuse_backward_plan', 'selfattn_mode', 'SELFATTN_OUTPUT_TYPES']

_ctx = {}
#: the library's LAFF_FC_STRIP_MFMA mode (process-wide; the library reads the variable whenever a context is created, and so does
#: _context, by the same rule: 32 selects the 32x32x16 kernels, anything else the 16x16x32 ones)
_fc_strip_mfma = 16

#: optional per-launch profiler (bench.py): object with begin(name) / end(name), called on the launching stream
profiler = None


def _call(name, fn, *args):
    if profiler is None:
        check(fn(*args))
    else:
        profiler.begin(name)
        check(fn(*args))
        rep = getattr(profiler, 'repeat', None)       # tools/energy_table.py: the launch issued n times in a row
        if rep is not None:
            for _ in range(rep(name) - 1):
                check(fn(*args))
        profiler.end(name)


def _atoi(text):
    """C's atoi: optional blanks and sign, leading digits, 0 when there are none."""
    m = re.match(r'\s*[+-]?\d+', text)
    return int(m.group(0)) if m else 0


def fc_strip_mfma(device):
    """The MFMA shape (16 or 32) of the strip-form FC kernels that the device's context packs for and launches."""
    _context(device)
    return _fc_strip_mfma


def _context(device):
    """One laff_ctx per device ordinal, re-bound to torch's current stream at every call."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    lib = _lib.load()
    if idx not in _ctx:
        h = C.c_void_p()
        check(lib.laff_ctx_create(idx, None, C.byref(h)))
        _ctx[idx] = h
        global _fc_strip_mfma
        _fc_strip_mfma = 32 if _atoi(os.environ.get('LAFF_FC_STRIP_MFMA', '16')) == 32 else 16
    h = _ctx[idx]
    check(lib.laff_ctx_set_stream(h, C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)))
    return lib, h


def stamp(slots, i):
    """laff_stamp: the device wall clock into slots[i] (int64 device tensor), ordered on the current stream, capturable."""
    lib, h = _context(slots.device)
    check(lib.laff_stamp(h, C.c_void_p(slots.data_ptr() + 8 * int(i))))


def wall_clock_khz(device):
    lib, h = _context(device)
    khz = C.c_int()
    check(lib.laff_wall_clock_khz(h, C.byref(khz)))
    return int(khz.value)


def reset_contexts():
    """Destroys the cached laff_ctx handles; the next call creates fresh ones (the LAFF_* environment knobs are read then)."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for k, h in list(_ctx.items()):
        if isinstance(k, int):                 # (other keys: per-context scratch kept alive for captured graphs)
            lib.laff_ctx_destroy(h)
    _ctx.clear()


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a CUDA (ROCm) tensor: laff_amd has no CPU path' % name)
    if t.dtype != dtype:
        raise TypeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    return t


def _rows(t, name):
    """2-D view with unit inner stride; returns (tensor, ld)."""
    _dev(t, name)
    if t.dim() != 2 or (t.numel() and t.stride(1) != 1):
        raise ValueError('%s must be 2-D with contiguous rows, got shape %s strides %s' % (name, tuple(t.shape), t.stride()))
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def _mat(t, name, align16=False):
    """A 2-D device fp32 operand of a training entry point as (tensor, pitch): a row view is read in place, anything else -- a non-unit
    inner stride, a pitch below the width (an expanded gradient) -- is made dense first.  align16: rows that are not 16-byte aligned
    (the base, or a pitch that is no multiple of 4 floats) are made dense too."""
    _dev(t, name)
    if t.dim() != 2:
        raise ValueError('%s must be 2-D, got shape %s' % (name, tuple(t.shape)))
    if t.numel() and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]) or
                      (align16 and (t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) % 4)))):
        t = t.contiguous()
    return _rows(t, name)


def _vec(t, D, name):
    """A contiguous device fp32 vector of D."""
    _dev(t, name)
    if tuple(t.shape) != (D,) or not t.is_contiguous():
        raise ValueError('%s must be a contiguous vector of %d, got shape %s' % (name, D, tuple(t.shape)))
    return t


def _vec_out(t, D, device, name):
    """A (D,) fp32 output: the caller's buffer through _vec, or a new one on `device`."""
    return torch.empty((D,), device=device, dtype=torch.float32) if t is None else _vec(t, D, name)


def _workspace(nbytes, device, floor=0):
    """A uint8 device workspace of max(nbytes, floor) bytes; None when that is zero."""
    if nbytes < floor:
        nbytes = floor
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def _csr_triple(x_csr):
    """(crow_indices int32, col_indices int32, values fp32) of a torch.sparse_csr matrix, contiguous, as the kernels read them."""
    return (x_csr.crow_indices().to(torch.int32).contiguous(), x_csr.col_indices().to(torch.int32).contiguous(),
            x_csr.values().to(torch.float32).contiguous())


def _csc_triple(csc, where='', Dk=None):
    """(colptr, rows, values, nnz) of a transposed pattern as csr_transpose returns it, checked: colptr and rows contiguous int32 device
    vectors (colptr of Dk + 1 entries where Dk is given), values None (all ones) or a contiguous fp32 device vector of nnz.  where:
    a prefix of the error texts ('segment %d: ')."""
    colptr, rows, values = csc
    for t, nm in ((colptr, 'colptr'), (rows, 'rows')):
        _dev(t, nm, torch.int32)
        if t.dim() != 1 or not t.is_contiguous():
            raise ValueError('%s%s must be a contiguous vector' % (where, nm))
    nnz = rows.numel()
    if Dk is not None and colptr.numel() != Dk + 1:
        raise ValueError('%scolptr has %d entries, expected Dk + 1 = %d' % (where, colptr.numel(), Dk + 1))
    if values is not None and (_dev(values, 'values').dim() != 1 or values.numel() != nnz or not values.is_contiguous()):
        raise ValueError('%svalues must be a contiguous vector of %d' % (where, nnz))
    return colptr, rows, values, nnz


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _size_query(symbol_name, *ints):
    """A laff_*_workspace_bytes style query: symbol(ints..., size_t* out) -> out."""
    n = C.c_size_t()
    check(getattr(_lib.load(), symbol_name)(*[int(i) for i in ints], C.byref(n)))
    return n.value


def _plan_query(symbol_name, n, *ints):
    """A laff_*_plan style query: symbol(ints..., int out[n]) -> out as a tuple."""
    out = (C.c_int * n)()
    check(getattr(_lib.load(), symbol_name)(*[int(i) for i in ints], out))
    return tuple(out)


def _offsets(off, off_host, name):
    """The offsets of a ragged batch (laff_amd/ragged.py): off [N+1] int32 on the device and off_host, the same on the host.
    Returns (off, off_host as a contiguous int32 array, N)."""
    off = _dev(off, name, torch.int32)
    if off.dim() != 1 or not off.is_contiguous():
        raise ValueError('%s must be a contiguous vector' % name)
    N = off.numel() - 1
    host = np.ascontiguousarray(off_host, dtype=np.int32)
    if host.shape != (N + 1,):
        raise ValueError('%s_host has %d entries, %s %d' % (name, host.size, name, N + 1))
    return off, host, N


def _out_rows(out, shape, device, name='out'):
    """An fp32 output of `shape` with a row pitch, allocated here when None: (out, its pointer, its pitch)."""
    if out is None:
        out = torch.empty(shape, device=device, dtype=torch.float32)
    if tuple(out.shape) != tuple(shape):
        raise ValueError('%s must be (%d, %d), got %s' % (name, shape[0], shape[1], tuple(out.shape)))
    o, ld = _rows(out, name)
    return out, _ptr(o), ld


def _ws_out(workspace, nbytes, out, shape, device):
    """A ragged entry point's workspace (allocated here from nbytes(), 16 bytes at least, when None) and its out through _out_rows:
    (workspace, out, out's pointer, out's pitch).  Allocates nothing when both are given."""
    if workspace is None:
        workspace = torch.empty(max(nbytes(), 16), dtype=torch.uint8, device=device)
    return (workspace,) + _out_rows(out, shape, device)


def alloc_scores(Nt, Nv, device):
    """(Nt, Nv) fp32 score matrix whose rows start on 128-byte lines (row pitch = Nv rounded up to 32 floats; a view when Nv is not
    a multiple of 32): the GEMM stores whole lines, which the memory system takes ~25 % faster than rows that straddle them
    (40000 x 10000: 0.496 -> 0.480 ms).  Every kernel of the library takes the row pitch (lds / ldo)."""
    pitch = (Nv + 31) & ~31
    if pitch == Nv or Nv < 1024:
        return torch.empty((Nt, Nv), device=device, dtype=torch.float32)
    return torch.empty((Nt, pitch), device=device, dtype=torch.float32)[:, :Nv]


def attention_flags(with_ave=False, mul=False, l2norm_each_head=False, split_head=True, just_average=False):
    return ((ATT_WITH_AVE if with_ave else 0) | (ATT_MUL if mul else 0) |
            (ATT_L2NORM_EACH_HEAD if l2norm_each_head else 0) | (0 if split_head else ATT_NO_SPLIT_HEAD) |
            (ATT_JUST_AVERAGE if just_average else 0))


def _fc_vectors(q, D):
    """An FC problem's bias / bn_scale / bn_shift as data pointers (None where absent), each checked to be a contiguous device
    vector of D."""
    ptrs = []
    for nm in ('bias', 'bn_scale', 'bn_shift'):
        t = q.get(nm)
        if t is not None:
            _dev(t, nm)
            if t.numel() != D or not t.is_contiguous():
                raise ValueError('%s must be a contiguous vector of %d' % (nm, D))
        ptrs.append(t.data_ptr() if t is not None else None)
    return ptrs


def _fc_epilogue(q, N, D, device):
    """(_fc_vectors(q, D), out, ldy): out is q['out'] or a new (N, D) fp32 matrix on `device`."""
    ptrs = _fc_vectors(q, D)
    out = q.get('out')
    if out is None:
        out = torch.empty((N, D), device=device, dtype=torch.float32)
    return ptrs, out, _rows(out, 'out')[1]


def fc_act_bn(x, weight, bias=None, bn_scale=None, bn_shift=None, activation=None, out=None):
    """Y = act(x @ weight.T + bias) * bn_scale + bn_shift   (TransformNet.forward, eval mode)."""
    return fc_act_bn_grouped([dict(x=x, weight=weight, bias=bias, bn_scale=bn_scale, bn_shift=bn_shift, activation=activation,
                                   out=out)])[0]


def fc_act_bn_grouped(problems):
    """Several independent projections in one launch.  problems: list of dicts with keys x, weight and optional
    bias, bn_scale, bn_shift, activation, out.  Returns the list of outputs."""
    if not problems:
        return []
    arr = (FcProblem * len(problems))()
    outs = []
    for i, q in enumerate(problems):
        x, ldx = _rows(q['x'], 'x')
        w, ldw = _rows(q['weight'], 'weight')
        N, Dk = x.shape
        D = w.shape[0]
        if w.shape[1] != Dk:
            raise ValueError('problem %d: weight is %s but x has %d columns' % (i, tuple(w.shape), Dk))
        vecs, out, ldy = _fc_epilogue(q, N, D, x.device)
        arr[i] = FcProblem(x.data_ptr(), N, Dk, ldx, w.data_ptr(), ldw, *vecs, D, ACT[q.get('activation')], out.data_ptr(), ldy)
        outs.append(out)
    lib, h = _context(problems[0]['x'].device)
    _call('fc_act_bn', lib.laff_fc_act_bn_grouped, h, arr, len(problems))
    return outs


def fc_gather_act_bn(x_csr, weight_t, bias=None, bn_scale=None, bn_shift=None, activation=None):
    """TransformNet on a sparse (torch CSR) feature matrix: gather-sum of rows of weight_t = W^T [Dk, D]."""
    if x_csr.layout != torch.sparse_csr or not x_csr.is_cuda:
        raise RuntimeError('x_csr must be a CUDA torch.sparse_csr tensor')
    N, Dk = x_csr.shape
    wt, ldwt = _rows(weight_t, 'weight_t')
    if wt.shape[0] != Dk:
        raise ValueError('weight_t is %s but x has %d columns' % (tuple(wt.shape), Dk))
    D = wt.shape[1]
    crow, col, val = _csr_triple(x_csr)
    for t, nm in ((bias, 'bias'), (bn_scale, 'bn_scale'), (bn_shift, 'bn_shift')):
        if t is not None:
            _dev(t, nm)
    out = torch.empty((N, D), device=wt.device, dtype=torch.float32)
    lib, h = _context(wt.device)
    _call('fc_gather', lib.laff_fc_gather_act_bn, h, _ptr(crow), _ptr(col), _ptr(val), N, Dk, _ptr(wt), ldwt, _ptr(bias),
          _ptr(bn_scale), _ptr(bn_shift), D, ACT[activation], _ptr(out), D)
    return out


def fc_concat_act_bn(segments, weight, bias=None, bn_scale=None, bn_shift=None, activation=None, out=None, weight_t=None):
    """Y = act(cat(segments, dim 1) @ weight.T + bias) * bn_scale + bn_shift without forming the concatenation (the W2VV++ towers)."""
    return fc_concat_act_bn_grouped([dict(segments=segments, weight=weight, bias=bias, bn_scale=bn_scale, bn_shift=bn_shift,
                                          activation=activation, out=out, weight_t=weight_t)])[0]


def fc_concat_act_bn_grouped(problems):
    """Several concat projections (both towers of a retrieval) in one launch.  problems: dicts with
        segments  list of 2-D fp32 CUDA matrices (contiguous rows, any row stride) and / or torch.sparse_csr matrices, all of N rows,
                  in the order their columns have in `weight`
        weight    (D, sum of the segment widths) fp32, read in place
        weight_t  optional {segment index: (width, ld >= D) transposed column block} for the sparse segments; a missing one is
                  made here (callers that keep the model cache it)
      and optional bias, bn_scale, bn_shift, activation, out.  fp32 arithmetic whatever FC_PRECISION says.  Returns the outputs."""
    if not problems:
        return []
    arr = (FcConcatProblem * len(problems))()
    outs, keep = [], []
    dev = None
    for i, q in enumerate(problems):
        segs = list(q['segments'])
        w, ldw = _rows(q['weight'], 'weight')
        D, K = w.shape
        dev = w.device
        if not segs:
            raise ValueError('problem %d: no segments' % i)
        N = segs[0].shape[0]
        sarr = (FcConcatSegment * len(segs))()
        col = 0
        for j, x in enumerate(segs):
            if x.dim() != 2 or x.shape[0] != N:
                raise ValueError('problem %d: segment %d is %s, expected %d rows' % (i, j, tuple(x.shape), N))
            Dk = x.shape[1]
            if x.layout == torch.sparse_csr:
                if not x.is_cuda:
                    raise RuntimeError('problem %d: segment %d must be a CUDA torch.sparse_csr tensor' % (i, j))
                wt = (q.get('weight_t') or {}).get(j)
                if wt is None:
                    wt = w[:, col:col + Dk].t().contiguous()
                wt, ldwt = _rows(wt, 'weight_t')
                if wt.shape[0] != Dk or wt.shape[1] != D:
                    raise ValueError('problem %d: weight_t of segment %d is %s, expected (%d, %d)' % (i, j, tuple(wt.shape), Dk, D))
                crow, cidx, val = _csr_triple(x)
                keep += [wt, crow, cidx, val]
                sarr[j] = FcConcatSegment(None, 0, crow.data_ptr(), cidx.data_ptr(), val.data_ptr(), wt.data_ptr(), ldwt, Dk, col)
            else:
                x, ldx = _rows(x, 'segment')
                sarr[j] = FcConcatSegment(x.data_ptr(), ldx, None, None, None, None, 0, Dk, col)
            col += Dk
        if col != K:
            raise ValueError('problem %d: weight is %s but the segments have %d columns' % (i, tuple(w.shape), col))
        vecs, out, ldy = _fc_epilogue(q, N, D, dev)
        if tuple(out.shape) != (N, D):
            raise ValueError('problem %d: out is %s, expected (%d, %d)' % (i, tuple(out.shape), N, D))
        arr[i] = FcConcatProblem(sarr, len(segs), N, w.data_ptr(), K, ldw, *vecs, D, ACT[q.get('activation')], out.data_ptr(), ldy)
        keep.append(sarr)
        outs.append(out)
    lib, h = _context(dev)
    _call('fc_concat', lib.laff_fc_concat_act_bn_grouped, h, arr, len(problems))
    return outs


LOSS_FLAGS = {k: _lib.K['LAFF_LOSS_' + c] for k, c in (('max_violation', 'MAX_VIOLATION'), ('mean', 'COST_MEAN'), ('i2t', 'DIR_I2T'), ('t2i', 'DIR_T2I'))}


def margin_loss(s, im, margin, max_violation=True, cost_style='sum', direction='t2i', want_grad=True):
    """MarginRankingLoss over heads (laff_margin_loss).  s, im: (B, d) or (B, H, d) fp32 CUDA tensors.
    Returns (loss 0-d tensor, d_s, d_im) -- the gradients are None when want_grad is False."""
    if s.shape != im.shape or s.dim() not in (2, 3):
        raise ValueError('s and im must both be (B, d) or (B, H, d); got %s and %s' % (tuple(s.shape), tuple(im.shape)))
    if direction not in ('i2t', 't2i', 'bidir'):
        raise ValueError("direction must be 'i2t', 't2i' or 'bidir'")
    if cost_style not in ('sum', 'mean'):
        raise ValueError("cost_style must be 'sum' or 'mean'")
    s_c = _dev(s.contiguous(), 's')
    im_c = _dev(im.contiguous(), 'im')
    B, H, d = (s.shape[0], 1, s.shape[1]) if s.dim() == 2 else s.shape
    flags = (LOSS_FLAGS['max_violation'] if max_violation else 0) | (LOSS_FLAGS['mean'] if cost_style == 'mean' else 0)
    flags |= {'i2t': LOSS_FLAGS['i2t'], 't2i': LOSS_FLAGS['t2i'], 'bidir': LOSS_FLAGS['i2t'] | LOSS_FLAGS['t2i']}[direction]
    lib, h = _context(s_c.device)
    nbytes = C.c_size_t()
    rc = lib.laff_margin_loss_workspace_bytes(B, H, d, C.byref(nbytes))
    if rc:
        raise RuntimeError(lib.laff_last_error().decode())
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=s_c.device)
    loss = torch.empty((), dtype=torch.float32, device=s_c.device)
    d_s = torch.empty_like(s_c) if want_grad else None
    d_im = torch.empty_like(im_c) if want_grad else None
    _call('margin_loss', lib.laff_margin_loss, h, _ptr(s_c), _ptr(im_c), B, H, d, float(margin), flags, _ptr(loss), _ptr(d_s),
          _ptr(d_im), _ptr(ws), nbytes.value)
    return loss, d_s, d_im


def dsl_loss(s, im, temp=1000, want_grad=True):
    """DualSoftmaxLoss over heads (laff_dsl_loss).  s, im: (B, d) or (B, H, d) fp32 CUDA tensors.
    Returns (loss 0-d tensor, d_s, d_im) -- the gradients are None, and no gradient buffer is allocated, when want_grad is False."""
    if s.shape != im.shape or s.dim() not in (2, 3):
        raise ValueError('s and im must both be (B, d) or (B, H, d); got %s and %s' % (tuple(s.shape), tuple(im.shape)))
    if not temp > 0:
        raise ValueError('temp must be positive, got %r' % (temp,))
    s_c = _dev(s.contiguous(), 's')
    im_c = _dev(im.contiguous(), 'im')
    if im_c.device != s_c.device:
        raise ValueError('s and im must be on one device, got %s and %s' % (s_c.device, im_c.device))
    B, H, d = (s.shape[0], 1, s.shape[1]) if s.dim() == 2 else s.shape
    lib, h = _context(s_c.device)
    nbytes = _size_query('laff_dsl_loss_workspace_bytes', B, H, d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s_c.device)
    loss = (torch.empty if B else torch.zeros)((), dtype=torch.float32, device=s_c.device)     # an empty batch sums to 0
    d_s = torch.empty_like(s_c) if want_grad else None
    d_im = torch.empty_like(im_c) if want_grad else None
    _call('dsl_loss', lib.laff_dsl_loss, h, _ptr(s_c), _ptr(im_c), B, H, d, float(temp), _ptr(loss), _ptr(d_s), _ptr(d_im), _ptr(ws),
          nbytes)
    return loss, d_s, d_im


def margin_loss_scores(score, margin, max_violation=True, cost_style='sum', direction='t2i', want_grad=True):
    """MarginRankingLossWithScore (laff_margin_loss_scores) on score (B, B), an fp32 CUDA matrix with any row stride.
    Returns (loss 0-d tensor, d_score (B, B)) -- d_score is None when want_grad is False."""
    if score.dim() != 2 or score.shape[0] != score.shape[1]:
        raise ValueError('score must be (B, B); got %s' % (tuple(score.shape),))
    if direction not in ('i2t', 't2i', 'bidir'):
        raise ValueError("direction must be 'i2t', 't2i' or 'bidir'")
    if cost_style not in ('sum', 'mean'):
        raise ValueError("cost_style must be 'sum' or 'mean'")
    _dev(score, 'score')
    if score.numel() and score.stride(1) != 1:
        score = score.contiguous()
    score, ld = _rows(score, 'score')
    B = score.shape[0]
    flags = (LOSS_FLAGS['max_violation'] if max_violation else 0) | (LOSS_FLAGS['mean'] if cost_style == 'mean' else 0)
    flags |= {'i2t': LOSS_FLAGS['i2t'], 't2i': LOSS_FLAGS['t2i'], 'bidir': LOSS_FLAGS['i2t'] | LOSS_FLAGS['t2i']}[direction]
    lib, h = _context(score.device)
    loss = (torch.empty if B else torch.zeros)((), dtype=torch.float32, device=score.device)
    d_score = torch.empty((B, ld), dtype=torch.float32, device=score.device) if want_grad else None     # the pitch of score
    _call('margin_loss_scores', lib.laff_margin_loss_scores, h, _ptr(score), ld, B, float(margin), flags, _ptr(loss), _ptr(d_score))
    return loss, (d_score[:, :B] if want_grad else None)


def gru_pack_whh(w_hh):
    """laff_gru_pack_whh: W_hh [3H, H] -> the step kernel's operand layout (a flat fp32 tensor of 3*H*H)."""
    w = _dev(w_hh, 'w_hh')
    if w.dim() != 2 or w.shape[0] != 3 * w.shape[1]:
        raise ValueError('w_hh must be (3H, H), got %s' % (tuple(w.shape),))
    w = w.contiguous()
    out = torch.empty(w.numel(), device=w.device, dtype=torch.float32)
    lib, h = _context(w.device)
    _call('gru_pack_whh', lib.laff_gru_pack_whh, h, _ptr(w), int(w.shape[1]), _ptr(out))
    return out


def gru_workspace_bytes(N, H, num_layers=1, bidirectional=False, pooling='mean'):
    return _size_query('laff_gru_workspace_bytes', N, H, num_layers, bool(bidirectional), GRU_POOLING[pooling])


def gru_encode(tokens, lengths, perm, batch_sizes, fwd, rev=None, pooling='mean', num_layers=1, out=None, workspace=None):
    """laff_gru_encode; the arguments are described at _gru_encode."""
    return _gru_encode(tokens, lengths, perm, batch_sizes, fwd, rev, pooling, num_layers, out, workspace, None)


def _gru_encode(tokens, lengths, perm, batch_sizes, fwd, rev, pooling, num_layers, out, workspace, reserve):
    """laff_gru_encode (reserve None) / laff_gru_encode_train.  tokens [T, N] int32 (time-major, length-sorted rows), lengths / perm [N] int32 on the device,
    batch_sizes: host sequence of T ints; fwd / rev: (P [V, 3H], packed W_hh, b_hh [3H]) of each direction (rev: bidirectional).
    Returns out [N, width] in the input order given by perm.  workspace: a uint8 device tensor of gru_workspace_bytes(...) bytes,
    or None to allocate one here (pass one for HIP-graph capture)."""
    tok = _dev(tokens, 'tokens', torch.int32)
    lens = _dev(lengths, 'lengths', torch.int32)
    prm = _dev(perm, 'perm', torch.int32)
    T, N = tok.shape
    P, Wp, bhh = fwd
    V, H3 = P.shape
    H = H3 // 3
    for t_, nm in ((P, 'P'), (Wp, 'whh'), (bhh, 'bhh')) + (((rev[0], 'P_rev'), (rev[1], 'whh_rev'), (rev[2], 'bhh_rev')) if rev else ()):
        _dev(t_, nm)
        if not t_.is_contiguous():
            raise ValueError('%s must be contiguous' % nm)
    if not tok.is_contiguous() or lens.numel() != N or prm.numel() != N:
        raise ValueError('tokens must be a contiguous [T, N] matrix and lengths / perm vectors of N')
    for P_, W_, b_ in (fwd, rev) if rev else (fwd,):
        if P_.dim() != 2 or P_.shape[1] != 3 * H or W_.numel() != 3 * H * H or b_.numel() != 3 * H:
            raise ValueError('each direction needs P [V, 3H], a packed W_hh of 3H*H and b_hh of 3H (H=%d)' % H)
        if P_.shape[0] != V:
            raise ValueError('both directions must use the same vocabulary')
    bs = (C.c_int * max(1, T))(*[int(b) for b in batch_sizes])
    if len(batch_sizes) != T:
        raise ValueError('batch_sizes has %d entries for T=%d' % (len(batch_sizes), T))
    bidir = rev is not None
    width = H if pooling == 'last' else 2 * H if (pooling == 'mean_last' or bidir) else H
    nbytes = gru_workspace_bytes(N, H, num_layers, bidir, pooling)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=tok.device)
    if out is None:
        out = torch.empty((N, width), device=tok.device, dtype=torch.float32)
    if tuple(out.shape) != (N, width):
        raise ValueError('out must be (%d, %d), got %s' % (N, width, tuple(out.shape)))
    o, ldo = _rows(out, 'out')
    Pr, Wr, br = rev if bidir else (None, None, None)
    lib, h = _context(tok.device)
    if reserve is not None:
        _call('gru_encode_train', lib.laff_gru_encode_train, h, _ptr(tok), _ptr(lens), _ptr(prm), bs, T, N, V, H, int(num_layers),
              int(bidir), GRU_POOLING[pooling], _ptr(P), _ptr(Wp), _ptr(bhh), _ptr(Pr), _ptr(Wr), _ptr(br), _ptr(o), ldo,
              _ptr(workspace), workspace.numel(), _ptr(reserve), reserve.numel())
        return out
    _call('gru_encode', lib.laff_gru_encode, h, _ptr(tok), _ptr(lens), _ptr(prm), bs, T, N, V, H, int(num_layers), int(bidir),
          GRU_POOLING[pooling], _ptr(P), _ptr(Wp), _ptr(bhh), _ptr(Pr), _ptr(Wr), _ptr(br), _ptr(o), ldo, _ptr(workspace),
          workspace.numel())
    return out


def gru_pack_whh_t(w_hh):
    """laff_gru_pack_whh_t: W_hh [3H, H] -> the backward step's operand layout (a flat fp32 tensor of 3*H*H)."""
    w = _dev(w_hh, 'w_hh')
    if w.dim() != 2 or w.shape[0] != 3 * w.shape[1]:
        raise ValueError('w_hh must be (3H, H), got %s' % (tuple(w.shape),))
    w = w.contiguous()
    out = torch.empty(w.numel(), device=w.device, dtype=torch.float32)
    lib, h = _context(w.device)
    _call('gru_pack_whh_t', lib.laff_gru_pack_whh_t, h, _ptr(w), int(w.shape[1]), _ptr(out))
    return out


def gru_gather_rows(table, ids, out=None):
    """laff_gru_gather_rows: table[ids] -- table [V, D] fp32, ids [M] int32 on the device -> [M, D]."""
    tb = _dev(table, 'table')
    ix = _dev(ids, 'ids', torch.int32)
    if tb.dim() != 2 or not tb.is_contiguous() or ix.dim() != 1 or not ix.is_contiguous():
        raise ValueError('table must be a contiguous matrix and ids a contiguous vector')
    M, (V, D) = ix.numel(), tb.shape
    if out is None:
        out = torch.empty((M, D), device=tb.device, dtype=torch.float32)
    if tuple(out.shape) != (M, D) or not _dev(out, 'out').is_contiguous():
        raise ValueError('out must be a contiguous (%d, %d) matrix' % (M, D))
    lib, h = _context(tb.device)
    _call('gru_gather_rows', lib.laff_gru_gather_rows, h, _ptr(tb), V, D, _ptr(ix), M, _ptr(out))
    return out


def _assemble_view(t, name, dims):
    """A device operand of batch_assemble with 4-byte elements (fp32 or int32) and unit inner stride, read or written IN PLACE (no copy
    of a resident array is ever made here); `dims`-dimensional.  Returns its row pitch in elements."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError('%s must be a CUDA (ROCm) tensor: laff_amd has no CPU path' % name)
    if t.dtype not in (torch.float32, torch.int32):
        raise TypeError('%s must be float32 or int32, got %s' % (name, t.dtype))
    if t.dim() != dims:
        raise ValueError('%s must be %d-D, got shape %s' % (name, dims, tuple(t.shape)))
    if dims == 1:
        if t.numel() > 1 and t.stride(0) != 1:
            raise ValueError('%s must be a contiguous vector' % name)
        return 1
    if dims == 3:
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous, got shape %s strides %s' % (name, tuple(t.shape), t.stride()))
        return t.shape[2]
    if t.numel() and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
        raise ValueError('%s must have contiguous rows, got shape %s strides %s' % (name, tuple(t.shape), t.stride()))
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def batch_assemble(jobs, control, control_host, B):
    """laff_batch_assemble: up to 16 gather jobs over the same B batch rows in one launch.  Every tensor is a device
    tensor of float32 or int32 that is read or written in place; `control` is the batch's int32 control block on the device and
    `control_host` the same values on the host (a numpy int32 array, e.g. the pinned block it was uploaded from).  A job is a tuple:
        ('rows', src, rows_at, dst)                      dst[b] = src[control[rows_at + b]]; src (Nsrc, w) and dst (B, w) row views
        ('ragged', src, seg_off, rows_at, dst, mask)     src (Nrows, w) row view, seg_off (Nseg + 1,) int32, dst (B, Fmax, w) contiguous,
                                                         mask (B, Fmax) fp32 contiguous or None; rows past a segment's end are zeros
        ('csr', (crow, col, val), rows_at, crow_at, (col_dst, val_dst))
                                                         the entries of row control[rows_at + b] to [control[crow_at + b], control[crow_at + b + 1])
    src and dst of a job have the same dtype.  Returns nothing: the destinations are the result."""
    B = int(B)
    jobs = list(jobs)
    if not 1 <= len(jobs) <= _lib.ASSEMBLE_MAX_JOBS:
        raise ValueError('batch_assemble takes 1 to %d jobs, got %d' % (_lib.ASSEMBLE_MAX_JOBS, len(jobs)))
    if not 1 <= B <= _lib.ASSEMBLE_MAX_BATCH:
        raise ValueError('batch_assemble takes 1 to %d batch rows, got %d' % (_lib.ASSEMBLE_MAX_BATCH, B))
    _dev(control, 'control', torch.int32)
    if control.dim() != 1 or not control.is_contiguous():
        raise ValueError('control must be a contiguous vector')
    host = control_host
    if not isinstance(host, np.ndarray) or host.dtype != np.int32 or host.ndim != 1 or not host.flags.c_contiguous:
        raise TypeError('control_host must be a contiguous 1-D numpy int32 array')
    if host.size != control.numel():
        raise ValueError('control_host has %d entries, control %d' % (host.size, control.numel()))
    dev = control.device
    arr = (_lib.AssembleJob * len(jobs))()

    def same(i, nm, t, dtype=None):
        if t.device != dev:
            raise ValueError('job %d: %s is on %s, control on %s' % (i, nm, t.device, dev))
        if dtype is not None and t.dtype != dtype:
            raise TypeError('job %d: %s must be %s, got %s' % (i, nm, dtype, t.dtype))

    for i, job in enumerate(jobs):
        kind = job[0]
        if kind not in _lib.ASSEMBLE_KIND:
            raise ValueError("job %d: unknown kind %r (one of 'rows', 'ragged', 'csr')" % (i, kind))
        q = arr[i]
        q.kind = _lib.ASSEMBLE_KIND[kind]
        if kind == 'rows':
            _, src, rows_at, dst = job
            q.ld_src, q.ld_dst = _assemble_view(src, 'job %d: src' % i, 2), _assemble_view(dst, 'job %d: dst' % i, 2)
            same(i, 'src', src), same(i, 'dst', dst, src.dtype)
            if dst.shape[0] != B or dst.shape[1] != src.shape[1]:
                raise ValueError('job %d: dst %s does not fit B = %d rows of src %s' % (i, tuple(dst.shape), B, tuple(src.shape)))
            q.w, q.n_src, q.rows_at = src.shape[1], src.shape[0], int(rows_at)
            q.src, q.dst = src.data_ptr(), dst.data_ptr()
        elif kind == 'ragged':
            _, src, seg_off, rows_at, dst, mask = job
            q.ld_src = _assemble_view(src, 'job %d: src' % i, 2)
            _assemble_view(dst, 'job %d: dst' % i, 3), _assemble_view(seg_off, 'job %d: seg_off' % i, 1)
            same(i, 'src', src), same(i, 'dst', dst, src.dtype), same(i, 'seg_off', seg_off, torch.int32)
            if dst.shape[0] != B or dst.shape[2] != src.shape[1] or seg_off.numel() < 2:
                raise ValueError('job %d: dst %s does not fit B = %d, src %s' % (i, tuple(dst.shape), B, tuple(src.shape)))
            if mask is not None:
                _assemble_view(mask, 'job %d: mask' % i, 2), same(i, 'mask', mask, torch.float32)
                if tuple(mask.shape) != tuple(dst.shape[:2]) or not mask.is_contiguous():
                    raise ValueError('job %d: mask must be a contiguous %s, got %s' % (i, tuple(dst.shape[:2]), tuple(mask.shape)))
                q.mask = mask.data_ptr()
            q.w, q.n_items, q.n_src, q.fmax, q.rows_at = src.shape[1], src.shape[0], seg_off.numel() - 1, dst.shape[1], int(rows_at)
            q.src, q.dst, q.off_src = src.data_ptr(), dst.data_ptr(), seg_off.data_ptr()
        else:
            _, (crow, col, val), rows_at, crow_at, (col_dst, val_dst) = job
            for nm, t, dt in (('crow', crow, torch.int32), ('col', col, torch.int32), ('val', val, None), ('col_dst', col_dst, torch.int32),
                              ('val_dst', val_dst, val.dtype)):
                _assemble_view(t, 'job %d: %s' % (i, nm), 1), same(i, nm, t, dt)
            if crow.numel() < 2 or col.numel() != val.numel() or col_dst.numel() != val_dst.numel():
                raise ValueError('job %d: crow has %d entries, col %d, val %d, col_dst %d, val_dst %d' %
                                 (i, crow.numel(), col.numel(), val.numel(), col_dst.numel(), val_dst.numel()))
            q.n_src, q.n_items, q.cap_dst, q.rows_at, q.crow_at = crow.numel() - 1, col.numel(), col_dst.numel(), int(rows_at), int(crow_at)
            # (an empty tensor has no storage: any aligned non-null address stands for it, nothing is read or written there)
            q.src, q.col_src = val.data_ptr() or control.data_ptr(), col.data_ptr() or control.data_ptr()
            q.dst, q.col_dst, q.off_src = val_dst.data_ptr() or control.data_ptr(), col_dst.data_ptr() or control.data_ptr(), crow.data_ptr()
    lib, h = _context(dev)
    _call('batch_assemble', lib.laff_batch_assemble, h, arr, len(jobs), B, _ptr(control), host.ctypes.data_as(C.c_void_p), host.size)


def _batch_sizes(batch_sizes):
    return (C.c_int * max(1, len(batch_sizes)))(*[int(b) for b in batch_sizes]), len(batch_sizes)


def gru_train_reserve_bytes(M, H, num_layers=1, bidirectional=False, pooling='mean'):
    return _size_query('laff_gru_train_reserve_bytes', M, H, num_layers, bool(bidirectional), GRU_POOLING[pooling])


def gru_backward_plan(batch_sizes, H, bidirectional=False, pooling='mean'):
    """laff_gru_backward_plan (host only): (fwd, bwd), per launch 1 where the saving forward / the backward step takes the 64 x 32 tile."""
    bs, T = _batch_sizes(batch_sizes)
    fwd, bwd = (C.c_int * max(1, T))(), (C.c_int * max(1, T))()
    check(_lib.load().laff_gru_backward_plan(bs, T, int(H), int(bool(bidirectional)), GRU_POOLING[pooling], fwd, bwd))
    return tuple(fwd[:T]), tuple(bwd[:T])


def gru_backward_workspace_bytes(batch_sizes, N, H, we_dim, num_layers=1, bidirectional=False, pooling='mean', want_dwe=True):
    bs, T = _batch_sizes(batch_sizes)
    n = C.c_size_t()
    check(_lib.load().laff_gru_backward_workspace_bytes(bs, T, int(N), int(H), int(we_dim), int(num_layers), int(bool(bidirectional)),
                                                        GRU_POOLING[pooling], int(bool(want_dwe)), C.byref(n)))
    return n.value


def gru_encode_train(pos, lengths, perm, batch_sizes, fwd, rev=None, pooling='mean', num_layers=1, out=None, workspace=None,
                     reserve=None):
    """laff_gru_encode_train: gru_encode with the batch's own table -- fwd / rev = (GI [M, 3H] = X . W_ih^T + b_ih, packed W_hh,
    b_hh [3H]), pos [T, N] int32 the packed positions -- that also fills reserve (a uint8 device tensor of gru_train_reserve_bytes
    bytes, allocated here when None) for gru_backward.  Returns (out, reserve)."""
    M, H = fwd[0].shape[0], fwd[0].shape[1] // 3
    bidir = rev is not None
    nbytes = gru_train_reserve_bytes(M, H, num_layers, bidir, pooling)
    if reserve is None:
        reserve = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=fwd[0].device)
    _dev(reserve, 'reserve', torch.uint8)
    return _gru_encode(pos, lengths, perm, batch_sizes, fwd, rev, pooling, num_layers, out, workspace, reserve), reserve


def gru_backward(grad_out, lengths, perm, batch_sizes, reserve, x, fwd, rev=None, pooling='mean', segments=None, vocab=None,
                 want=None, out=None, workspace=None, num_layers=1):
    """laff_gru_backward.  grad_out [N, width] (input order); lengths / perm as gru_encode takes them; reserve from gru_encode_train;
    x [M, we_dim] = we[tokens] in packed order; fwd / rev = (W_ih [3H, we_dim], transposed pack of W_hh) per direction.
    segments = (seg_off [U + 1], seg_tok [U], seg_pos [M]) int32 device vectors and vocab = V ask for d_we [V, we_dim].
    want: per direction four flags (dW_ih, dW_hh, db_ih, db_hh), default all.  out: {'d_we': ..., 'fwd': [4], 'rev': [4]} buffers to
    write into (missing ones are allocated here).  Returns (d_we | None, [4 tensors | None] forward, the same reverse | None)."""
    g, lddo = _rows(grad_out if grad_out.stride(-1) == 1 else grad_out.contiguous(), 'grad_out')
    lens, prm = _dev(lengths, 'lengths', torch.int32), _dev(perm, 'perm', torch.int32)
    x = _dev(x, 'x')
    dev, N, bidir = g.device, g.shape[0], rev is not None
    (M, we_dim), H = x.shape, fwd[0].shape[0] // 3
    if not x.is_contiguous() or lens.numel() != N or prm.numel() != N:
        raise ValueError('x must be contiguous and lengths / perm vectors of N=%d' % N)
    for w_ih, wt in (fwd, rev) if bidir else (fwd,):
        _dev(w_ih, 'W_ih')
        _dev(wt, 'packed W_hh')
        if tuple(w_ih.shape) != (3 * H, we_dim) or not w_ih.is_contiguous() or wt.numel() != 3 * H * H or not wt.is_contiguous():
            raise ValueError('each direction needs a contiguous W_ih [3H, we_dim] and a transposed pack of W_hh (H=%d)' % H)
    width = H if pooling == 'last' else 2 * H if (pooling == 'mean_last' or bidir) else H
    if g.shape[1] != width:
        raise ValueError('grad_out must be (%d, %d), got %s' % (N, width, tuple(g.shape)))
    bs, T = _batch_sizes(batch_sizes)
    _dev(reserve, 'reserve', torch.uint8)
    out = out or {}
    want = want or ([True] * 4, [True] * 4)
    shapes = ((3 * H, we_dim), (3 * H, H), (3 * H,), (3 * H,))

    def side(key, flags):
        given = out.get(key) or [None] * 4
        ts = []
        for f, s, t in zip(flags, shapes, given):
            if f and t is None:
                t = torch.empty(s, device=dev, dtype=torch.float32)
            if f and (tuple(_dev(t, key).shape) != s or not t.is_contiguous()):
                raise ValueError('out %s: a gradient buffer must be contiguous %s' % (key, s))
            ts.append(t if f else None)
        return ts, (C.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in ts])
    gf, pf = side('fwd', want[0])
    gr, pr = side('rev', want[1]) if bidir else (None, None)
    d_we, seg = None, (None, None, None)
    U = V = 0
    if segments is not None:
        seg = tuple(_dev(s, 'segments', torch.int32) for s in segments)
        U, V = seg[1].numel(), int(vocab)
        if seg[0].numel() != U + 1 or seg[2].numel() != M or not all(s.is_contiguous() for s in seg):
            raise ValueError('segments must be contiguous vectors of U + 1, U and M = %d entries' % M)
        d_we = out.get('d_we')
        if d_we is None:
            d_we = torch.empty((V, we_dim), device=dev, dtype=torch.float32)
        if tuple(_dev(d_we, 'd_we').shape) != (V, we_dim) or not d_we.is_contiguous():
            raise ValueError('out d_we must be a contiguous (%d, %d) matrix' % (V, we_dim))
    nbytes = gru_backward_workspace_bytes(batch_sizes, N, H, we_dim, num_layers, bidir, pooling, d_we is not None)
    if workspace is None:
        workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    lib, h = _context(dev)
    _call('gru_backward', lib.laff_gru_backward, h, _ptr(lens), _ptr(prm), bs, T, N, M, H, we_dim, int(num_layers), int(bidir),
          GRU_POOLING[pooling], _ptr(g), lddo, _ptr(reserve), reserve.numel(), _ptr(x), _ptr(fwd[0]), _ptr(fwd[1]),
          _ptr(rev[0]) if bidir else None, _ptr(rev[1]) if bidir else None, _ptr(seg[0]), _ptr(seg[1]), _ptr(seg[2]), U, max(V, 1),
          _ptr(d_we), pf, pr, _ptr(workspace), workspace.numel())
    return d_we, gf, gr


def clip_pack_weight(w, precision='fp16', transpose=False, padded_cols=None):
    """laff_clip_pack_weight: an fp32 weight [rows, cols] -> the CLIP GEMM operand in the encoder's precision (fp16 or fp32),
    [rows, cols], or [cols, rows] with transpose (text_projection).  padded_cols: laff_clip_pack_weight_padded, [rows, padded_cols]
    zero past cols (conv1.weight viewed as [width, 3 p^2])."""
    w = _dev(w, 'w')
    if w.dim() != 2:
        raise ValueError('w must be 2-D, got %s' % (tuple(w.shape),))
    w = w.contiguous()
    rows, cols = w.shape
    dt = torch.float16 if precision == 'fp16' else torch.float32
    lib, h = _context(w.device)
    if padded_cols is not None:
        out = torch.empty((rows, int(padded_cols)), device=w.device, dtype=dt)
        _call('clip_pack_weight_padded', lib.laff_clip_pack_weight_padded, h, _ptr(w), int(rows), int(cols), int(padded_cols),
              PREC[precision], _ptr(out))
        return out
    out = torch.empty((cols, rows) if transpose else (rows, cols), device=w.device, dtype=dt)
    _call('clip_pack_weight', lib.laff_clip_pack_weight, h, _ptr(w), int(rows), int(cols), int(bool(transpose)), PREC[precision],
          _ptr(out))
    return out


def _text_encode(name, ids, row_off, row_off_host, model, precision, out, workspace, nbytes, width):
    """clip_encode / bert_encode (laff_<name>): nbytes(R, N) is the workspace query, width the columns of out."""
    ids = _dev(ids, 'ids', torch.int32)
    if ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError('ids and row_off must be contiguous vectors')
    row_off, roh, N = _offsets(row_off, row_off_host, 'row_off')
    R = ids.numel()
    workspace, out, o, ldo = _ws_out(workspace, lambda: nbytes(R, N), out, (N, width), ids.device)
    lib, h = _context(ids.device)
    _call(name, getattr(lib, 'laff_' + name), h, _ptr(ids), _ptr(row_off), roh.ctypes.data_as(C.POINTER(C.c_int)), N, R, C.byref(model),
          PREC[precision], o, ldo, _ptr(workspace), workspace.numel())
    return out


def clip_workspace_bytes(R, N, width, precision='fp16'):
    return _size_query('laff_clip_workspace_bytes', R, N, width, PREC[precision])


def clip_encode(ids, row_off, row_off_host, model, precision='fp16', out=None, workspace=None):
    """laff_clip_encode.  ids [R] int32 (the captions' rows concatenated) and row_off [N+1] int32 on the device, row_off_host: the
    same offsets as a host int32 array; model: a laff_amd._lib.ClipText of device pointers (ClipTxtEncoder builds it).  Returns out
    [N, embed_dim] fp32.  workspace: a uint8 device tensor of clip_workspace_bytes(R, N, width, precision) bytes, or None to
    allocate one here (pass one for HIP-graph capture)."""
    return _text_encode('clip_encode', ids, row_off, row_off_host, model, precision, out, workspace,
                        lambda R, N: clip_workspace_bytes(R, N, model.width, precision), model.embed_dim)


def bert_workspace_bytes(R, N, width, intermediate, precision='fp32'):
    return _size_query('laff_bert_workspace_bytes', R, N, width, intermediate, PREC[precision])


def bert_encode(ids, row_off, row_off_host, model, precision='fp32', out=None, workspace=None):
    """laff_bert_encode.  ids [R] int32 (the captions' wordpiece rows concatenated) and row_off [N+1] int32 on the device,
    row_off_host: the same offsets as a host int32 array; model: a laff_amd._lib.BertText of device pointers (BertTxtEncoder builds
    it).  Returns out [N, width] fp32 (pooler_output).  workspace: a uint8 device tensor of bert_workspace_bytes(R, N, ...) bytes, or
    None to allocate one here (pass one for HIP-graph capture)."""
    return _text_encode('bert_encode', ids, row_off, row_off_host, model, precision, out, workspace,
                        lambda R, N: bert_workspace_bytes(R, N, model.width, model.intermediate, precision), model.width)


def netvlad_workspace_bytes(R, K):
    return _size_query('laff_netvlad_workspace_bytes', R, K)


def netvlad_train_reserve_bytes(N, R, K):
    return _size_query('laff_netvlad_train_reserve_bytes', N, R, K)


def netvlad_backward_workspace_bytes(N, R, K, D):
    return _size_query('laff_netvlad_backward_workspace_bytes', N, R, K, D)


def _netvlad_args(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids):
    """What netvlad_encode, netvlad_encode_train and netvlad_backward check alike.  Returns the arguments table .. K that their C calls
    share after the context, (V, D, K, R, N) and the tensors that have to outlive the call."""
    table, fc1_weight, centroids = _dev(table, 'table'), _dev(fc1_weight, 'fc1_weight'), _dev(centroids, 'centroids')
    ids, row_off = _dev(ids, 'ids', torch.int32), _dev(row_off, 'row_off', torch.int32)
    zero_rows = _dev(zero_rows, 'zero_rows', torch.int32)
    for t, nm in ((table, 'table'), (fc1_weight, 'fc1_weight'), (centroids, 'centroids'), (ids, 'ids'), (row_off, 'row_off'),
                  (zero_rows, 'zero_rows')):
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % nm)
    if table.dim() != 2 or ids.dim() != 1 or row_off.dim() != 1:
        raise ValueError('table must be [V, D], ids and row_off vectors')
    V, D = table.shape
    K = fc1_weight.shape[0]
    if tuple(fc1_weight.shape) != (K, D) or tuple(centroids.shape) != (K, D):
        raise ValueError('fc1_weight and centroids must both be [K, %d], got %s and %s' % (D, tuple(fc1_weight.shape),
                                                                                           tuple(centroids.shape)))
    R, N = ids.numel(), row_off.numel() - 1
    if zero_rows.numel() != N:
        raise ValueError('zero_rows has %d entries for %d captions' % (zero_rows.numel(), N))
    row_off, roh, N = _offsets(row_off, row_off_host, 'row_off')
    keep = (table, ids, row_off, roh, zero_rows, fc1_weight, centroids)
    head = (_ptr(table), V, D, _ptr(ids), _ptr(row_off), roh.ctypes.data_as(C.POINTER(C.c_int)), _ptr(zero_rows), N, R,
            _ptr(fc1_weight), _ptr(centroids), K)
    return head, (V, D, K, R, N), keep


def netvlad_encode(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids, out=None, workspace=None):
    """laff_netvlad_encode.  table [V, D] fp32 (word2vec rows), ids [R] int32, row_off [N+1] int32 and zero_rows [N] int32 on the
    device, row_off_host: the same offsets as a host int32 array; fc1_weight / centroids [K, D] fp32.  Returns out [N, K*D] fp32.
    workspace: a uint8 device tensor of netvlad_workspace_bytes(R, K) bytes, or None to allocate one here (pass one for HIP-graph
    capture)."""
    head, (V, D, K, R, N), keep = _netvlad_args(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids)
    workspace, out, o, ldo = _ws_out(workspace, lambda: netvlad_workspace_bytes(R, K), out, (N, K * D), keep[0].device)
    lib, h = _context(keep[0].device)
    _call('netvlad_encode', lib.laff_netvlad_encode, h, *head, o, ldo, _ptr(workspace), workspace.numel())
    return out


def _byte_buffer(buf, name, nbytes, device):
    """A caller's uint8 device buffer of at least nbytes, or a fresh one."""
    if buf is None:
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
    _dev(buf, name, torch.uint8)
    if buf.numel() < nbytes:
        raise ValueError('%s has %d bytes, %d are needed' % (name, buf.numel(), nbytes))
    return buf


def netvlad_encode_train(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids, out=None, reserve=None):
    """laff_netvlad_encode_train: netvlad_encode (the same bits) that also fills reserve, a uint8 device tensor of
    netvlad_train_reserve_bytes(N, R, K) bytes (allocated here when None), for netvlad_backward.  It needs no workspace: the
    assignments go straight into the reserve.  Returns (out, reserve)."""
    head, (V, D, K, R, N), keep = _netvlad_args(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids)
    dev = keep[0].device
    reserve = _byte_buffer(reserve, 'reserve', netvlad_train_reserve_bytes(N, R, K), dev)
    out, o, ldo = _out_rows(out, (N, K * D), dev)
    lib, h = _context(dev)
    _call('netvlad_encode_train', lib.laff_netvlad_encode_train, h, *head, o, ldo, _ptr(reserve), reserve.numel(), None, 0)
    return out, reserve


def netvlad_backward(grad_out, out, reserve, table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids, want=(True, True),
                     d_fc1=None, d_centroids=None, workspace=None):
    """laff_netvlad_backward.  grad_out [N, K*D] the gradient of out (the forward's output, with its reserve from
    netvlad_encode_train on the same batch and parameters).  want = (d_fc1, d_centroids): which gradients to form; d_fc1 /
    d_centroids: contiguous [K, D] fp32 buffers to write into (allocated here when wanted and None); workspace: a uint8 device
    tensor of netvlad_backward_workspace_bytes(N, R, K, D) bytes, or None to allocate one.  Returns (d_fc1 | None, d_centroids | None)."""
    head, (V, D, K, R, N), keep = _netvlad_args(table, ids, row_off, row_off_host, zero_rows, fc1_weight, centroids)
    dev = keep[0].device
    g, ldg = _mat(grad_out, 'grad_out', align16=True)
    o, ldo = _rows(out, 'out')
    if tuple(g.shape) != (N, K * D) or tuple(o.shape) != (N, K * D):
        raise ValueError('grad_out and out must both be (%d, %d), got %s and %s' % (N, K * D, tuple(g.shape), tuple(o.shape)))
    reserve = _byte_buffer(_dev(reserve, 'reserve', torch.uint8), 'reserve', netvlad_train_reserve_bytes(N, R, K), dev)
    grads = []
    for flag, t, nm in ((want[0], d_fc1, 'd_fc1'), (want[1], d_centroids, 'd_centroids')):
        if flag and t is None:
            t = torch.empty((K, D), device=dev, dtype=torch.float32)
        if flag and (tuple(_dev(t, nm).shape) != (K, D) or not t.is_contiguous()):
            raise ValueError('%s must be a contiguous (%d, %d) matrix' % (nm, K, D))
        grads.append(t if flag else None)
    workspace = _byte_buffer(workspace, 'workspace', netvlad_backward_workspace_bytes(N, R, K, D), dev)
    lib, h = _context(dev)
    _call('netvlad_backward', lib.laff_netvlad_backward, h, *head, _ptr(o), ldo, _ptr(g), ldg, _ptr(reserve), reserve.numel(),
          _ptr(grads[0]), _ptr(grads[1]), _ptr(workspace), workspace.numel())
    return grads[0], grads[1]


def clip_image_kpad(patch_size, precision='fp16'):
    """laff_clip_image_kpad: the padded K of the patch GEMM (3 p^2 rounded up to the GEMM's 128-byte K-step)."""
    n = C.c_int()
    check(_lib.load().laff_clip_image_kpad(int(patch_size), PREC[precision], C.byref(n)))
    return n.value


def clip_image_workspace_bytes(F, width, input_resolution, patch_size, precision='fp16'):
    return _size_query('laff_clip_image_workspace_bytes', F, width, input_resolution, patch_size, PREC[precision])


def clip_image_encode(pixels, frame_off, frame_off_host, model, precision='fp16', out=None, out_mean=None, workspace=None):
    """laff_clip_image_encode.  pixels [F, 3, R, R] fp32 (contiguous NCHW) on the device; frame_off [V+1] int32 on the device and
    frame_off_host: the same offsets as a host int32 array (V = 0: both may be None, no means); model: a laff_amd._lib.ClipVisual of
    device pointers (ClipImageEncoder builds it).  Returns (out [F, embed_dim], out_mean [V, embed_dim] or None), fp32.  workspace: a
    uint8 device tensor of clip_image_workspace_bytes(F, ...) bytes, or None to allocate one here (pass one for HIP-graph capture)."""
    pixels = _dev(pixels, 'pixels')
    R = model.input_resolution
    if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, R, R) or not pixels.is_contiguous():
        raise ValueError('pixels must be a contiguous [F, 3, %d, %d] tensor, got %s' % (R, R, tuple(pixels.shape)))
    F = pixels.shape[0]
    if frame_off is None:
        V, fo, roh = 0, None, np.zeros(1, np.int32)
    else:
        fo, roh, V = _offsets(frame_off, frame_off_host, 'frame_off')
    E = model.embed_dim
    workspace, out, o, ldo = _ws_out(workspace, lambda: clip_image_workspace_bytes(F, model.width, R, model.patch_size, precision), out,
                                     (F, E), pixels.device)
    mo, ldm = None, E
    if V > 0:
        out_mean, mo, ldm = _out_rows(out_mean, (V, E), pixels.device, 'out_mean')
    lib, h = _context(pixels.device)
    _call('clip_image_encode', lib.laff_clip_image_encode, h, _ptr(pixels), F, _ptr(fo), roh.ctypes.data_as(C.POINTER(C.c_int)), V,
          C.byref(model), PREC[precision], o, ldo, mo, ldm, _ptr(workspace), workspace.numel())
    return out, (out_mean if V > 0 else None)


#: frames per laff_frame_preprocess call (the kernel's grid.y)
FRAME_PREP_MAX_FRAMES = 65535


def frame_desc_device(desc, F, device):
    """A _lib.FrameDesc array's first F descriptors as a uint8 device tensor."""
    raw = np.frombuffer(memoryview(desc), dtype=np.uint8)[:F * C.sizeof(_lib.FrameDesc)].copy()
    return torch.from_numpy(raw).to(device)


def frame_preprocess(frames, desc, F, R, taps, taps_host, mean, std, out=None, out_u8=None, desc_dev=None):
    """laff_frame_preprocess.  frames: uint8 device buffer of packed HWC frames; desc: a _lib.FrameDesc array of F descriptors (host;
    desc_dev: the same bytes on the device, or None to copy them here -- pass one for HIP-graph capture); taps: the int32 tap tables on
    the device and taps_host the same words as a host int32 array; mean, std: 3 floats each.  Returns out [F, 3, R, R] fp32; out_u8
    [F, R, R, 3] uint8, when given, receives the resized, cropped image."""
    frames = _dev(frames, 'frames', torch.uint8)
    taps = _dev(taps, 'taps', torch.int32)
    F, R = int(F), int(R)
    th = np.ascontiguousarray(taps_host, dtype=np.int32)
    if not frames.is_contiguous() or not taps.is_contiguous() or taps.numel() != th.size:
        raise ValueError('frames / taps must be contiguous and taps_host must hold the words of taps')
    if len(desc) < F:
        raise ValueError('desc holds %d descriptors, F = %d' % (len(desc), F))
    if out is None:
        out = torch.empty((F, 3, R, R), device=frames.device, dtype=torch.float32)
    _dev(out, 'out')
    if tuple(out.shape) != (F, 3, R, R) or not out.is_contiguous():
        raise ValueError('out must be a contiguous (%d, 3, %d, %d) tensor, got %s' % (F, R, R, tuple(out.shape)))
    if out_u8 is not None:
        _dev(out_u8, 'out_u8', torch.uint8)
        if tuple(out_u8.shape) != (F, R, R, 3) or not out_u8.is_contiguous():
            raise ValueError('out_u8 must be a contiguous (%d, %d, %d, 3) tensor, got %s' % (F, R, R, tuple(out_u8.shape)))
    if desc_dev is None and F:
        desc_dev = frame_desc_device(desc, F, frames.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    sd = (C.c_float * 3)(*[float(v) for v in std])
    lib, h = _context(frames.device)
    _call('frame_preprocess', lib.laff_frame_preprocess, h, _ptr(frames), frames.numel(), _ptr(desc_dev), C.cast(desc, C.c_void_p), F, R,
          _ptr(taps), C.c_void_p(th.ctypes.data), th.size, m, sd, _ptr(out), _ptr(out_u8), None, 0)
    return out


class SplitOperand:
    """fp16 hi/lo split of an fp32 matrix (laff_split_rows): buffer [2][N][Kp] + per-row reciprocal scales."""

    def __init__(self, buf, rscale, N, K):
        self.buf, self.rscale, self.N, self.K = buf, rscale, N, K


def split_rows(x):
    return split_rows_grouped([x])[0]


def split_rows_grouped(xs):
    """split_rows for several matrices in one launch."""
    if not xs:
        return []
    n = len(xs)
    lib, h = _context(xs[0].device)
    X, N, K, LD, O, R = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    outs = []
    for i, x in enumerate(xs):
        x, ldx = _rows(x, 'x')
        nbytes = C.c_size_t()
        check(lib.laff_split_rows_bytes(x.shape[0], x.shape[1], C.byref(nbytes)))
        buf = torch.empty((max(nbytes.value, 16),), device=x.device, dtype=torch.uint8)
        rscale = torch.empty((max(x.shape[0], 1),), device=x.device, dtype=torch.float32)
        X[i], N[i], K[i], LD[i], O[i], R[i] = x.data_ptr(), x.shape[0], x.shape[1], ldx, buf.data_ptr(), rscale.data_ptr()
        outs.append(SplitOperand(buf, rscale, x.shape[0], x.shape[1]))
    _call('split_rows', lib.laff_split_rows_grouped, h, n, X, N, K, LD, O, R)
    return outs


def fc_act_bn_split_grouped(problems):
    """fc_act_bn_grouped on the fp16 matrix pipe with fp32-class accuracy.  problems: dicts with x (fp32 tensor or
    SplitOperand), weight_split (SplitOperand of W), optional bias / bn_scale / bn_shift / activation / out."""
    if not problems:
        return []
    arr = (FcSplitProblem * len(problems))()
    outs = []
    dev = problems[0]['weight_split'].buf.device
    todo = [i for i, q in enumerate(problems) if not isinstance(q['x'], SplitOperand)]
    split = dict(zip(todo, split_rows_grouped([problems[i]['x'] for i in todo])))      # all inputs in ONE launch
    for i, q in enumerate(problems):
        xs = split.get(i, q['x'])
        ws = q['weight_split']
        if xs.K != ws.K:
            raise ValueError('problem %d: x has %d columns, weight %d' % (i, xs.K, ws.K))
        N, D = xs.N, ws.N
        vecs, out, ldy = _fc_epilogue(q, N, D, dev)
        arr[i] = FcSplitProblem(xs.buf.data_ptr(), xs.rscale.data_ptr(), N, xs.K, ws.buf.data_ptr(), ws.rscale.data_ptr(), *vecs, D,
                                ACT[q.get('activation')], out.data_ptr(), ldy)
        outs.append(out)
    lib, h = _context(dev)
    _call('fc_act_bn', lib.laff_fc_act_bn_split_grouped, h, arr, len(problems))
    return outs


def fused_split_eligible(x, weight_split):
    """Can laff_fc_act_bn_fused_grouped take this input?  (fp32 CUDA matrix, 16-byte aligned rows, K a multiple of 32.)"""
    return (torch.is_tensor(x) and x.is_cuda and x.layout == torch.strided and x.dtype == torch.float32 and x.dim() == 2 and
            x.shape[1] % 32 == 0 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and
            x.shape[1] == weight_split.K)


def fc_act_bn_fused_grouped(problems):
    """fc_act_bn_split_grouped without materialising the split of the inputs: one pass over the inputs for their per-row scales
    (laff_row_scales_grouped), then the GEMM splits them on the way into LDS.  problems: dicts with x (fp32 tensor),
    weight_split (SplitOperand of W), optional bias / bn_scale / bn_shift / activation / out."""
    if not problems:
        return []
    n = len(problems)
    dev = problems[0]['weight_split'].buf.device
    lib, h = _context(dev)
    X, N, K, LD, R = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_void_p * n)()
    arr = (FcFusedProblem * n)()
    outs = []
    total = sum(q['x'].shape[0] for q in problems)
    scales = torch.empty((max(total, 1),), device=dev, dtype=torch.float32)      # one buffer, one slice per problem
    at = 0
    for i, q in enumerate(problems):
        x, ldx = _rows(q['x'], 'x')
        ws = q['weight_split']
        if not fused_split_eligible(x, ws):
            raise ValueError('problem %d is not eligible for the fused split (see fused_split_eligible)' % i)
        rs = scales[at:at + x.shape[0]]
        at += x.shape[0]
        X[i], N[i], K[i], LD[i], R[i] = x.data_ptr(), x.shape[0], x.shape[1], ldx, rs.data_ptr()
        D = ws.N
        vecs, out, ldy = _fc_epilogue(q, x.shape[0], D, dev)
        arr[i] = FcFusedProblem(x.data_ptr(), ldx, rs.data_ptr(), x.shape[0], x.shape[1], ws.buf.data_ptr(), ws.rscale.data_ptr(),
                                *vecs, D, ACT[q.get('activation')], out.data_ptr(), ldy)
        outs.append(out)
    _call('row_scales', lib.laff_row_scales_grouped, h, n, X, N, K, LD, R)
    _call('fc_act_bn', lib.laff_fc_act_bn_fused_grouped, h, arr, n)
    return outs


#: the kernels behind the FC projections (LAFF_FC_KERNEL_* of include/laff_hip.h, in that order).  The first six are what
#: fc_act_bn_grouped / fc_act_bn_split_grouped / fc_act_bn_fused_grouped choose between; fc_act_bn_strip_grouped, fc_gather_act_bn and
#: fc_concat_act_bn_grouped each have a kernel family of their own.
FC_ROUTES = _lib.enum_names('LAFF_FC_KERNEL_')[:_lib.K['LAFF_FC_KERNEL_CONCAT'] + 1]      # F16_256, behind it, is no FC entry point's kernel
_FC_FAMILIES = {k: _lib.K['LAFF_FC_FAMILY_' + c] for k, c in (('fp32', 'F32'), ('split', 'SPLIT'), ('fused', 'FUSED'))}
_FC_OWN_KERNEL = {'strip': 'STRIP', 'gather': 'GATHER', 'concat': 'CONCAT'}


class FcRoute:
    """What fc_route reports.  kinds: per problem, the staging kind 0 / 1 / 2 (family 'fp32') or the tile edge 128 / 256 ('split',
    'fused'), None for an empty problem; launch_of: per problem, the index of its launch (None: empty); launches: in launch order,
    dicts with kernel (FC_ROUTES), problems (indices), tiles, nbig and quarters (the split tile's tail split, 0 elsewhere)."""

    def __init__(self, kinds, launch_of, launches):
        self.kinds, self.launch_of, self.launches = kinds, launch_of, launches

    @property
    def kernels(self):
        return [l['kernel'] for l in self.launches]


def fc_route(family, shapes, device=None):
    """Which kernels an FC entry point runs for a list of problems, in launch order; launches nothing (laff_fc_route: the answer of the
    functions the launches themselves go through, with the CU count of the device's context).
    family: 'fp32' (fc_act_bn_grouped), 'split' (fc_act_bn_split_grouped), 'fused' (fc_act_bn_fused_grouped); 'strip', 'gather' and
    'concat' (fc_act_bn_strip_grouped, fc_gather_act_bn, fc_concat_act_bn_grouped) have one kernel family each and are only named.
    shapes: dicts with N, Dk, D and optional ldx, ldw (default Dk), x_aligned, w_aligned (16-byte aligned bases, default True) --
    or with x and weight, the tensors themselves (weight may be a SplitOperand)."""
    if family in _FC_OWN_KERNEL:
        k = _FC_OWN_KERNEL[family]
        return FcRoute([None] * len(shapes), [None] * len(shapes), [dict(kernel=k, problems=list(range(len(shapes))), tiles=0, nbig=0,
                                                                         quarters=0)])
    if family not in _FC_FAMILIES:
        raise ValueError('family must be one of %s, got %r' % (sorted(list(_FC_FAMILIES) + list(_FC_OWN_KERNEL)), family))
    n = len(shapes)
    arr = (FcShape * max(n, 1))()
    for i, q in enumerate(shapes):
        if 'x' in q:
            x, w = q['x'], q.get('weight', q.get('weight_split'))
            if isinstance(x, SplitOperand):
                N, Dk, ldx, xa = x.N, x.K, x.K, True
            else:
                N, Dk, ldx, xa = x.shape[0], x.shape[1], _rows(x, 'x')[1], x.data_ptr() % 16 == 0
            if isinstance(w, SplitOperand):
                D, ldw, wa = w.N, w.K, True
            else:
                D, ldw, wa = w.shape[0], _rows(w, 'weight')[1], w.data_ptr() % 16 == 0
            if device is None:
                device = (x.buf if isinstance(x, SplitOperand) else x).device
        else:
            N, Dk, D = int(q['N']), int(q['Dk']), int(q['D'])
            ldx, ldw = int(q.get('ldx', Dk)), int(q.get('ldw', Dk))
            xa, wa = bool(q.get('x_aligned', True)), bool(q.get('w_aligned', True))
        arr[i] = FcShape(N, Dk, D, ldx, ldw, int(xa), int(wa))
    lib, h = _context(torch.device(device) if device is not None else torch.device('cuda'))
    kind, launch_of = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    cap = 3 * (n // 8 + 1)
    launches, nl = (FcLaunch * cap)(), C.c_int(0)
    check(lib.laff_fc_route(h, _FC_FAMILIES[family], arr, n, kind, launch_of, launches, cap, C.byref(nl)))
    out = []
    for j in range(nl.value):
        l = launches[j]
        if l.kernel >= len(FC_ROUTES):
            raise RuntimeError('laff_fc_route: kernel %d is not an FC route' % l.kernel)
        out.append(dict(kernel=FC_ROUTES[l.kernel], problems=[i for i in range(n) if launch_of[i] == j], tiles=int(l.tiles),
                        nbig=int(l.nbig), quarters=int(l.quarters)))
        assert len(out[-1]['problems']) == l.count
    return FcRoute([kind[i] if kind[i] >= 0 else None for i in range(n)], [launch_of[i] if launch_of[i] >= 0 else None for i in range(n)],
                   out)


class StripWeights:
    """A TransformNet's parameters packed for the strip-form FC (laff_fc_strip_pack): the W stream's LDS image + the per-column
    epilogue constants (bias, activation and folded BatchNorm combined)."""

    def __init__(self, img, D, K, act, mfma):
        self.img, self.D, self.K, self.act, self.mfma = img, D, K, act, mfma       # mfma: the LAFF_FC_STRIP_MFMA mode it was packed under


def fc_strip_pack(weight, bias=None, bn_scale=None, bn_shift=None, activation=None):
    """Pack W [D, 512] (+ bias / folded BatchNorm / activation) once per model for fc_act_bn_strip_grouped.
    The image's layout follows the context's LAFF_FC_STRIP_MFMA mode (16 by default, 32: the 32x32x16 kernel; read when the context
    is created) and is recorded in the result: fc_act_bn_strip_grouped refuses an image packed under the other mode, so pack again
    after changing the mode (ops.reset_contexts())."""
    w, ldw = _rows(weight, 'weight')
    D, K = w.shape
    lib, h = _context(w.device)
    nbytes = C.c_size_t()
    check(lib.laff_fc_strip_pack_bytes(D, K, C.byref(nbytes)))
    vecs = _fc_vectors(dict(bias=bias, bn_scale=bn_scale, bn_shift=bn_shift), D)
    img = torch.empty((nbytes.value,), device=w.device, dtype=torch.uint8)
    _call('fc_strip_pack', lib.laff_fc_strip_pack, h, _ptr(w), ldw, *vecs, D, K, ACT[activation], _ptr(img))
    return StripWeights(img, D, K, ACT[activation], _fc_strip_mfma)


def fc_strip_eligible(x, D):
    """Can laff_fc_act_bn_strip_grouped take this input?  (fp32 CUDA matrix of 512 columns, 16-byte aligned rows, D % 32 == 0.)"""
    return (torch.is_tensor(x) and x.is_cuda and x.layout == torch.strided and x.dtype == torch.float32 and x.dim() == 2 and
            x.shape[1] == 512 and (x.shape[0] == 0 or (x.stride(1) == 1 and (x.stride(0) % 4 == 0 or x.shape[0] == 1) and
                                                       x.data_ptr() % 16 == 0)) and D % 32 == 0 and D >= 32)


def fc_act_bn_strip_grouped(problems):
    """TransformNet.forward for several features in the strip form (X stationary in registers, no row-scale pass).
    problems: dicts with x (fp32 tensor [N, 512]), strip (StripWeights), optional out.  Returns the list of outputs."""
    if not problems:
        return []
    n = len(problems)
    arr = (FcStripProblem * n)()
    outs = []
    dev = problems[0]['strip'].img.device
    for i, q in enumerate(problems):
        x, ldx = _rows(q['x'], 'x')
        sw = q['strip']
        if not fc_strip_eligible(x, sw.D):
            raise ValueError('problem %d is not eligible for the strip form (see fc_strip_eligible)' % i)
        out = q.get('out')
        if out is None:
            out = torch.empty((x.shape[0], sw.D), device=dev, dtype=torch.float32)
        y, ldy = _rows(out, 'out')
        arr[i] = FcStripProblem(x.data_ptr(), max(ldx, 512), x.shape[0], sw.img.data_ptr(), sw.D, sw.act, y.data_ptr(), ldy)
        outs.append(out)
    lib, h = _context(dev)
    for i, q in enumerate(problems):
        if q['strip'].mfma != _fc_strip_mfma:
            raise ValueError('problem %d: its image was packed under LAFF_FC_STRIP_MFMA=%d, the context runs %d: pack it again'
                             % (i, q['strip'].mfma, _fc_strip_mfma))
    _call('fc_act_bn', lib.laff_fc_act_bn_strip_grouped, h, arr, n)
    return outs


def _out_buffer(t, shape, device, name):
    """A caller-owned fp32 output of exactly `shape` (contiguous, on `device`), or a fresh one."""
    if t is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _dev(t, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError('%s must be a contiguous fp32 %s tensor on %s, got %s' % (name, tuple(shape), device, tuple(t.shape)))
    return t


def fuse(planes, H, d, w, b, gw, flags, return_weights=False, packed_precision=None, l2norm_planes=False, rank_side=None, out=None,
         weights_out=None, packed_out=None):
    """planes: list of (src[N, ld-view], tile, scale, shift[, act]) -- act ('tanh' | 'relu' | 'sigmoid' | None) is applied to src
    before the affine (a projection that left its activation + BatchNorm to this kernel).  Returns E (N, H, d) [and softmax
    weights (N, H, L)].
    packed_precision ('fp16' | 'bf16'): also emit the similarity operand in the same launch; returned last.
    l2norm_planes: every plane row is first divided by its l2 norm over all H*d columns (`l2norm(local_embs, dim=2)` of the
    expert-embedding branch, model/model.py:1866-1873): one extra launch computes the norms (laff_plane_row_norms).
    out / weights_out / packed_out: caller-owned buffers the launch writes instead of fresh ones -- contiguous fp32 (N, H, d) /
    (N, H, L), and uint8 of at least N * H * d * 2 bytes for the operand."""
    L = len(planes)
    arr = (Plane * L)()
    first = planes[0]
    N = (first[5][0] if (len(first) > 5 and first[5] is not None) else first[0]).shape[0]
    keep = []
    for i, pl in enumerate(planes):
        src, tile, scale, shift = pl[:4]
        act = pl[4] if len(pl) > 4 else None
        gather = pl[5] if len(pl) > 5 else None
        for t in (scale, shift):
            if t is not None:
                _dev(t, 'plane affine')
        sp, tp = (scale.data_ptr() if scale is not None else None), (shift.data_ptr() if shift is not None else None)
        if gather is not None:
            # (csr, weight_t, bias): a sparse feature through its FC, gathered inside the fuse launch
            csr, wt, bias = gather
            if csr.layout != torch.sparse_csr or csr.shape[0] != N:
                raise ValueError('gather plane %d must be a CSR matrix with %d rows' % (i, N))
            wt, ldwt = _rows(wt, 'weight_t')
            if wt.shape[0] != csr.shape[1] or wt.shape[1] != H * d or tile or (flags & ATT_NO_SPLIT_HEAD) or d > 512:
                raise ValueError('gather plane %d: weight_t must be (%d, %d), split heads of d <= 512' % (i, csr.shape[1], H * d))
            crow, col, val = _csr_triple(csr)
            if bias is not None:
                _dev(bias, 'bias')
            arr[i] = Plane(None, 0, 0, sp, tp, ACT[act], crow.data_ptr(), col.data_ptr(), val.data_ptr(), wt.data_ptr(), ldwt,
                           csr.shape[1], bias.data_ptr() if bias is not None else None)
            keep.append((crow, col, val, wt, bias, scale, shift))
            continue
        src, ld = _rows(src, 'plane %d' % i)
        if src.shape[0] != N:
            raise ValueError('plane %d has %d rows, expected %d' % (i, src.shape[0], N))
        need = d if (tile or (flags & ATT_NO_SPLIT_HEAD)) else H * d
        if src.shape[1] != need:
            raise ValueError('plane %d has %d columns, expected %d' % (i, src.shape[1], need))
        arr[i] = Plane(src.data_ptr(), ld, 1 if tile else 0, sp, tp, ACT[act], None, None, None, None, 0, 0, None)
        keep.append((src, scale, shift))
    dev = (first[5][1] if (len(first) > 5 and first[5] is not None) else first[0]).device
    E = _out_buffer(out, (N, H, d), dev, 'out')
    aw = _out_buffer(weights_out, (N, H, L), dev, 'weights_out') if return_weights else None
    for t, nm in ((w, 'w'), (b, 'b'), (gw, 'gw')):
        if t is not None:
            _dev(t, nm)
    lib, h = _context(dev)
    if l2norm_planes:
        norms = torch.empty((L, max(N, 1)), device=dev, dtype=torch.float32)
        _call('plane_row_norms', lib.laff_plane_row_norms, h, arr, L, N, H, d, flags, _ptr(norms))
        for i in range(L):
            arr[i].row_scale = norms[i].data_ptr()
        keep.append(norms)
    packed = None
    if packed_precision is not None:
        prescale = default_prescale(packed_precision)
        if packed_out is None:
            buf = torch.empty((max(N * H * d * 2, 16),), device=dev, dtype=torch.uint8)
        else:
            buf = _dev(packed_out, 'packed_out', torch.uint8)
            if buf.dim() != 1 or not buf.is_contiguous() or buf.numel() < N * H * d * 2:
                raise ValueError('packed_out must be a contiguous uint8 vector of >= %d bytes' % (N * H * d * 2))
        rs = None
        if rank_side is not None:
            # FusedPrepare (below) for this side: laff_rank_prepare's work for these rows rides in this launch
            rs = rank_side.side_struct(N, E)
        _call('fuse', lib.laff_fuse_packed_rank, h, arr, L, N, H, d, _ptr(w), _ptr(b), _ptr(gw), flags, _ptr(E), _ptr(aw), _ptr(buf),
              PREC[packed_precision], prescale, rs)
        packed = Packed(buf, N, H * d, packed_precision, prescale)
        if rank_side is not None:
            rank_side.done(E, packed)
    else:
        _call('fuse', lib.laff_fuse, h, arr, L, N, H, d, _ptr(w), _ptr(b), _ptr(gw), flags, _ptr(E), _ptr(aw))
    out = (E, aw) if return_weights else (E,)
    if packed_precision is not None:
        out = out + (packed,)
    return out if len(out) > 1 else out[0]


def dense_plane(plane, i=0):
    """The source of a plane that the fusion's backward covers: a tensor, or a (src, tile, scale, shift[, act[, gather]]) tuple of
    fuse() that is plain and dense.  Anything else -- tiling, a folded affine, a deferred activation, a gather plane -- belongs to an
    upstream op with its own autograd and is refused by name."""
    if isinstance(plane, torch.Tensor):
        return plane
    src, tile, scale, shift = plane[:4]
    missing = [name for name, on in (('a tiled plane', bool(tile)), ('a folded affine (scale / shift)', scale is not None or shift is not None),
                                     ('a deferred activation', len(plane) > 4 and plane[4] is not None),
                                     ('a gather plane', len(plane) > 5 and plane[5] is not None)) if on]
    if missing:
        raise NotImplementedError('plane %d: the backward of the fusion has no %s; apply it upstream as a torch op, which brings its own '
                                  'autograd' % (i, ' / '.join(missing)))
    return src


def fuse_backward(planes, H, d, w, b, gw, flags, grad_E, want_param_grads=True, out=None):
    """Backward of fuse() over plain dense planes (laff_fuse_backward): planes as fuse() takes them (tensors, or (src, False, None, None)
    tuples; row views with a pitch are read in place), grad_E (N, H, d) or (N, H * d) with any strides.
    Returns (list of dx, dw (H, d), db (H)) -- dw and db are None when want_param_grads is False or the flags say just_average.
    out: a list of L fp32 row views (N, H * d; (N, d) without split heads) that receive the dx, e.g. the slices of a stacked gradient."""
    L = len(planes)
    srcs = [dense_plane(p, i) for i, p in enumerate(planes)]
    N, dev = srcs[0].shape[0], srcs[0].device
    need = d if (flags & ATT_NO_SPLIT_HEAD) else H * d
    rows = []
    for i, s in enumerate(srcs):
        s, ld = _rows(s, 'plane %d' % i)
        if s.shape[0] != N or s.shape[1] != need:
            raise ValueError('plane %d is %s, expected (%d, %d)' % (i, tuple(s.shape), N, need))
        rows.append((s, ld))
    _dev(grad_E, 'grad_E')
    if grad_E.numel() != N * H * d:
        raise ValueError('grad_E has %d elements, expected (%d, %d, %d)' % (grad_E.numel(), N, H, d))
    g = grad_E.reshape(N, H * d)                                      # a view where the strides allow it
    if N and (g.stride(1) != 1 or (N > 1 and g.stride(0) % 4) or g.data_ptr() % 16):
        g = g.contiguous()
    g, lde = _rows(g, 'grad_E')
    if out is None:
        dxs = [torch.empty((N, need), device=dev, dtype=torch.float32) for _ in range(L)]
    else:
        dxs = list(out)
        if len(dxs) != L or any(tuple(t.shape) != (N, need) or t.device != dev for t in dxs):
            raise ValueError('out must hold %d tensors of (%d, %d) on %s' % (L, N, need, dev))
    drows = [_rows(t, 'out %d' % i) for i, t in enumerate(dxs)]
    just_average = bool(flags & ATT_JUST_AVERAGE)
    for t, nm in ((w, 'w'), (b, 'b'), (gw, 'gw')):
        if t is not None:
            _dev(t, nm)
            if not t.is_contiguous():
                raise ValueError('%s must be contiguous' % nm)
    if not just_average and (w is None or b is None or tuple(w.shape) != (H, d) or b.numel() != H):
        raise ValueError('w must be (%d, %d) and b (%d,)' % (H, d, H))
    want = want_param_grads and not just_average
    dw = torch.empty((H, d), device=dev, dtype=torch.float32) if want else None
    db = torch.empty((H,), device=dev, dtype=torch.float32) if want else None
    if N == 0:
        if want:
            dw.zero_()
            db.zero_()
        return dxs, dw, db
    lib, h = _context(dev)
    nbytes = _size_query('laff_fuse_backward_workspace_bytes', L, N, H, d, flags) if want else 0
    ws = _workspace(nbytes, dev, floor=16) if want else None
    xp = (C.c_void_p * L)(*[s.data_ptr() for s, _ in rows])
    xl = (C.c_int * L)(*[ld for _, ld in rows])
    dp = (C.c_void_p * L)(*[t.data_ptr() for t, _ in drows])
    dl = (C.c_int * L)(*[ld for _, ld in drows])
    _call('fuse_backward', lib.laff_fuse_backward, h, xp, xl, L, N, H, d, _ptr(w), _ptr(b), _ptr(gw), flags, _ptr(g), lde, dp, dl,
          _ptr(dw), _ptr(db), _ptr(ws), nbytes)
    return dxs, dw, db


SELFATTN_OUTPUT_TYPES = ('mean', 'max', 'first', 'last', 'second', 'third', 'max_embedding', 'mean_embedding', 'random', 'Attention_1')


def selfattn_mode(output_type, L):
    """(prepend, pool, token) of laff_selfattn_fuse for an output type of Multi_head_MyApply_selfAttention over L planes.  'random' is
    its eval-mode meaning, the mean (model/Attention.py:418-422 of the reference); the caller refuses it in training."""
    K = _lib.K
    none, mean, mx, tok = K['LAFF_SA_PREPEND_NONE'], K['LAFF_SA_POOL_MEAN'], K['LAFF_SA_POOL_MAX'], K['LAFF_SA_POOL_TOKEN']
    table = {'mean': (none, mean, 0), 'random': (none, mean, 0), 'max': (none, mx, 0), 'first': (none, tok, 0),
             'last': (none, tok, L - 1), 'second': (none, tok, 1 if L >= 2 else 0), 'third': (none, tok, 2 if L >= 3 else 0),
             'max_embedding': (K['LAFF_SA_PREPEND_MAX'], tok, 0), 'mean_embedding': (K['LAFF_SA_PREPEND_MEAN'], tok, 0),
             'Attention_1': (none, K['LAFF_SA_POOL_ALL'], 0)}
    if output_type not in table:
        raise NotImplementedError('my_self_attention output type %r is not provided (provided: %s)' %
                                  (output_type, ', '.join(SELFATTN_OUTPUT_TYPES)))
    return table[output_type]


def _selfattn_operands(planes, H, d, gamma, beta):
    """The planes of a self-attention launch as host arrays -- (N, device, tensors kept alive, pointers, pitches) -- and gamma / beta
    checked.  A plane whose rows are not 16-byte aligned is copied."""
    srcs = [dense_plane(p, i) for i, p in enumerate(planes)]
    N = srcs[0].shape[0]
    kept, ptrs, lds = _plane_arrays(srcs, 'planes', N, H * d)
    _vec(gamma, d, 'gamma')
    _vec(beta, d, 'beta')
    return N, kept[0].device, kept, ptrs, lds


def selfattn_fuse(planes, H, d, gamma, beta, output_type, l2norm_each_head=False, out=None):
    """The multi-head self-attention fusion block (laff_selfattn_fuse) over L plain dense fp32 planes (N, H * d) -- tensors or
    (src, False, None, None) tuples; row views with 16-byte aligned rows are read in place --, gamma / beta (d,) the LayerNorm shared by
    all heads.  Returns E (N, H, d), or for 'Attention_1' the stacked tokens (N, L, H * d).  out: the buffer that receives them
    (pitches allowed)."""
    L = len(planes)
    prepend, pool, token = selfattn_mode(output_type, L)
    N, dev, kept, ptrs, lds = _selfattn_operands(planes, H, d, gamma, beta)
    flags = ATT_L2NORM_EACH_HEAD if l2norm_each_head else 0
    lib, h = _context(dev)
    if pool == _lib.K['LAFF_SA_POOL_ALL']:
        O = torch.empty((N, L, H * d), device=dev, dtype=torch.float32) if out is None else out
        O, ldn, ldl = _stacked3(O, N, L, H * d, 'out')
        _call('selfattn_fuse', lib.laff_selfattn_fuse, h, ptrs, lds, L, N, H, d, _ptr(gamma), _ptr(beta), prepend, pool, token, flags,
              None, 0, _ptr(O), ldn, ldl)
        return O
    E = torch.empty((N, H, d), device=dev, dtype=torch.float32) if out is None else out
    E2, lde = _rows(E.view(N, H * d), 'out')
    _call('selfattn_fuse', lib.laff_selfattn_fuse, h, ptrs, lds, L, N, H, d, _ptr(gamma), _ptr(beta), prepend, pool, token, flags,
          _ptr(E2), (lde + 3) // 4 * 4 if N <= 1 else lde, None, 0, 0)
    return E


def selfattn_fuse_backward_plan(N, H, d):
    """laff_selfattn_fuse_backward_plan (host only): (workspace bytes when dgamma / dbeta are asked, partial rows = blocks)."""
    return _plan_query('laff_selfattn_fuse_backward_plan', 2, N, H, d)


def selfattn_fuse_backward(planes, H, d, gamma, beta, output_type, l2norm_each_head, grad, want_param_grads=True, out=None):
    """Backward of selfattn_fuse (laff_selfattn_fuse_backward): the forward's planes and parameters, grad = the gradient of E ((N, H, d)
    or (N, H * d), any strides) or, for 'Attention_1', of the stacked tokens (N, L, H * d) (read in place when its rows are 16-byte
    aligned).  Returns (list of L dx (N, H * d), dgamma (d,), dbeta (d,)) -- the last two None unless want_param_grads.
    out: a list of L fp32 row views (N, H * d) with 16-byte aligned rows that receive the dx, e.g. the slices of a stacked gradient."""
    L = len(planes)
    prepend, pool, token = selfattn_mode(output_type, L)
    N, dev, kept, ptrs, lds = _selfattn_operands(planes, H, d, gamma, beta)
    D = H * d
    flags = ATT_L2NORM_EACH_HEAD if l2norm_each_head else 0
    _dev(grad, 'grad')
    gE = gO = None
    lde = ldn = ldl = 0
    if pool == _lib.K['LAFF_SA_POOL_ALL']:
        g = grad
        if g.dim() == 3 and g.numel() and (g.stride(2) != 1 or g.stride(0) % 4 or g.stride(1) % 4 or g.data_ptr() % 16 or
                                           (N > 1 and g.stride(0) < D) or (L > 1 and g.stride(1) < D)):
            g = g.contiguous()
        gO, ldn, ldl = _stacked3(g, N, L, D, 'grad')
    else:
        if grad.numel() != N * D:
            raise ValueError('grad has %d elements, expected (%d, %d, %d)' % (grad.numel(), N, H, d))
        gE, lde = _mat(grad.reshape(N, D), 'grad', align16=True)
        if N <= 1:
            lde = (lde + 3) // 4 * 4
    dxs = [torch.empty((N, D), device=dev, dtype=torch.float32) for _ in range(L)] if out is None else list(out)
    if len(dxs) != L:
        raise ValueError('out must hold %d tensors' % L)
    dkept, dptrs, dlds = _plane_arrays(dxs, 'out', N, D)
    if any(a is not b for a, b in zip(dkept, dxs)):
        raise ValueError('out must be row views with 16-byte aligned rows')
    dgamma = torch.empty((d,), device=dev, dtype=torch.float32) if want_param_grads else None
    dbeta = torch.empty((d,), device=dev, dtype=torch.float32) if want_param_grads else None
    nbytes = selfattn_fuse_backward_plan(N, H, d)[0] if want_param_grads else 0
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('selfattn_fuse_backward', lib.laff_selfattn_fuse_backward, h, ptrs, lds, L, N, H, d, _ptr(gamma), _ptr(beta), prepend, pool, token,
          flags, _ptr(gE), lde, _ptr(gO), ldn, ldl, dptrs, dlds, _ptr(dgamma), _ptr(dbeta), _ptr(ws), nbytes)
    return dxs, dgamma, dbeta


def fc_backward_plan(N, Dk, D, want_dx=True, want_dw=True):
    """laff_fc_backward_plan (host only): (chunks of dW's and db's sum over N, workspace bytes for the wanted outputs -- db's always
    counted --, chunks of dX's sum over D, tile variants: bit 0 dW and bit 1 dX on 128 x 128 tiles, else 64 x 64)."""
    return _plan_query('laff_fc_backward_plan', 4, N, Dk, D, bool(want_dx), bool(want_dw))


def fc_backward(x, weight, a, grad_a, activation, want_dx=True, want_dw=True, want_db=True, out=None):
    """Backward of a = act(x @ weight.T + bias) (laff_fc_backward): x (N, Dk), weight (D, Dk), a (N, D) the saved forward output,
    grad_a (N, D) its gradient; device fp32, row views with a pitch are read in place, a non-unit inner stride is made dense first.
    Returns (dx (N, Dk) | None, dw (D, Dk) | None, db (D,) | None).  out: a (dx, dw, db) triple of fp32 buffers (None entries are
    allocated here; dx and dw may be row views with a pitch, db is contiguous) that receive the wanted outputs."""
    if activation not in ACT:
        raise ValueError('unknown activation %r' % (activation,))
    (x, ldx), (w, ldw), (a, lda), (g, ldg) = [_mat(t, nm) for t, nm in ((x, 'x'), (weight, 'weight'), (a, 'a'), (grad_a, 'grad_a'))]
    (N, Dk), D, dev = x.shape, w.shape[0], x.device
    if w.shape[1] != Dk or tuple(a.shape) != (N, D) or tuple(g.shape) != (N, D):
        raise ValueError('x %s, weight %s, a %s and grad_a %s do not fit together' % (tuple(x.shape), tuple(w.shape), tuple(a.shape),
                                                                                    tuple(g.shape)))
    odx, odw, odb = out if out is not None else (None, None, None)
    dx, pdx, lddx = _out_rows(odx, (N, Dk), dev, 'out dx') if want_dx else (None, None, 0)
    dw, pdw, lddw = _out_rows(odw, (D, Dk), dev, 'out dw') if want_dw else (None, None, 0)
    db = _vec_out(odb, D, dev, 'out db') if want_db else None
    if not (want_dx or want_dw or want_db):
        return None, None, None
    nbytes = fc_backward_plan(N, Dk, D, want_dx, want_dw)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('fc_backward', lib.laff_fc_backward, h, _ptr(x), N, Dk, ldx, _ptr(w), ldw, D, ACT[activation], _ptr(a), lda, _ptr(g), ldg,
          pdx, lddx, pdw, lddw, _ptr(db), _ptr(ws), nbytes)
    return dx, dw, db


def csr_transpose(x_csr):
    """The pattern of a torch.sparse_csr matrix (N, Dk) transposed, as laff_fc_gather_backward reads it: (colptr [Dk + 1] int32,
    rows [nnz] int32, values [nnz] fp32) on the CSR's device.  Column v owns the entries [colptr[v], colptr[v + 1]), in the order the
    CSR holds them (ascending row; a word that a row names twice stays twice).  The entries are sorted by column id with a stable sort
    and colptr is searchsorted(sorted ids, arange(Dk + 1)): ids outside [0, Dk) stay in rows / values but lie in front of colptr[0] or
    behind colptr[Dk], in no column's range -- dropped, as the forward ignores them, without a data-dependent size.  A host CSR is
    transposed with numpy, a device CSR with torch ops and no host synchronisation."""
    if x_csr.layout != torch.sparse_csr or x_csr.dim() != 2:
        raise ValueError('x_csr must be a 2-D torch.sparse_csr tensor')
    N, Dk = x_csr.shape
    crow, col, val = x_csr.crow_indices(), x_csr.col_indices(), x_csr.values()
    nnz = col.numel()
    if not x_csr.is_cuda:
        col = col.numpy().astype(np.int64)
        row = np.repeat(np.arange(N, dtype=np.int32), np.diff(crow.numpy().astype(np.int64)))
        order = np.argsort(col, kind='stable')
        colptr = np.searchsorted(col[order], np.arange(Dk + 1), side='left').astype(np.int32)
        return (torch.from_numpy(colptr), torch.from_numpy(row[order]),
                torch.from_numpy(np.ascontiguousarray(val.numpy().astype(np.float32)[order])))
    dev = col.device
    # the row of entry j: the last r with crow[r] <= j
    row = torch.searchsorted(crow.to(torch.int64), torch.arange(nnz, device=dev), right=True) - 1
    scol, order = torch.sort(col.to(torch.int64), stable=True)
    colptr = torch.searchsorted(scol, torch.arange(Dk + 1, device=dev), right=False).to(torch.int32)
    return colptr, row[order].to(torch.int32), val.to(torch.float32)[order].contiguous()


def fc_gather_backward(csc, N, Dk, a, grad_a, activation, want_dw=True, want_db=True, out=None):
    """Backward of a = act(x @ weight.T + bias) for a sparse x (N, Dk) (laff_fc_gather_backward): csc = (colptr, rows, values) as
    csr_transpose returns them (values may be None: all ones), a (N, D) the saved forward output, grad_a (N, D) its gradient; device
    fp32, row views whose rows are 16-byte aligned (base and pitch) are read in place, anything else is made dense first.
    Returns (dw (D, Dk) | None, db (D,) | None); dw is in weight's own layout.  out: a (dw, db) pair of fp32 buffers (None entries are
    allocated here; dw may be a row view with any pitch and any 4-byte aligned base, e.g. a column window of a wider gradient -- every
    element of the window is written and nothing else; db is contiguous)."""
    if activation not in ACT:
        raise ValueError('unknown activation %r' % (activation,))
    N, Dk = int(N), int(Dk)
    colptr, rows, values, nnz = _csc_triple(csc, Dk=Dk)
    (a, lda), (g, ldg) = _mat(a, 'a', align16=True), _mat(grad_a, 'grad_a', align16=True)
    D, dev = a.shape[1], a.device
    lda, ldg = (lda + 3) // 4 * 4, (ldg + 3) // 4 * 4          # a single row: no pitch of its own
    if a.shape[0] != N or tuple(g.shape) != (N, D):
        raise ValueError('a %s and grad_a %s do not fit N = %d' % (tuple(a.shape), tuple(g.shape), N))
    odw, odb = out if out is not None else (None, None)
    dw, pdw, lddw = _out_rows(odw, (D, Dk), dev, 'out dw') if want_dw else (None, None, 0)
    db = _vec_out(odb, D, dev, 'out db') if want_db else None
    if not (want_dw or want_db):
        return None, None
    lib, h = _context(dev)
    _call('fc_gather_backward', lib.laff_fc_gather_backward, h, _ptr(colptr), _ptr(rows), _ptr(values), nnz, N, Dk, D, ACT[activation],
          _ptr(a), lda, _ptr(g), ldg, pdw, lddw, _ptr(db))
    return dw, db


def _concat_kinds(segments, want_dx):
    """(widths, kinds) of a concat layer's segments as laff_fc_concat_backward_plan takes them: a segment is a dense (N, Dk) matrix (or
    just its width, for a plan) or a transposed pattern (colptr, rows, values); kinds = bit 0 CSR | bit 1 dX wanted."""
    want_dx = list(want_dx) if want_dx is not None else [False] * len(segments)
    if len(want_dx) != len(segments):
        raise ValueError('want_dx has %d entries for %d segments' % (len(want_dx), len(segments)))
    widths, kinds = [], []
    for j, (x, wdx) in enumerate(zip(segments, want_dx)):
        csr = isinstance(x, (tuple, list))
        if csr and wdx:
            raise ValueError('segment %d is sparse (counts): it has no dx' % j)
        widths.append(x[0].numel() - 1 if csr else int(x) if isinstance(x, int) else x.shape[1])
        kinds.append((1 if csr else 0) | (2 if wdx else 0))
    return widths, kinds, want_dx


def fc_concat_backward_plan(N, D, segments, want_dx=None, want_dw=True):
    """laff_fc_concat_backward_plan (host only): (chunks of dW's and db's sum over N, workspace bytes, chunks of dX's sum over D, tile
    variants: bit 0 dW and bit 1 dX on 128 x 128 tiles).  segments: as fc_concat_backward takes them, a dense one also as its width."""
    widths, kinds, _ = _concat_kinds(segments, want_dx)
    n = len(widths)
    out = (C.c_int * 4)()
    check(_lib.load().laff_fc_concat_backward_plan(int(N), int(D), (C.c_int * n)(*widths), (C.c_int * n)(*kinds), n, bool(want_dw), out))
    return tuple(out)


def fc_concat_backward(segments, weight, a, grad_a, activation, want_dx=None, want_dw=True, want_db=True, out=None, columns=None):
    """Backward of a = act(cat(segments, dim 1) @ weight.T + bias) without the concatenation (laff_fc_concat_backward): one launch
    writes the column windows of ONE (D, K) dw for all dense segments (and db), one launch the dx of every dense segment that wants
    one, and each sparse segment's window is one laff_fc_gather_backward launch.  segments: dense (N, Dk) device fp32 matrices (row
    views with a pitch are read in place) and / or transposed patterns (colptr, rows, values) as csr_transpose returns them, in the
    order their columns have in weight (D, K); a (N, D) the saved forward output, grad_a (N, D) its gradient.  want_dx: one flag per
    segment (default: none).  columns: the first column of every segment's window in weight where the windows do not simply follow
    each other (they may then leave columns of weight out: those columns of dw are not written).
    Returns (dxs -- a list with None where no dx was asked for --, dw (D, K) | None, db (D,) | None).
    out: a (dxs, dw, db) triple of fp32 buffers; dxs a list (None entries are allocated here), dw may be a row view with a pitch."""
    if activation not in ACT:
        raise ValueError('unknown activation %r' % (activation,))
    segments = list(segments)
    widths, kinds, want_dx = _concat_kinds(segments, want_dx)
    sparse = any(k & 1 for k in kinds)
    (w, ldw) = _mat(weight, 'weight')
    (a, lda), (g, ldg) = _mat(a, 'a', align16=sparse), _mat(grad_a, 'grad_a', align16=sparse)
    (N, D), K, dev = a.shape, w.shape[1], a.device
    if sparse:
        lda, ldg = (lda + 3) // 4 * 4, (ldg + 3) // 4 * 4      # a single row: no pitch of its own
    free = columns is not None
    if not free:
        columns = [sum(widths[:j]) for j in range(len(widths))]
    if len(columns) != len(widths):
        raise ValueError('columns has %d entries for %d segments' % (len(columns), len(widths)))
    if w.shape[0] != D or tuple(g.shape) != (N, D) or (
            max(c + k for c, k in zip(columns, widths)) > K if free else sum(widths) != K):
        raise ValueError('weight %s, a %s, grad_a %s and segments of %d columns do not fit together' % (
            tuple(w.shape), tuple(a.shape), tuple(g.shape), sum(widths)))
    odx, odw, odb = out if out is not None else (None, None, None)
    odx = list(odx) if odx is not None else [None] * len(segments)
    dw, pdw, lddw = _out_rows(odw, (D, K), dev, 'out dw') if want_dw else (None, None, 0)
    db = _vec_out(odb, D, dev, 'out db') if want_db else None
    n = len(segments)
    ints = {k: (C.c_int * n)() for k in ('cols', 'nnz', 'ldx', 'lddx')}
    ptrs = {k: (C.c_void_p * n)() for k in ('x', 'dx', 'colptr', 'rows', 'values')}
    dxs, keep = [], []
    for j, x in enumerate(segments):
        ints['cols'][j], ints['nnz'][j] = int(columns[j]), -1
        if kinds[j] & 1:
            colptr, rows, values, ints['nnz'][j] = _csc_triple(x, 'segment %d: ' % j)
            ptrs['colptr'][j], ptrs['rows'][j] = colptr.data_ptr(), rows.data_ptr()
            ptrs['values'][j] = values.data_ptr() if values is not None else None
            dxs.append(None)
        else:
            x, ints['ldx'][j] = _mat(x, 'segment %d' % j)
            if x.shape[0] != N:
                raise ValueError('segment %d is %s, expected %d rows' % (j, tuple(x.shape), N))
            dx, _, ints['lddx'][j] = _out_rows(odx[j], (N, widths[j]), dev, 'out dx %d' % j) if want_dx[j] else (None, None, 0)
            ptrs['x'][j], ptrs['dx'][j] = x.data_ptr(), dx.data_ptr() if dx is not None else None
            keep.append(x)
            dxs.append(dx)
    if not (any(want_dx) or want_dw or want_db):
        return dxs, None, None
    nbytes = fc_concat_backward_plan(N, D, segments, want_dx, want_dw)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('fc_concat_backward', lib.laff_fc_concat_backward, h, n, (C.c_int * n)(*widths), ints['cols'], ints['nnz'], ptrs['x'], ints['ldx'],
          ptrs['dx'], ints['lddx'], ptrs['colptr'], ptrs['rows'], ptrs['values'], N, _ptr(w), K, ldw, D, ACT[activation], _ptr(a), lda,
          _ptr(g), ldg, pdw, lddw, _ptr(db), _ptr(ws), nbytes)
    return dxs, dw, db


def dropout_bn_train_plan(N, D, has_bn=True):
    """laff_dropout_bn_train_plan (host only): (row chunks of the column sums -- 1 without a BatchNorm stage --, workspace bytes,
    launches per direction, rows of a chunk)."""
    return _plan_query('laff_dropout_bn_train_plan', 4, N, D, bool(has_bn))


def _bn_fwd_out(out, shape, width, dev, has_bn=True):
    """((y, its pointer, its pitch), save_mean, save_invstd) from `out`, a y buffer or a triple; the statistics are (width,) or None."""
    oy, omean, oinv = out if isinstance(out, (tuple, list)) else (out, None, None)
    y = _out_rows(oy, shape, dev, 'out y')
    if not has_bn:
        return y, None, None
    return y, _vec_out(omean, width, dev, 'out save_mean'), _vec_out(oinv, width, dev, 'out save_invstd')


def _bn_bwd_out(out, shape, width, dev, name, want_dx, want_dgamma, want_dbeta):
    """((d_input, its pointer, its pitch), dgamma, dbeta) from `out`, a triple or None; the last two are (width,), the unwanted None."""
    odx, odg, odb = out if out is not None else (None, None, None)
    dx = _out_rows(odx, shape, dev, 'out ' + name) if want_dx else (None, None, 0)
    dgamma = _vec_out(odg, width, dev, 'out dgamma') if want_dgamma else None
    dbeta = _vec_out(odb, width, dev, 'out dbeta') if want_dbeta else None
    return dx, dgamma, dbeta


def _bn_seed(p, seed):
    p = float(p)
    if p > 0.0:
        _dev(seed, 'seed', torch.int64)
        if seed.numel() != 1:
            raise ValueError('seed must hold one int64, got shape %s' % (tuple(seed.shape),))
    return p, (seed if p > 0.0 else None)


def dropout_bn_train(a, p, seed, weight, bias, running_mean, running_var, momentum, eps, out=None):
    """Dropout by the counter-based mask of laff_dropout_bn_train, then training-mode BatchNorm1d: a (N, D) device fp32 (a row view with
    a pitch is read in place), p in [0, 1), seed a device int64 tensor of one element (None allowed with p == 0), weight / bias /
    running_mean / running_var (D,) contiguous device fp32 -- the running statistics are UPDATED IN PLACE through raw pointers (their
    version counters are the caller's to bump).  weight None: no BatchNorm stage, y = a (.) mask / (1 - p), the other vectors are
    ignored.  Returns (y, save_mean, save_invstd), the last two None without a BatchNorm stage.  out: a y buffer, or a
    (y, save_mean, save_invstd) triple of buffers (None entries are allocated here; y may be a row view with a pitch)."""
    a, lda = _mat(a, 'a')
    (N, D), dev = a.shape, a.device
    p, seed = _bn_seed(p, seed)
    if weight is not None:
        weight, bias = _vec(weight, D, 'weight'), _vec(bias, D, 'bias')
        running_mean, running_var = _vec(running_mean, D, 'running_mean'), _vec(running_var, D, 'running_var')
    else:
        bias = running_mean = running_var = None
    (y, py, ldy), mean, invstd = _bn_fwd_out(out, (N, D), D, dev, weight is not None)
    nbytes = dropout_bn_train_plan(N, D, weight is not None)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('dropout_bn_train', lib.laff_dropout_bn_train, h, _ptr(a), N, D, lda, p, _ptr(seed), _ptr(weight), _ptr(bias), _ptr(running_mean),
          _ptr(running_var), float(momentum), float(eps), py, ldy, _ptr(mean), _ptr(invstd), _ptr(ws), nbytes)
    return y, mean, invstd


def dropout_bn_train_backward(grad_y, a, p, seed, weight, save_mean, save_invstd, want_da=True, want_dgamma=True, want_dbeta=True, out=None):
    """Backward of dropout_bn_train (laff_dropout_bn_train_backward): grad_y and a (N, D) device fp32, p and seed as the forward had them
    (the mask is recomputed), weight and the forward's save_mean / save_invstd (None, None, None: no BatchNorm stage, and then no
    dgamma / dbeta).  Returns (da | None, dgamma | None, dbeta | None).  out: a (da, dgamma, dbeta) triple of buffers (None entries
    are allocated here; da may be a row view with a pitch)."""
    g, ldg = _mat(grad_y, 'grad_y')
    a, lda = _mat(a, 'a')
    (N, D), dev = a.shape, a.device
    if tuple(g.shape) != (N, D):
        raise ValueError('grad_y %s and a %s do not fit together' % (tuple(g.shape), tuple(a.shape)))
    p, seed = _bn_seed(p, seed)
    if weight is not None:
        weight, save_mean = _vec(weight, D, 'weight'), _vec(save_mean, D, 'save_mean')
        save_invstd = _vec(save_invstd, D, 'save_invstd')
    else:
        save_mean = save_invstd = None
        if want_dgamma or want_dbeta:
            raise ValueError('dgamma / dbeta are wanted, but there is no BatchNorm stage (weight is None)')
    (da, pda, ldda), dgamma, dbeta = _bn_bwd_out(out, (N, D), D, dev, 'da', want_da, want_dgamma, want_dbeta)
    if not (want_da or want_dgamma or want_dbeta):
        return None, None, None
    nbytes = dropout_bn_train_plan(N, D, weight is not None)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('dropout_bn_train_backward', lib.laff_dropout_bn_train_backward, h, _ptr(g), ldg, _ptr(a), N, D, lda, p, _ptr(seed), _ptr(weight),
          _ptr(save_mean), _ptr(save_invstd), pda, ldda, _ptr(dgamma), _ptr(dbeta), _ptr(ws), nbytes)
    return da, dgamma, dbeta


def tile_bn_train_plan(N, C_in, H):
    """laff_tile_bn_train_plan (host only) for N rows of C_in columns tiled over H heads: (row chunks of the column sums, workspace bytes
    of either direction, launches per direction, rows of a chunk)."""
    return _plan_query('laff_tile_bn_train_plan', 4, N, C_in, H)


def tile_bn_train(x, heads, weight, bias, running_mean, running_var, momentum, eps, out=None):
    """Training-mode BatchNorm1d(heads * W) over x.repeat(1, heads) on laff_tile_bn_train, the tiled input never formed: x (N, W) device
    fp32 (a row view with a pitch is read in place), weight / bias / running_mean / running_var (heads * W,) contiguous device fp32 --
    the running statistics are UPDATED IN PLACE through raw pointers (their version counters are the caller's to bump).  Returns
    (y (N, heads * W), save_mean (W,), save_invstd (W,)): the statistics are per input column.  out: a y buffer, or a
    (y, save_mean, save_invstd) triple of buffers (None entries are allocated here; y may be a row view with a pitch)."""
    x, ldx = _mat(x, 'x')
    (N, W), dev, H = x.shape, x.device, int(heads)
    weight, bias = _vec(weight, H * W, 'weight'), _vec(bias, H * W, 'bias')
    running_mean, running_var = _vec(running_mean, H * W, 'running_mean'), _vec(running_var, H * W, 'running_var')
    (y, py, ldy), mean, invstd = _bn_fwd_out(out, (N, H * W), W, dev)
    nbytes = tile_bn_train_plan(N, W, H)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('tile_bn_train', lib.laff_tile_bn_train, h, _ptr(x), N, W, ldx, H, _ptr(weight), _ptr(bias), _ptr(running_mean),
          _ptr(running_var), float(momentum), float(eps), py, ldy, _ptr(mean), _ptr(invstd), _ptr(ws), nbytes)
    return y, mean, invstd


def tile_bn_train_backward(grad_y, x, heads, weight, save_mean, save_invstd, want_dx=True, want_dgamma=True, want_dbeta=True, out=None):
    """Backward of tile_bn_train (laff_tile_bn_train_backward): grad_y (N, heads * W) and x (N, W) device fp32, weight and the forward's
    save_mean / save_invstd.  Returns (dx (N, W) | None -- the heads' contributions summed in ascending order --, dgamma | None,
    dbeta | None, both (heads * W,)).  out: a (dx, dgamma, dbeta) triple of buffers (None entries are allocated here; dx may be a row
    view with a pitch)."""
    g, ldg = _mat(grad_y, 'grad_y')
    x, ldx = _mat(x, 'x')
    (N, W), dev, H = x.shape, x.device, int(heads)
    if tuple(g.shape) != (N, H * W):
        raise ValueError('grad_y %s does not fit x %s tiled over %d heads' % (tuple(g.shape), tuple(x.shape), H))
    weight, save_mean, save_invstd = _vec(weight, H * W, 'weight'), _vec(save_mean, W, 'save_mean'), _vec(save_invstd, W, 'save_invstd')
    (dx, pdx, lddx), dgamma, dbeta = _bn_bwd_out(out, (N, W), H * W, dev, 'dx', want_dx, want_dgamma, want_dbeta)
    if not (want_dx or want_dgamma or want_dbeta):
        return None, None, None
    nbytes = tile_bn_train_plan(N, W, H)[1]
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('tile_bn_train_backward', lib.laff_tile_bn_train_backward, h, _ptr(g), ldg, _ptr(x), N, W, ldx, H, _ptr(weight), _ptr(save_mean),
          _ptr(save_invstd), pdx, lddx, _ptr(dgamma), _ptr(dbeta), _ptr(ws), nbytes)
    return dx, dgamma, dbeta


def expert_stage_train_plan(N, L, D):
    """laff_expert_stage_train_plan (host only) for L planes of N rows and D columns: (blocks of the backward launch per plane -- one
    partial column sum of d_expert each --, workspace bytes of the backward when d_expert is asked)."""
    return _plan_query('laff_expert_stage_train_plan', 2, N, L, D)


def _stacked3(t, N, L, D, name):
    """An (N, L, D) device fp32 tensor as the expert stage addresses it: (tensor, row pitch, plane pitch).  Unit inner stride, 16-byte
    aligned rows; anything else is refused (an output) -- the callers make their inputs so."""
    _dev(t, name)
    if tuple(t.shape) != (N, L, D):
        raise ValueError('%s must be (%d, %d, %d), got %s' % (name, N, L, D, tuple(t.shape)))
    if t.numel() and (t.stride(2) != 1 or t.stride(0) % 4 or t.stride(1) % 4 or t.data_ptr() % 16):
        raise ValueError('%s must have unit inner stride and 16-byte aligned rows, got strides %s' % (name, t.stride()))
    ldn = t.stride(0) if N > 1 else max(t.stride(0), (L - 1) * max(t.stride(1), D) + D)
    ldl = t.stride(1) if L > 1 else max(t.stride(1), D)
    return t, ldn, ldl


def _plane_arrays(planes, name, N, D):
    """L (N, D) device fp32 row views as the host arrays of the expert stage: (tensors kept alive, pointer array, pitch array).  A plane
    whose rows are not 16-byte aligned is made dense first."""
    kept, L = [], len(planes)
    ptrs, lds = (C.c_void_p * L)(), (C.c_int * L)()
    for l, t in enumerate(planes):
        t, ld = _mat(t, '%s[%d]' % (name, l), align16=True)
        if tuple(t.shape) != (N, D):
            raise ValueError('%s[%d] must be (%d, %d), got %s' % (name, l, N, D, tuple(t.shape)))
        kept.append(t)
        ptrs[l], lds[l] = t.data_ptr(), (ld + 3) // 4 * 4 if t.shape[0] <= 1 else ld
    return kept, ptrs, lds


def expert_stage_train(planes, expert, l2norm, out=None):
    """The expert stage of a tower in training mode on laff_expert_stage_train, one launch for all planes: planes L device fp32 (N, D)
    matrices (row views with 16-byte aligned rows are read in place), expert (L, D) device fp32 or None, added row l to plane l; with
    l2norm every row of every plane is then divided by its norm over all D columns (+ 1e-13 + 1e-14).  Returns (stacked (N, L, D),
    rnorm (L, N) or None without l2norm).  out: a (stacked, rnorm) pair of buffers (None entries are allocated here; stacked may have
    pitches)."""
    L = len(planes)
    N, D = planes[0].shape
    kept, ptrs, lds = _plane_arrays(planes, 'planes', N, D)
    dev = kept[0].device
    if expert is not None:
        expert, lde = _mat(expert, 'expert', align16=True)
        if tuple(expert.shape) != (L, D):
            raise ValueError('expert must be (%d, %d), got %s' % (L, D, tuple(expert.shape)))
    else:
        lde = 0
    oy, orn = out if out is not None else (None, None)
    if oy is None:
        oy = torch.empty((N, L, D), device=dev, dtype=torch.float32)
    oy, ldn, ldl = _stacked3(oy, N, L, D, 'out stacked')
    rnorm = None
    if l2norm:
        rnorm = torch.empty((L, N), device=dev, dtype=torch.float32) if orn is None else _dev(orn, 'out rnorm')
        if tuple(rnorm.shape) != (L, N) or not rnorm.is_contiguous():
            raise ValueError('out rnorm must be a contiguous (%d, %d), got %s' % (L, N, tuple(rnorm.shape)))
    lib, h = _context(dev)
    _call('expert_stage_train', lib.laff_expert_stage_train, h, ptrs, lds, N, L, D, _ptr(expert), lde, int(bool(l2norm)), _ptr(oy), ldn, ldl,
          _ptr(rnorm))
    return oy, rnorm


def expert_stage_train_backward(grad_stacked, planes, expert, l2norm, rnorm, want_d_expert=True, out=None):
    """Backward of expert_stage_train (laff_expert_stage_train_backward): grad_stacked (N, L, D) device fp32 (read in place when its
    rows are 16-byte aligned), the forward's planes, expert and rnorm.  Returns (list of L dx (N, D), d_expert (L, D) | None).
    out: a (list of dx buffers or None, d_expert buffer or None) pair."""
    L = len(planes)
    N, D = planes[0].shape
    kept, ptrs, lds = _plane_arrays(planes, 'planes', N, D)
    dev = kept[0].device
    g = _dev(grad_stacked, 'grad_stacked')
    if g.dim() == 3 and g.numel() and (g.stride(2) != 1 or g.stride(0) % 4 or g.stride(1) % 4 or g.data_ptr() % 16 or
                                       (N > 1 and g.stride(0) < D) or (L > 1 and g.stride(1) < D)):
        g = g.contiguous()
    g, ldn, ldl = _stacked3(g, N, L, D, 'grad_stacked')
    if expert is not None:
        expert, lde = _mat(expert, 'expert', align16=True)
    else:
        lde = 0
    odx, ode = out if out is not None else (None, None)
    dxs = [torch.empty((N, D), device=dev, dtype=torch.float32) for _ in range(L)] if odx is None else list(odx)
    dkept, dptrs, dlds = _plane_arrays(dxs, 'out dx', N, D)
    if any(a is not b for a, b in zip(dkept, dxs)):
        raise ValueError('out dx must be row views with 16-byte aligned rows')
    d_expert = None
    if want_d_expert:
        if expert is None:
            raise ValueError('d_expert was asked without an expert table')
        d_expert = torch.empty((L, D), device=dev, dtype=torch.float32) if ode is None else _dev(ode, 'out d_expert')
        if tuple(d_expert.shape) != (L, D) or not d_expert.is_contiguous():
            raise ValueError('out d_expert must be a contiguous (%d, %d), got %s' % (L, D, tuple(d_expert.shape)))
    nbytes = expert_stage_train_plan(N, L, D)[1] if want_d_expert else 0
    ws = _workspace(nbytes, dev)
    lib, h = _context(dev)
    _call('expert_stage_train_backward', lib.laff_expert_stage_train_backward, h, _ptr(g), ldn, ldl, ptrs, lds, N, L, D, _ptr(expert), lde,
          int(bool(l2norm)), _ptr(rnorm), dptrs, dlds, _ptr(d_expert), _ptr(ws), nbytes)
    return dxs, d_expert


def optim_plan(sizes):
    """laff_optim_plan (host only) for a tensor list with these element counts: (elements of a chunk, tensors of one launch's table,
    norm launches, partials -- the workspace of grad_sqnorm holds 8 bytes each --, update launches, blocks a launch has at most)."""
    sizes = [int(s) for s in sizes]
    out = (C.c_int * 6)()
    check(_lib.load().laff_optim_plan(len(sizes), (C.c_longlong * len(sizes))(*sizes), out))
    return tuple(out)


def optim_last_launches():
    """(launches of the 16-byte variant, launches of the single-float variant) that this thread's last grad_sqnorm / grad_scale /
    optim_step issued."""
    out = (C.c_int * 2)()
    check(_lib.load().laff_optim_last_launches(out))
    return tuple(out)


def _flat_list(tensors, name):
    """A tensor list of the optimizer entry points: device fp32, contiguous, on one device.  Returns (device, element counts)."""
    dev = _dev(tensors[0], '%s[0]' % name).device if tensors else None
    for i, t in enumerate(tensors):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev:
            continue
        _dev(t, '%s[%d]' % (name, i))                      # names what is wrong
        if not t.is_contiguous():
            raise ValueError('%s[%d] must be contiguous, got shape %s strides %s' % (name, i, tuple(t.shape), t.stride()))
        raise ValueError('%s[%d] is on %s, %s[0] on %s' % (name, i, t.device, name, dev))
    return dev, [t.numel() for t in tensors]


def grad_sqnorm(grads, workspace=None):
    """laff_grad_sqnorm: float64 partial sums of g*g over the list into `workspace` (a uint8 device buffer of 8 bytes a partial,
    allocated here when None).  Returns (workspace, partials) for grad_scale / optim_step."""
    grads = list(grads)
    dev, sizes = _flat_list(grads, 'grads')
    partials = optim_plan(sizes)[3]
    if dev is None:
        return workspace, 0
    if workspace is None:
        workspace = torch.empty(max(8 * partials, 16), dtype=torch.uint8, device=dev)
    _dev(workspace, 'workspace', torch.uint8)
    lib, h = _context(dev)
    L = len(grads)
    _call('grad_sqnorm', lib.laff_grad_sqnorm, h, L, (C.c_void_p * L)(*[g.data_ptr() for g in grads]), (C.c_longlong * L)(*sizes),
          _ptr(workspace), workspace.numel())
    return workspace, partials


def grad_scale(grads, max_norm, workspace, partials, total_norm_out=None):
    """laff_grad_scale: g *= min(1, max_norm / (total + 1e-6)) in place over the list, total = the L2 norm grad_sqnorm left in
    (workspace, partials).  Returns the total norm, a 0-d fp32 device tensor (total_norm_out when given)."""
    grads = list(grads)
    dev, sizes = _flat_list(grads, 'grads')
    if dev is None:
        raise ValueError('grad_scale of an empty list has no device to answer on')
    if total_norm_out is None:
        total_norm_out = torch.empty((), dtype=torch.float32, device=dev)
    _dev(total_norm_out, 'total_norm_out')
    if workspace is not None:
        _dev(workspace, 'workspace', torch.uint8)
    if int(partials) < 0 or 8 * int(partials) > (workspace.numel() if workspace is not None else 0):
        raise ValueError('workspace holds %d bytes, %d partials need %d' % (workspace.numel() if workspace is not None else 0,
                                                                           partials, 8 * int(partials)))
    lib, h = _context(dev)
    L = len(grads)
    _call('grad_scale', lib.laff_grad_scale, h, L, (C.c_void_p * L)(*[g.data_ptr() for g in grads]), (C.c_longlong * L)(*sizes),
          float(max_norm), _ptr(workspace), int(partials), _ptr(total_norm_out))
    return total_norm_out


def optim_step(kind, params, grads, state1, state2, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0,
               workspace=None, partials=0, total_norm_out=None, checked=False):
    """laff_optim_step over a tensor list: kind 'adam' (state1 = exp_avg, state2 = exp_avg_sq, bias corrections of `step` >= 1) or
    'rmsprop' (state1 = square_avg, beta2 = alpha, state2 = None).  With max_norm > 0 the gradients enter scaled by
    min(1, max_norm / (total + 1e-6)), total from grad_sqnorm's (workspace, partials), and the norm goes to total_norm_out (0-d, optional);
    the gradients themselves are not written.  params and states are updated in place.  checked: the caller has held grads and states
    to what this function checks (device fp32, contiguous, of their parameter's size and device), as laff_amd.optim has."""
    if kind not in _lib.OPT_KIND:
        raise ValueError('unknown optimizer kind %r' % (kind,))
    params, grads, state1 = list(params), list(grads), list(state1)
    adam = kind == 'adam'
    state2 = list(state2) if adam else [None] * len(params)
    if not (len(params) == len(grads) == len(state1) == len(state2)):
        raise ValueError('params, grads and states must have one entry per tensor')
    dev, sizes = _flat_list(params, 'params')
    for nm, ts in () if checked else (('grads', grads), ('state1', state1)) + ((('state2', state2),) if adam else ()):
        d, ns = _flat_list(ts, nm)
        if ns != sizes or d != dev:
            raise ValueError('%s do not match params in size or device' % nm)
    if dev is None:
        return
    clip = float(max_norm) > 0.0
    if clip:
        _dev(workspace, 'workspace', torch.uint8)
        if int(partials) < 0 or 8 * int(partials) > workspace.numel():
            raise ValueError('workspace holds %d bytes, %d partials need %d' % (workspace.numel(), partials, 8 * int(partials)))
        if total_norm_out is not None:
            _dev(total_norm_out, 'total_norm_out')
    L = len(params)
    # laff_optim_tensor is five 8-byte words {p, g, s1, s2, n}: the host array is filled in one constructor call, not L structures
    words = []
    for p, g, a, b, n in zip(params, grads, state1, state2, sizes):
        words += (p.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr() if adam else 0, n)
    table = C.cast((C.c_longlong * (5 * L))(*words), C.POINTER(_lib.OptimTensor))
    hyper = _lib.OptimHyper(_lib.OPT_KIND[kind], float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    lib, h = _context(dev)
    _call('optim_step', lib.laff_optim_step, h, table, L, C.byref(hyper), float(max_norm), _ptr(workspace) if clip else None,
          int(partials) if clip else 0, _ptr(total_norm_out) if clip else None)


def frame_fuse(frames, lens, w, b, gw, flags, out=None):
    """frames (B, Fmax, d) zero padded, lens int32 (B,) or None -> (B, d).  out: a contiguous fp32 (B, d) buffer to write instead."""
    _dev(frames, 'frames')
    if frames.dim() != 3 or not frames.is_contiguous():
        raise ValueError('frames must be contiguous (B, Fmax, d)')
    B, Fmax, d = frames.shape
    if lens is not None:
        _dev(lens, 'lens', torch.int32)
        if lens.numel() != B:
            raise ValueError('lens must have %d entries' % B)
    V = _out_buffer(out, (B, d), frames.device, 'out')
    lib, h = _context(frames.device)
    _call('frame_fuse', lib.laff_frame_fuse, h, _ptr(frames), _ptr(lens), B, Fmax, d, _ptr(_dev(w, 'w')), _ptr(_dev(b, 'b')),
                              _ptr(gw), flags, _ptr(V))
    return V


def frame_fuse_backward_plan(count, B, Fmax, d, want_dw=True):
    """laff_frame_fuse_backward_plan (host only): (workspace bytes, kernel variant -- the 256-column chunks a lane owns: 1 / 2 / 4 for
    d <= 256 / 512 / 1024 --, launches of the main kernel, partial rows of dw per feature)."""
    return _plan_query('laff_frame_fuse_backward_plan', 4, count, B, Fmax, d, bool(want_dw))


def frame_fuse_backward(frames_list, lens, params, flags, grad_list, want_param_grads=True, out=None):
    """Backward of frame_fuse / frame_fuse_grouped (laff_frame_fuse_backward).  frames_list: [(B, Fmax, d)] contiguous, lens int32 (B,)
    or None, params: [(w (d,), b (1,), gw (1,) | None)], grad_list: [(B, d)] the gradients of the outputs (a row pitch that all of
    them share is read in place, anything else is made dense).  Returns (list of dframes (B, Fmax, d), list of dw (d,) | None, list of
    db (1,) | None) -- the last two are None when want_param_grads is False.  Rows at or past a video's length come back as zeros.
    out: one contiguous fp32 (B, Fmax, d) buffer per feature that receives dframes."""
    n = len(frames_list)
    if n == 0 or len(params) != n or len(grad_list) != n or (out is not None and len(out) != n):
        raise ValueError('frames_list, params, grad_list (and out) must hold one entry per frame feature, at least one')
    for fr in frames_list:
        _dev(fr, 'frames')
    if frames_list[0].dim() != 3:
        raise ValueError('frames must be (B, Fmax, d), got shape %s' % (tuple(frames_list[0].shape),))
    B, Fmax, d = frames_list[0].shape
    dev = frames_list[0].device
    for fr in frames_list:
        if tuple(fr.shape) != (B, Fmax, d) or not fr.is_contiguous() or fr.device != dev:
            raise ValueError('the frame features must share one contiguous (B, Fmax, d) shape on one device')
    if lens is not None:
        _dev(lens, 'lens', torch.int32)
        if lens.numel() != B or not lens.is_contiguous():
            raise ValueError('lens must be a contiguous vector of %d entries' % B)
    grads = []
    for g in grad_list:
        _dev(g, 'grad')
        if g.numel() != B * d:
            raise ValueError('a grad has %d elements, expected (%d, %d)' % (g.numel(), B, d))
        grads.append(g.reshape(B, d))
    pitch = {_rows(g, 'grad')[1] if g.numel() and g.stride(1) == 1 else -1 for g in grads}
    if B and (len(pitch) != 1 or min(pitch) < d or min(pitch) % 4 or any(g.data_ptr() % 16 for g in grads)):     # (an expanded grad: 0)
        grads = [g.contiguous() for g in grads]
    lddv = _rows(grads[0], 'grad')[1] if B else d
    for w, b, gw in params:
        for t, nm, k in ((w, 'w', d), (b, 'b', 1)) + (((gw, 'gw', 1),) if gw is not None else ()):
            _dev(t, nm)
            if t.numel() != k or not t.is_contiguous():
                raise ValueError('%s must be a contiguous vector of %d' % (nm, k))
        if gw is None and (flags & ATT_WITH_AVE):
            raise ValueError('with_ave needs gw')
    dfs = [_out_buffer(out[i] if out is not None else None, (B, Fmax, d), dev, 'out[%d]' % i) for i in range(n)]
    dws = [torch.empty((d,), device=dev, dtype=torch.float32) for _ in range(n)] if want_param_grads else None
    dbs = [torch.empty((1,), device=dev, dtype=torch.float32) for _ in range(n)] if want_param_grads else None
    if B == 0:
        for t in (dws or []) + (dbs or []):
            t.zero_()
        return dfs, dws, dbs
    nbytes = frame_fuse_backward_plan(n, B, Fmax, d, want_param_grads)[0]
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev) if want_param_grads else None

    def table(ts):
        return (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    has_gw = all(p[2] is not None for p in params)
    lib, h = _context(dev)
    _call('frame_fuse_backward', lib.laff_frame_fuse_backward, h, n, table(frames_list), _ptr(lens), B, Fmax, d,
          table([p[0] for p in params]), table([p[1] for p in params]), table([p[2] for p in params]) if has_gw else None, flags,
          table(grads), lddv, table(dfs), table(dws) if want_param_grads else None, table(dbs) if want_param_grads else None, _ptr(ws),
          nbytes)
    return dfs, dws, dbs


def frame_fuse_grouped(frames_list, lens, params, flags, mask=None, out=None):
    """frame_fuse for several frame features of the same shape in one launch.  frames_list: [(B, Fmax, d)], params: [(w, b, gw)].
    mask (fp32 (B, >= Fmax) device tensor, rows of ones then zeros: the reference's mask_tensor) replaces lens: the launch sums it.
    out: one contiguous fp32 (B, d) buffer per feature to write instead."""
    n = len(frames_list)
    if out is not None and len(out) != n:
        raise ValueError('out must hold one buffer per frame feature (%d)' % n)
    B, Fmax, d = frames_list[0].shape
    F, W, Bb, G, Vv = ((C.c_void_p * n)() for _ in range(5))
    outs, keep = [], []
    for i, (fr, (w, b, gw)) in enumerate(zip(frames_list, params)):
        _dev(fr, 'frames')
        if tuple(fr.shape) != (B, Fmax, d) or not fr.is_contiguous():
            raise ValueError('grouped frame features must share one contiguous (B, Fmax, d) shape')
        V = _out_buffer(out[i] if out is not None else None, (B, d), fr.device, 'out[%d]' % i)
        F[i], W[i], Bb[i], G[i], Vv[i] = fr.data_ptr(), _dev(w, 'w').data_ptr(), _dev(b, 'b').data_ptr(), _ptr(gw), V.data_ptr()
        outs.append(V)
        keep.append((fr, w, b, gw))
    lib, h = _context(frames_list[0].device)
    if mask is not None:
        _dev(mask, 'mask')
        if mask.dim() != 2 or mask.shape[0] != B or mask.shape[1] < Fmax or mask.stride(1) != 1:
            raise ValueError('mask must be (%d, >= %d) with unit column stride' % (B, Fmax))
        _call('frame_fuse', lib.laff_frame_fuse_grouped_mask, h, n, F, _ptr(mask), mask.stride(0), B, Fmax, d, W, Bb, G, flags, Vv)
        return outs
    if lens is not None:
        _dev(lens, 'lens', torch.int32)
    _call('frame_fuse', lib.laff_frame_fuse_grouped, h, n, F, _ptr(lens), B, Fmax, d, W, Bb, G, flags, Vv)
    return outs


def default_prescale(precision):
    """fp16x3 operands are pre-scaled by 64 (exact) so that the low part of the hi/lo split stays normal.  Single-pass fp16 operands
    are not scaled: the fp16 MFMA honours denormal inputs exactly (tools/debug/denorm_probe.py), an element below 2^-14 of a unit-norm
    row then carries an absolute error of 2^-25 -- that of its normal neighbours -- and the measured band (laff_rank_prepare) covers
    it; with scale == 1 the GEMM epilogue has no product per score to make (sim_strip.hip, SCALE1)."""
    return 64.0 if precision == 'fp16x3' else 1.0


class Packed:
    """GEMM operand produced by pack_rows: raw 16/32-bit buffer + its logical shape and precision."""

    def __init__(self, buf, N, K, precision, prescale):
        self.buf, self.N, self.K, self.precision, self.prescale = buf, N, K, precision, prescale

    def rows(self, a, b):
        """The operand of rows [a, b): a view for one-plane formats, a copy of the two plane slices for the hi/lo split formats
        (their planes are N rows apart)."""
        a, b = max(0, int(a)), min(self.N, int(b))
        esz = 4 if self.precision == 'fp32' else 2
        rb = self.K * esz
        if self.precision in ('fp16x3', 'bf16x3'):
            plane = self.N * rb
            buf = torch.cat([self.buf[a * rb:b * rb], self.buf[plane + a * rb:plane + b * rb]])
        else:
            buf = self.buf[a * rb:b * rb]
        if buf.data_ptr() % 16:
            buf = buf.clone()
        return Packed(buf, b - a, self.K, self.precision, self.prescale)


def pack_rows(E, normalize=True, eps=1e-13, precision='fp16', prescale=None):
    """E (N, H, d) or (N, d): per-(row, head) l2norm (loss.l2norm) then conversion to the GEMM operand format."""
    _dev(E, 'E')
    if E.dim() == 2:
        E = E.unsqueeze(1)
    if E.dim() != 3 or E.stride(2) != 1 or E.stride(1) != E.shape[2]:
        raise ValueError('E must be (N, H, d) with contiguous heads')
    N, H, d = E.shape
    lde = E.stride(0) if N > 1 else H * d
    if prescale is None:
        prescale = default_prescale(precision)
    lib, h = _context(E.device)
    nbytes = C.c_size_t()
    check(lib.laff_packed_bytes(N, H * d, PREC[precision], C.byref(nbytes)))
    buf = torch.empty((max(nbytes.value, 16),), device=E.device, dtype=torch.uint8)
    _call('pack_rows', lib.laff_pack_rows, h, _ptr(E), N, H, d, lde, 1 if normalize else 0, eps, prescale, PREC[precision], _ptr(buf))
    return Packed(buf, N, H * d, precision, prescale)


def _sim_out(T, V, heads, want_scores, out):
    """What sim_gemm and sim_gemm_banded share: the (Nt, Nv) score output (`out`, or allocated here; None with the pitch of a dense
    matrix when only counts are wanted) and the scale that undoes the operands' prescale.  Returns (S, lds, scale)."""
    S, lds = None, V.N
    if want_scores:
        S, lds = _rows(out if out is not None else alloc_scores(T.N, V.N, T.buf.device), 'out')
        if tuple(S.shape) != (T.N, V.N):
            raise ValueError('out must be (%d, %d)' % (T.N, V.N))
    return S, lds, 1.0 / (heads * T.prescale * V.prescale)


def sim_gemm(T, V, heads=1, out=None, want_scores=True, gt_col=None, s_gt=None, count=None, col0=0):
    """S = T.V^T / (heads * prescale^2) on Packed operands; optional fused ground-truth rank count."""
    if T.precision != V.precision or T.K != V.K:
        raise ValueError('operands differ in precision or K')
    S, lds, scale = _sim_out(T, V, heads, want_scores, out)
    if gt_col is not None:
        _dev(gt_col, 'gt_col', torch.int32)
        _dev(s_gt, 's_gt')
        _dev(count, 'count', torch.int32)
    lib, h = _context(T.buf.device)
    _call('sim_gemm', lib.laff_sim_gemm, h, _ptr(T.buf), _ptr(V.buf), T.N, V.N, T.K, scale, PREC[T.precision], _ptr(S), lds,
                            _ptr(gt_col), col0, _ptr(s_gt), _ptr(count))
    return S


def _hist_rows(E, name, heads):
    """An operand of sim_hist as rows: (2-D view, its pitch, heads, d)."""
    _dev(E, name)
    rows = E
    if E.dim() == 3:
        N, heads, d = E.shape
        if E.numel() and (E.stride(2) != 1 or E.stride(1) != d):
            raise ValueError('%s must be (N, H, d) with the heads of a row contiguous, got strides %s' % (name, E.stride()))
        rows = E.as_strided((N, heads * d), (E.stride(0), 1)) if E.numel() else E.reshape(N, heads * d)
    rows, ld = _rows(rows, name)
    if heads < 1 or rows.shape[1] < 1 or rows.shape[1] % heads:
        raise ValueError('%s: width %d does not split into %d heads' % (name, rows.shape[1], heads))
    return rows, ld, heads, rows.shape[1] // heads


def sim_hist(T, V, heads=1, eps=1e-14, out=None):
    """The 'hist' measure (generalised Jaccard; loss.hist_sim / jaccard_sim of the reference) of every text row against every video
    row: S[t, v] = mean over heads of sum_k min(T, V) / (sum_k max(T, V) + eps), fp32.  T (Nt, H d) / V (Nv, H d) with `heads`, or
    (Nt, H, d) / (Nv, H, d); row views with a pitch are taken as they are.  `out`: an (Nt, Nv) fp32 tensor with contiguous rows
    (default: alloc_scores).  eps = 0 gives NaN for a pair of all-zero rows."""
    t, ldt, Ht, dt = _hist_rows(T, 'T', heads)
    v, ldv, Hv, dv = _hist_rows(V, 'V', heads)
    if T.dim() != V.dim() or (Ht, dt) != (Hv, dv):
        raise ValueError('T %s and V %s differ in heads or width' % (tuple(T.shape), tuple(V.shape)))
    if t.device != v.device:
        raise ValueError('T and V are on different devices')
    Nt, Nv = t.shape[0], v.shape[0]
    S, lds = _rows(_dev(out, 'out') if out is not None else alloc_scores(Nt, Nv, t.device), 'out')
    if tuple(S.shape) != (Nt, Nv):
        raise ValueError('out must be (%d, %d), got %s' % (Nt, Nv, tuple(S.shape)))
    lib, h = _context(t.device)
    _call('sim_hist', lib.laff_sim_hist, h, _ptr(t), ldt, _ptr(v), ldv, Nt, Nv, Ht, dt, float(eps), _ptr(S), lds)
    return S


#: the kernels laff_sim_gemm / laff_sim_gemm_banded choose between (LAFF_ROUTE_* of include/laff_hip.h, in that order)
SIM_ROUTES = _lib.enum_names('LAFF_ROUTE_')
_COUNT_MODES = {None: 0, 'approx': 1, 'banded': 2}


def sim_gemm_route(Nt, Nv, K, precision, lds=None, count=None, pair_cap=None, device=None):
    """Name of the kernel (SIM_ROUTES) that sim_gemm (count None / 'approx') or sim_gemm_banded (count 'banded') runs for an Nt x Nv
    problem of K packed elements, with scores of row pitch lds (None: count only) in a 16-byte aligned buffer; launches nothing.
    Reads the LAFF_STRIP mode and CU count of the device's context (laff_sim_gemm_route)."""
    if count not in _COUNT_MODES:
        raise ValueError('count must be None, \'approx\' or \'banded\', got %r' % (count,))
    if count == 'banded' and pair_cap is None:
        pair_cap = default_pair_cap(Nt)
    lib, h = _context(torch.device(device) if device is not None else torch.device('cuda'))
    route = C.c_int(-1)
    check(lib.laff_sim_gemm_route(h, int(Nt), int(Nv), int(K), PREC[precision], int(lds or 0), _COUNT_MODES[count], int(pair_cap or 0),
                                  C.byref(route)))
    return SIM_ROUTES[route.value]


def row_dot_gt(T, V, gt_col, heads=1, col0=0, zero_count=None):
    """s_gt[t] = <T[t], V[gt[t]-col0]> / (heads * prescale^2) on the packed operands; -inf outside this shard.
    zero_count: optional int32 (Nt,) tensor cleared by the same launch (the accumulator of the fused count)."""
    _dev(gt_col, 'gt_col', torch.int32)
    if zero_count is not None:
        _dev(zero_count, 'zero_count', torch.int32)
        if zero_count.numel() != T.N or not zero_count.is_contiguous():
            raise ValueError('zero_count must be a contiguous int32 vector of %d' % T.N)
    out = torch.empty((T.N,), device=T.buf.device, dtype=torch.float32)
    scale = 1.0 / (heads * T.prescale * V.prescale)
    lib, h = _context(T.buf.device)
    _call('row_dot_gt', lib.laff_row_dot_gt, h, _ptr(T.buf), _ptr(V.buf), T.N, V.N, T.K, scale, PREC[T.precision], _ptr(gt_col),
          col0, _ptr(out), _ptr(zero_count))
    return out


class RankState:
    """What the exact-rank pipeline carries between its three launches (laff_rank_prepare -> laff_sim_gemm_banded ->
    laff_rank_resolve): the exact ground-truth scores (fp64; all-reduce MAX them when videos are sharded), the two band vectors,
    the count accumulator and the list of pairs inside the band."""

    def __init__(self, Et, Ev, T, V, heads, gt_col, col0, s_gt64, band_t, band_v, count, pairs, pair_cap):
        self.Et, self.Ev, self.T, self.V, self.heads, self.gt_col, self.col0 = Et, Ev, T, V, heads, gt_col, col0
        self.s_gt64, self.band_t, self.band_v, self.count, self.pairs, self.pair_cap = s_gt64, band_t, band_v, count, pairs, pair_cap

    GROUP_WORDS, GROUP_CHUNK = 24, 64      # the strip kernel's list (sim_strip.hip): entries of 24 words in chunks of 64

    def _header(self):
        h = self.pairs[:4].cpu().tolist()
        return h[0] & 0xffffffff, h[1], h[2] & 0xffffffff, h[3] & 0xffffffff

    def listed_pairs(self):
        """(number of pairs inside the error band that the GEMM handed to laff_rank_resolve, overflow flag) -- synchronises;
        diagnostics only.  Two list layouts (the header's third word tells them apart):
          tiled kernel: header {overflow count, overflow flag, A, chunk}, A slots of per-wavefront segments (unused slots have row
                        0xffffffff), then the overflow pairs;
          strip kernel: header {chunks taken, overflow flag, NW | 1 << 31, NCH}, NCH per-chunk entry counts, then NCH chunks of 64
                        entries {row, colbase, lo, hi | mask16, the row's ground-truth column, 0, 0 | 16 raw accumulators}: the
                        pairs are the listed elements with lo <= x <= hi (the test laff_rank_resolve applies)."""
        return int(self.pair_indices().shape[0]), self.overflowed()

    def overflowed(self):
        """The list's overflow flag (one 16-byte copy; synchronises): pairs were dropped, the counts are poisoned."""
        return bool(self._header()[1])

    def pair_indices(self):
        """(n, 2) int64 tensor of the (row, col) pairs inside the band -- synchronises; diagnostics / tests only."""
        n_over, _, third, fourth = self._header()
        if not (third & 0x80000000):
            reg_a = third
            seg = self.pairs[4:4 + 2 * reg_a].view(-1, 2)
            over = self.pairs[4 + 2 * reg_a:4 + 2 * (reg_a + min(n_over, max(self.pair_cap - reg_a, 0)))].view(-1, 2)
            return torch.cat([seg[seg[:, 0] != -1], over]).long()
        nw, nch, W, CH = third & 0x7fffffff, fourth, self.GROUP_WORDS, self.GROUP_CHUNK
        cnt_words = (nch + 3) & ~3
        nchunks = min(nw + n_over, nch)                   # (header word 0: chunks taken from the pool)
        counts = self.pairs[4:4 + nchunks].long().clamp(max=CH)
        ent = self.pairs[4 + cnt_words:4 + cnt_words + nchunks * CH * W].view(nchunks, CH, W)
        live = torch.arange(CH, device=ent.device)[None, :] < counts[:, None]
        ent = ent[live]
        if ent.shape[0] == 0:
            return torch.zeros((0, 2), dtype=torch.int64, device=ent.device)
        e = torch.arange(16, device=ent.device)
        x = ent[:, 8:24].view(torch.float32)
        lo, hi = ent[:, 2:3].view(torch.float32), ent[:, 3:4].view(torch.float32)
        rows = ent[:, 0:1].long().expand(-1, 16)
        cols = ent[:, 1:2].long() + 8 * (e >> 2)[None, :] + (e & 3)[None, :]
        listed = ((ent[:, 4:5] >> e[None, :]) & 1).bool() & (cols != ent[:, 5:6].long()) & (x >= lo) & (x <= hi)
        return torch.stack([rows[listed], cols[listed]], dim=1)


def _emb3(E, name):
    _dev(E, name)
    if E.dim() == 2:
        E = E.unsqueeze(1)
    if E.dim() != 3 or not E.is_contiguous():
        raise ValueError('%s must be a contiguous (N, H, d) or (N, d) fp32 tensor' % name)
    return E


def default_pair_cap(Nt):
    """Slots (8 bytes each) of the in-band list.  The strip kernel lists groups of 16 accumulators (96 bytes per dumped lane): 128 Nt
    slots hold ~10 dumped lanes per text -- C4 uses 3.3 (1.3e5 of 4.3e5) with fp16 operands."""
    return max(1 << 20, 128 * int(Nt))


def _gt_col(gt_col, Nt=None):
    """gt_col as the rank kernels take it: int32 (with Nt: a contiguous vector of Nt), cloned when it does not start on 16 bytes
    (the banded GEMM fetches it in 16-byte groups)."""
    _dev(gt_col, 'gt_col', torch.int32)
    if Nt is not None and (gt_col.numel() != Nt or not gt_col.is_contiguous()):
        raise ValueError('gt_col must be a contiguous int32 vector of %d' % Nt)
    return gt_col.clone() if gt_col.data_ptr() % 16 else gt_col


# The rank-state buffers.  The slack is what the banded GEMM may read past the end: it fetches these vectors in 16-byte groups.
def _alloc_text_bands(Nt, dev):
    """(s_gt64: Nt float64 of Nt + 2, band_t: Nt + 4 float32)."""
    return torch.empty((Nt + 2,), device=dev, dtype=torch.float64)[:Nt], torch.empty((Nt + 4,), device=dev, dtype=torch.float32)


def _alloc_band_v(Nv, dev):
    """band_v in the layout the banded GEMM reads: one float per column, then -- from a 16-byte aligned offset -- the maximum of
    every 64-column block, + 4 of slack."""
    return torch.empty((((Nv + 3) & ~3) + (Nv + 63) // 64 + 4,), device=dev, dtype=torch.float32)


def _alloc_list(Nt, pair_cap, dev):
    """The in-band list of pair_cap slots (None: default_pair_cap) in the whole groups of four the kernels use, one at least:
    (count: Nt int32, pairs: a header of 4 int32 then cap slots of {row, col}, cap)."""
    cap = (int(pair_cap) if pair_cap is not None else default_pair_cap(Nt)) & ~3
    if cap < 4:
        raise ValueError('pair_cap must be >= 4')
    return torch.empty((Nt,), device=dev, dtype=torch.int32), torch.empty((4 + 2 * cap,), device=dev, dtype=torch.int32), cap


def _opt_scores(S):
    """An optional score matrix argument: (S, its row pitch), or (None, 0)."""
    return _rows(S, 'S') if S is not None else (None, 0)


def fused_prepare_eligible(Nt, Nv, H, d, precision):
    """laff_fuse_packed_rank covers split heads of d <= 512 with a single-plane 16-bit operand; the text launch finishes the videos'
    64-column block maxima (it needs ceil(Nv / 64) workgroups of 4 (row, head) items)."""
    return H >= 1 and d <= 512 and d % 4 == 0 and precision in ('fp16', 'bf16') and Nv >= 1 and 16 * Nt * H >= Nv * 4 and 16 * Nt >= Nv


class FusedPrepare:
    """laff_rank_prepare's outputs produced by the two fuse launches of a pass (laff_fuse_packed_rank, videos first): allocate with the
    problem's sizes, hand `.video` / `.text` to the fuse calls of the two towers as `rank_side`, then `.state()` is the RankState
    rank_prepare would have returned."""

    class _Side:
        def __init__(self, owner, side):
            self.owner, self.side = owner, side

        def side_struct(self, N, E):
            o = self.owner
            H = E.shape[1]
            if H != o.heads:
                raise ValueError('the tower produced %d heads, FusedPrepare was made for %d' % (H, o.heads))
            part = tick = None
            if H > 1:
                part = torch.empty((N, H, 2), device=E.device, dtype=torch.float64)
                tick = torch.empty((N,), device=E.device, dtype=torch.int32)
                o._scratch.append((part, tick))
            pp, tp = (part.data_ptr() if part is not None else None), (tick.data_ptr() if tick is not None else None)
            if self.side == 2:
                if N != o.Nv:
                    raise ValueError('the video tower produced %d rows, FusedPrepare was made for %d' % (N, o.Nv))
                return RankSide(2, None, 0, None, 0, None, o.band_v.data_ptr(), None, None, None, pp, tp)
            if N != o.Nt or o.Ev is None:
                raise ValueError('the text tower must run behind the video tower (%d rows, FusedPrepare made for %d)' % (N, o.Nt))
            return RankSide(1, o.gt_col.data_ptr(), o.col0, o.Ev.data_ptr(), o.Nv, o.s_gt64.data_ptr(), o.band_t.data_ptr(),
                            o.band_v.data_ptr(), o.count.data_ptr(), o.pairs.data_ptr(), pp, tp)

        def done(self, E, packed):
            if self.side == 2:
                self.owner.Ev, self.owner.V = E, packed
            else:
                self.owner.Et, self.owner.T = E, packed

    def __init__(self, Nt, Nv, gt_col, col0=0, pair_cap=None, heads=1):
        gt_col = _gt_col(gt_col, Nt)
        dev = gt_col.device
        self.Nt, self.Nv, self.gt_col, self.col0, self.heads = Nt, Nv, gt_col, int(col0), int(heads)
        self.s_gt64, self.band_t = _alloc_text_bands(Nt, dev)
        self.band_v = _alloc_band_v(Nv, dev)
        self.count, self.pairs, self.pair_cap = _alloc_list(Nt, pair_cap, dev)
        self.Et = self.Ev = self.T = self.V = None
        self._scratch = []
        self.video, self.text = self._Side(self, 2), self._Side(self, 1)

    def state(self):
        if self.Et is None or self.Ev is None:
            raise RuntimeError('FusedPrepare.state(): both fuse launches must have run (videos first)')
        return RankState(self.Et, self.Ev, self.T, self.V, self.heads, self.gt_col, self.col0, self.s_gt64, self.band_t, self.band_v,
                         self.count, self.pairs, self.pair_cap)


def rank_prepare(Et, Ev, T, V, gt_col, col0=0, pair_cap=None, emit_precision=None):
    """First launch of the exact-rank pipeline.  Et (Nt, H, d) / Ev (Nv, H, d): the fp32 embeddings; T / V: the Packed GEMM
    operands made from them; gt_col int32 (Nt,) ground-truth column of every text (global index; col0 = first column of this
    video shard).  Returns a RankState.
    T or V None (with emit_precision 'fp16' | 'bf16', or the other operand's): that operand is PRODUCED by the launch from the
    embedding rows -- E * prescale converted without re-normalising, what pack_rows(E, normalize=False) returns (laff_rank_prepare_emit);
    it is in the returned state."""
    Et, Ev = _emb3(Et, 'Et'), _emb3(Ev, 'Ev')
    Nt, H, d = Et.shape
    Nv = Ev.shape[0]
    emit = (1 if T is None else 0) | (2 if V is None else 0)
    if emit:
        have = T if T is not None else V
        prec = emit_precision or (have.precision if have is not None else None)
        if prec not in ('fp16', 'bf16'):
            raise ValueError("rank_prepare can only produce single-plane 16-bit operands ('fp16' | 'bf16'), got %r" % prec)
        ps = have.prescale if have is not None else default_prescale(prec)
        if T is None:
            T = Packed(torch.empty((max(Nt * H * d * 2, 16),), device=Et.device, dtype=torch.uint8), Nt, H * d, prec, ps)
        if V is None:
            V = Packed(torch.empty((max(Nv * H * d * 2, 16),), device=Et.device, dtype=torch.uint8), Nv, H * d, prec, ps)
    if tuple(Ev.shape[1:]) != (H, d) or T.N != Nt or V.N != Nv or T.K != H * d or V.K != H * d:
        raise ValueError('embeddings %s / %s do not match the operands (%d x %d, %d x %d)' % (tuple(Et.shape), tuple(Ev.shape), T.N, T.K, V.N, V.K))
    if T.precision != V.precision or T.prescale != V.prescale:
        raise ValueError('operands differ in precision or prescale')
    gt_col = _gt_col(gt_col, Nt)
    dev = Et.device
    s_gt64, band_t = _alloc_text_bands(Nt, dev)
    band_v = _alloc_band_v(Nv, dev)
    count, pairs, cap = _alloc_list(Nt, pair_cap, dev)
    lib, h = _context(dev)
    entry = (lib.laff_rank_prepare_emit, h, emit) if emit else (lib.laff_rank_prepare, h)
    _call('rank_prepare', *entry, _ptr(Et), _ptr(Ev), _ptr(T.buf), _ptr(V.buf), Nt, Nv, H, d, PREC[T.precision], float(T.prescale),
          _ptr(gt_col), int(col0), _ptr(s_gt64), _ptr(band_t), _ptr(band_v), _ptr(count), _ptr(pairs))
    return RankState(Et, Ev, T, V, H, gt_col, int(col0), s_gt64, band_t, band_v, count, pairs, cap)


def rank_prepare_text(Et, Ev, T, gt_col, col0=0, prescale=None):
    """The TEXT side of laff_rank_prepare alone (laff_rank_prepare_part, sides = 1): exact ground-truth scores of the texts Et against
    the fp32 video rows Ev (gt_col - col0 indexes them; -inf outside) and their error bands.  Returns (s_gt64, band_t)."""
    Et, Ev = _emb3(Et, 'Et'), _emb3(Ev, 'Ev')
    Nt, H, d = Et.shape
    if tuple(Ev.shape[1:]) != (H, d) or T.N != Nt or T.K != H * d:
        raise ValueError('embeddings %s / %s do not match the operand (%d x %d)' % (tuple(Et.shape), tuple(Ev.shape), T.N, T.K))
    gt_col = _gt_col(gt_col, Nt)
    s_gt64, band_t = _alloc_text_bands(Nt, Et.device)
    lib, h = _context(Et.device)
    _call('rank_prepare', lib.laff_rank_prepare_part, h, 1, _ptr(Et), _ptr(Ev), _ptr(T.buf), None, Nt, Ev.shape[0], H, d, PREC[T.precision],
          float(T.prescale), _ptr(gt_col), int(col0), _ptr(s_gt64), _ptr(band_t), None, None, None)
    return s_gt64, band_t


def rank_band_video(Ev, V):
    """The VIDEO side of laff_rank_prepare alone (sides = 2): band_v of the rows Ev / their operand V, in the layout the banded GEMM
    reads (per column, then per 64-column block)."""
    Ev = _emb3(Ev, 'Ev')
    Nv, H, d = Ev.shape
    if V.N != Nv or V.K != H * d:
        raise ValueError('embeddings %s do not match the operand (%d x %d)' % (tuple(Ev.shape), V.N, V.K))
    band_v = _alloc_band_v(Nv, Ev.device)
    lib, h = _context(Ev.device)
    _call('rank_prepare', lib.laff_rank_prepare_part, h, 2, None, _ptr(Ev), None, _ptr(V.buf), 0, Nv, H, d, PREC[V.precision], float(V.prescale),
          None, 0, None, None, _ptr(band_v), None, None)
    return band_v


def banded_state(T, V, heads, gt_col, col0, s_gt64, band_t, band_v, pair_cap=None):
    """A RankState for laff_sim_gemm_banded assembled from parts (no fp32 rows: its list is exported, not resolved here)."""
    gt_col = _gt_col(gt_col)
    count, pairs, cap = _alloc_list(T.N, pair_cap, T.buf.device)
    count.zero_()
    pairs[:4].zero_()
    return RankState(None, None, T, V, heads, gt_col, int(col0), s_gt64, band_t, band_v, count, pairs, cap)


def rank_export_pairs(st, S, bounds, col0, cap):
    """The listed pairs of a banded GEMM, bucketed by the owner of the text row (laff_rank_export_pairs).  bounds: int32 device
    tensor (world + 1).  Returns (out (world, cap, 2) int32 -- unused slots -1 --, fill (world + 1) int32)."""
    world = bounds.numel() - 1
    cap = (int(cap) + 3) & ~3
    dev = st.pairs.device
    out = torch.empty((world, cap, 2), device=dev, dtype=torch.int32)
    fill = torch.empty((world + 1,), device=dev, dtype=torch.int32)
    S, lds = _opt_scores(S)
    lib, h = _context(dev)
    _call('rank_export', lib.laff_rank_export_pairs, h, _ptr(st.s_gt64), _ptr(st.count), _ptr(S), lds, st.V.N, _ptr(st.pairs), st.pair_cap,
          _ptr(bounds), world, int(col0), _ptr(out), cap, _ptr(fill))
    return out, fill


def rank_resolve_list(Et, Ev, s_gt64, count, lst):
    """laff_rank_resolve on a plain list: lst int32 (4 + 2 n), header {0, 0, n, 4} then n slots {row, col} with unused slots -1 and
    the valid pairs first in every group of four (what concatenated laff_rank_export_pairs buckets are).  count += wins."""
    return rank_resolve(RankState(_emb3(Et, 'Et'), _emb3(Ev, 'Ev'), None, None, None, None, 0, s_gt64, None, None, count, lst,
                                  (lst.numel() - 4) // 2))


def sim_gemm_banded(st, want_scores=True, out=None):
    """Second launch: the similarity GEMM with the banded count (state.count, state.pairs are filled).  Returns S or None."""
    T, V = st.T, st.V
    S, lds, scale = _sim_out(T, V, st.heads, want_scores, out)
    lib, h = _context(T.buf.device)
    _call('sim_gemm', lib.laff_sim_gemm_banded, h, _ptr(T.buf), _ptr(V.buf), T.N, V.N, T.K, scale, PREC[T.precision], _ptr(S), lds,
          _ptr(st.gt_col), st.col0, _ptr(st.s_gt64), _ptr(st.band_t), _ptr(st.band_v), _ptr(st.count), _ptr(st.pairs), st.pair_cap)
    return S


def rank_resolve(st, S=None):
    """Third launch: exact re-score of the listed pairs; state.count (+ S) are final afterwards."""
    S, lds = _opt_scores(S)
    Nt, H, d = st.Et.shape
    lib, h = _context(st.Et.device)
    _call('rank_resolve', lib.laff_rank_resolve, h, _ptr(st.Et), _ptr(st.Ev), Nt, st.Ev.shape[0], H, d, _ptr(st.s_gt64), _ptr(st.count),
          _ptr(S), lds, _ptr(st.pairs), st.pair_cap)
    return st.count


def rank_resolve_metrics(st, S=None, out_pinned=None, base=1, ranks_out=None):
    """laff_rank_resolve + the rank metrics in ONE launch (laff_rank_resolve_metrics): the resolve workgroup that finishes last turns
    the final counts into ranks (ranks_out <- count + base) and the seven metrics.
    out_pinned None: synchronises, returns the 7-tuple (RuntimeError if a rank < 1 was flagged: overflowed pair list).
    out_pinned (pinned float64 tensor of >= 8): no sync, capturable; the device writes the 8 doubles into it directly; returns None."""
    S, lds = _opt_scores(S)
    Nt, H, d = st.Et.shape
    lib, h = _metrics_context(st.Et.device)
    ro = _ranks_out(st.count, ranks_out)
    sync = out_pinned is None
    out = (C.c_double * 8)() if sync else _pinned8(out_pinned)
    _call('rank_resolve', lib.laff_rank_resolve_metrics, h, _ptr(st.Et), _ptr(st.Ev), Nt, st.Ev.shape[0], H, d, _ptr(st.s_gt64),
          _ptr(st.count), _ptr(S), lds, _ptr(st.pairs), st.pair_cap, int(base), _ptr(ro), out, 1 if sync else 0)
    return tuple(out)[:7] if sync else None


def exact_ranks(Et, Ev, T, V, gt_col, want_scores=True, col0=0, pair_cap=None):
    """prepare -> banded GEMM -> resolve on one device.  Returns (S or None, count int32 (Nt,), RankState); ranks = count + 1.
    An overflowing pair list (state.listed_pairs()[1]) poisons count[0]: rank_metrics(base=1) raises on it."""
    st = rank_prepare(Et, Ev, T, V, gt_col, col0, pair_cap)
    S = sim_gemm_banded(st, want_scores)
    rank_resolve(st, S)
    return S, st.count, st


def gather_gt(S, gt_col, col0=0):
    S, lds = _rows(S, 'S')
    _dev(gt_col, 'gt_col', torch.int32)
    out = torch.empty((S.shape[0],), device=S.device, dtype=torch.float32)
    lib, h = _context(S.device)
    _call('gather_gt', lib.laff_gather_gt, h, _ptr(S), S.shape[0], S.shape[1], lds, _ptr(gt_col), col0, _ptr(out))
    return out


def rank_count(S, gt_col, s_gt, col0=0, count=None):
    S, lds = _rows(S, 'S')
    _dev(gt_col, 'gt_col', torch.int32)
    _dev(s_gt, 's_gt')
    acc = count is not None
    if count is None:
        count = torch.empty((S.shape[0],), device=S.device, dtype=torch.int32)
    _dev(count, 'count', torch.int32)
    lib, h = _context(S.device)
    _call('rank_count', lib.laff_rank_count, h, _ptr(S), S.shape[0], S.shape[1], lds, _ptr(gt_col), col0, _ptr(s_gt), _ptr(count),
                              1 if acc else 0)
    return count


def _topk_kp(K):
    return 64 if K <= 64 else (512 if K <= 512 else (2048 if K <= 2048 else (4096 if K <= 4096 else 8192)))


def topk_max_columns(K):
    """columns of one laff_topk_rows call: the row lives in LDS next to the K' selected (key, index) pairs"""
    return (160 * 1024 - _topk_kp(K) * 8 - 1040) // 4


def _topk_call(S, K):
    S, lds = _rows(S, 'S')
    Nt, Nv = S.shape
    idx = torch.empty((Nt, K), device=S.device, dtype=torch.int32)
    val = torch.empty((Nt, K), device=S.device, dtype=torch.float32)
    lib, h = _context(S.device)
    _call('topk_rows', lib.laff_topk_rows, h, _ptr(S), Nt, Nv, lds, int(K), _ptr(idx), _ptr(val))
    return idx, val


def _topk_blocks(blocks, K, Nv):
    """K best of every row over column blocks handed in one at a time as (first column, (Nt, w) score tensor): each block's K best
    are taken (laff_topk_rows) and the lists merged by the same kernel -- block lists are laid out in ascending (score, index) order
    and blocks in column order, so that position order equals index order among equal scores and the reference's tie rule (larger
    index first) carries over.  A block may be overwritten as soon as the next one is asked for."""
    cap = topk_max_columns(K)
    vals, idxs = [], []
    for c0, blk in blocks:
        k = min(K, blk.shape[1])
        i, v = _topk_call(blk, k)
        vals.append(v.flip(1))
        idxs.append((i + c0).flip(1))
    if len(vals) == 1 and vals[0].shape[1] == K:
        return idxs[0].flip(1).contiguous(), vals[0].flip(1).contiguous()
    cand_v, cand_i = torch.cat(vals, dim=1).contiguous(), torch.cat(idxs, dim=1).contiguous()
    while cand_v.shape[1] > cap:             # very wide collections: merge groups of block lists first
        group = max(2, cap // K) * K
        nv, ni = [], []
        for c0 in range(0, cand_v.shape[1], group):
            pv, pi = cand_v[:, c0:c0 + group], cand_i[:, c0:c0 + group]
            k = min(K, pv.shape[1])
            p, v = _topk_call(pv, k)
            nv.append(v.flip(1))
            ni.append(torch.gather(pi, 1, p.long()).flip(1))
        cand_v, cand_i = torch.cat(nv, dim=1).contiguous(), torch.cat(ni, dim=1).contiguous()
    pos, val = _topk_call(cand_v, K)
    return torch.gather(cand_i, 1, pos.long()).contiguous(), val


def topk_rows(S, K):
    """Per row: indices (int32) and scores (fp32) of the K best columns, score descending, ties by larger index first (what the
    reference's `np.argsort(...)[::-1][:K]` yields with a stable sort, predictor.py:53-65).  Any number of columns: a collection that
    does not fit the kernel's LDS-resident row (~36k columns at K <= 2048) is split into column blocks (_topk_blocks).  K <= 8192."""
    S, lds = _rows(S, 'S')
    Nt, Nv = S.shape
    K = int(K)
    if K < 1 or K > Nv or K > 8192:
        raise ValueError('topk_rows: need 1 <= K <= min(Nv, 8192), got K=%d for %d columns' % (K, Nv))
    cap = topk_max_columns(K)
    if Nv <= cap:
        return _topk_call(S, K)
    return _topk_blocks(((c0, S[:, c0:min(Nv, c0 + cap)]) for c0 in range(0, Nv, cap)), K, Nv)


def topk_from_operands(T, V, K, heads=1, block_rows=None, scratch_bytes=192 << 20):
    """The K best videos of every text WITHOUT the (Nt, Nv) score matrix (the reference argsorts all of it to keep 500-2000 columns
    per row, predictor.py:53-65; at 100k x 30k that matrix is 12 GB written and read back).  Rows are independent, so the texts are
    taken in blocks: one block of the text operand is scored against all videos into ONE reusable (block_rows, Nv) buffer
    (laff_sim_gemm) and reduced to its lists right away (laff_topk_rows; collections wider than its LDS row are split by columns and
    merged, see topk_rows).  The default buffer (192 MB) stays inside the 256 MB Infinity Cache: the top-K kernel reads the block
    the GEMM just wrote without going to HBM.  (A running top-K inside the GEMM epilogue is not possible at these K: 64 rows x 2000
    entries x 8 bytes per wavefront against 160 KB of LDS per CU.)  Scores and order are exactly those of
    topk_rows(sim_gemm(T, V), K): an entry of the GEMM does not depend on the block it is computed in.
    Returns (idx int32 (Nt, K), val fp32 (Nt, K))."""
    if T.precision != V.precision or T.K != V.K:
        raise ValueError('operands differ in precision or K')
    Nt, Nv, K = T.N, V.N, int(K)
    if K < 1 or K > Nv or K > 8192:
        raise ValueError('topk_from_operands: need 1 <= K <= min(Nv, 8192), got K=%d for %d columns' % (K, Nv))
    dev = T.buf.device
    pitch = (Nv + 31) & ~31
    if block_rows is None:
        block_rows = max(256, (scratch_bytes // (4 * pitch)) & ~255)
    block_rows = int(min(max(int(block_rows), 1), Nt))
    buf = torch.empty((block_rows, pitch), device=dev, dtype=torch.float32)
    idx = torch.empty((Nt, K), device=dev, dtype=torch.int32)
    val = torch.empty((Nt, K), device=dev, dtype=torch.float32)
    for r0 in range(0, Nt, block_rows):
        r1 = min(Nt, r0 + block_rows)
        S = sim_gemm(T.rows(r0, r1), V, heads, out=buf[:r1 - r0, :Nv])
        i, v = topk_rows(S, K)
        idx[r0:r1], val[r0:r1] = i, v
    return idx, val


def _rerank_array(sizes):
    arr = (RerankProblem * max(len(sizes), 1))()
    for a, (Q, G) in zip(arr, sizes):
        a.Q, a.G = int(Q), int(G)
    return arr


def rerank_workspace_bytes(sizes, k1=20, k2=6):
    """laff_rerank_workspace_bytes for problems of the given (Q, G) sizes; raises on sizes or k1 / k2 outside the kernels' limits."""
    lib = _lib.load()
    n = C.c_size_t()
    check(lib.laff_rerank_workspace_bytes(_rerank_array(sizes), len(sizes), int(k1), int(k2), C.byref(n)))
    return n.value


def rerank_run(problems, k1=20, k2=6, lambda_value=0.3, workspace=None):
    """laff_rerank_run: k-reciprocal re-ranking of P independent problems in one call.  problems: a list of (qg [Q, G], qq [Q, Q],
    gg [G, G]) fp32 device SIMILARITY matrices with contiguous rows (views with a pitch are taken as they are).  Returns the list of
    [Q, G] fp32 results.  workspace: a uint8 device tensor of rerank_workspace_bytes(...) bytes, or None to allocate one here."""
    if not problems:
        return []
    arr = (RerankProblem * len(problems))()
    outs = []
    dev = problems[0][0].device
    for a, (qg, qq, gg) in zip(arr, problems):
        (qg, ldqg), (qq, ldqq), (gg, ldgg) = _rows(qg, 'q_g_dist'), _rows(qq, 'q_q_dist'), _rows(gg, 'g_g_dist')
        Q, G = qg.shape
        if tuple(qq.shape) != (Q, Q) or tuple(gg.shape) != (G, G):
            raise ValueError('re-ranking blocks must be q_g [Q, G], q_q [Q, Q], g_g [G, G]; got %s, %s, %s'
                             % (tuple(qg.shape), tuple(qq.shape), tuple(gg.shape)))
        out = torch.empty((Q, G), device=dev, dtype=torch.float32)
        a.qq, a.ldqq, a.qg, a.ldqg, a.gg, a.ldgg = qq.data_ptr(), ldqq, qg.data_ptr(), ldqg, gg.data_ptr(), ldgg
        a.out, a.ldo, a.Q, a.G = out.data_ptr(), max(G, 1), Q, G
        outs.append(out)
    lib, h = _context(dev)
    n = C.c_size_t()
    check(lib.laff_rerank_workspace_bytes(arr, len(problems), int(k1), int(k2), C.byref(n)))
    if workspace is None:
        workspace = torch.empty(max(n.value, 256), dtype=torch.uint8, device=dev)
    _call('rerank_run', lib.laff_rerank_run, h, arr, len(problems), int(k1), int(k2), float(lambda_value), _ptr(workspace),
          workspace.numel())
    return outs


def rerank_tkb(nn, cand, G):
    """laff_rerank_tkb: nn [G, k1] int32 (the k1 best columns of every g_g row), cand [Q, K] int32 (the K best columns of every q_g
    row).  Returns (out [Q, G] fp32: log(count + 1) at the candidate columns, 0 elsewhere; count [G] int32)."""
    nn, cand = _dev(nn, 'nn', torch.int32), _dev(cand, 'cand', torch.int32)
    if nn.dim() != 2 or cand.dim() != 2 or nn.shape[0] != G or not nn.is_contiguous() or not cand.is_contiguous():
        raise ValueError('nn must be [G, k1] and cand [Q, K], contiguous')
    Q, K = cand.shape
    count = torch.empty((G,), device=nn.device, dtype=torch.int32)
    out = torch.empty((Q, G), device=nn.device, dtype=torch.float32)
    lib, h = _context(nn.device)
    _call('rerank_tkb', lib.laff_rerank_tkb, h, _ptr(nn), int(G), nn.shape[1], _ptr(cand), Q, K, _ptr(count), _ptr(out), int(G))
    return out, count


def v2t_count(S, grp_off, grp_idx, max_group):
    S, lds = _rows(S, 'S')
    _dev(grp_off, 'grp_off', torch.int32)
    _dev(grp_idx, 'grp_idx', torch.int32)
    count = torch.zeros((S.shape[0],), device=S.device, dtype=torch.int32)
    lib, h = _context(S.device)
    _call('v2t_count', lib.laff_v2t_count, h, _ptr(S), S.shape[0], S.shape[1], lds, _ptr(grp_off), _ptr(grp_idx), int(max_group),
                             _ptr(count))
    return count


def v2t_count_exact(S, st, grp_off, grp_idx, max_group, list_cap=None):
    """laff_v2t_count_exact on the score matrix and RankState of exact_ranks (same operands, col0 == 0): int32 (Nt,) counts of texts
    that beat caption t in the column of its video, decided with the exact fp64 scores.  Synchronises (reads the overflow flag);
    a list that was too small is re-sized once."""
    S, lds = _rows(S, 'S')
    _dev(grp_off, 'grp_off', torch.int32)
    _dev(grp_idx, 'grp_idx', torch.int32)
    Nt, H, d = st.Et.shape
    if tuple(S.shape) != (Nt, st.Ev.shape[0]) or st.col0 != 0:
        raise ValueError('S %s does not belong to this RankState (%d x %d, col0 %d)' % (tuple(S.shape), Nt, st.Ev.shape[0], st.col0))
    count = torch.empty((Nt,), device=S.device, dtype=torch.int32)
    cap = int(list_cap) if list_cap is not None else max(1 << 16, 8 * Nt)
    lib, h = _context(S.device)
    for attempt in range(2):
        lst = torch.empty((4 + 3 * cap,), device=S.device, dtype=torch.int32)
        _call('v2t_count_exact', lib.laff_v2t_count_exact, h, _ptr(S), Nt, S.shape[1], lds, _ptr(grp_off), _ptr(grp_idx), int(max_group),
              _ptr(st.Et), _ptr(st.Ev), H, d, _ptr(st.s_gt64), _ptr(st.band_t), _ptr(st.band_v), _ptr(count), _ptr(lst), cap)
        wanted, overflow = [int(x) & 0xffffffff for x in lst[:2].cpu().tolist()]
        if not overflow:
            return count
        cap = wanted + 1024
    raise RuntimeError('laff_v2t_count_exact: the list of in-band pairs overflowed twice (%d wanted)' % wanted)


def _ranks_out(r, ranks_out):
    if ranks_out is not None:
        _dev(ranks_out, 'ranks_out', torch.int32)
        if ranks_out.numel() != r.numel() or not ranks_out.is_contiguous():
            raise ValueError('ranks_out must be a contiguous int32 vector of %d' % r.numel())
    return ranks_out


def _pinned8(out_pinned):
    """The address of a pinned result buffer (the device writes the 8 doubles into it itself)."""
    if out_pinned.dtype != torch.float64 or out_pinned.numel() < 8 or not out_pinned.is_pinned():
        raise ValueError('out_pinned must be a pinned float64 tensor of >= 8 elements')
    return C.c_void_p(out_pinned.data_ptr())


def _metrics_context(device):
    """_context for a call that takes an asynchronous metrics slot: the context's metrics scratch must exist before a capture."""
    lib, h = _context(device)
    if ('metrics', h.value) not in _ctx:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('call ops.ctx_prepare_metrics(device) before capturing a graph (it allocates scratch)')
        ctx_prepare_metrics(device)
    return lib, h


def rank_metrics(rank1, base=0, ranks_out=None):
    """(r1, r5, r10, medr, meanr, mir, mAP) from int32 device values r with rank = r + base (1-based ranks: base 0; counts of
    better-scoring videos: base 1); ranks_out optionally receives the ranks.  Synchronises the stream."""
    _dev(rank1, 'rank1', torch.int32)
    out = (C.c_double * 7)()
    lib, h = _context(rank1.device)
    _call('rank_metrics', lib.laff_rank_metrics, h, _ptr(rank1.contiguous()), rank1.numel(), int(base), _ptr(_ranks_out(rank1, ranks_out)), out)
    return tuple(out)


def rank_metrics_async(rank1, out_pinned, base=0, ranks_out=None):
    """Launch the metrics reduction and the 64-byte D2H copy without synchronising (HIP-graph capturable).
    out_pinned: pinned CPU float64 tensor of 8; after a stream sync [:7] are the metrics, [7] != 0 flags a rank < 1."""
    _dev(rank1, 'rank1', torch.int32)
    out = _pinned8(out_pinned)
    lib, h = _metrics_context(rank1.device)
    _call('rank_metrics', lib.laff_rank_metrics_async, h, _ptr(rank1.contiguous()), rank1.numel(), int(base), _ptr(_ranks_out(rank1, ranks_out)),
          out)


def ctx_prepare_metrics(device):
    """Allocate the ctx's metrics scratch outside any graph capture (hipMalloc is not capturable)."""
    lib, h = _context(device)
    key = ('metrics', h.value)
    if key not in _ctx:
        r = torch.ones(1, dtype=torch.int32, device=device)
        out = (C.c_double * 7)()
        check(lib.laff_rank_metrics(h, _ptr(r), 1, 0, None, out))
        _ctx[key] = True
