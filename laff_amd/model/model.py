"""Retrieval towers and predict() of the reference's model/model.py on the MI355X kernels.

Same registry keys, class names, constructor/forward signatures, config attribute names and state_dict keys
as /root/reference/model/model.py for the symbols on the hot path:

  TransformNet                         :211-276     -> laff_fc_act_bn (fp32 MFMA GEMM + fused epilogue)
  VisMutiTransformNet                  :1787-1827
  VisMutiTransformNetAddAttnetion      :1830-1881   -> planes + one laff_fuse launch (no stack / repeat copies)
  MultiScaleTxtEncoderAttention        :1641-1709
  VisMutiTransformNetPlusFrameFeat     :2101-2194   -> laff_frame_fuse instead of the per-sample Python loop
  W2VVPP.get_txt2vis_matrix / predict  :1003-1128   -> one laff_sim_gemm over all pairs instead of the
                                                       (Nt/bs)x(Nv/bs) block loop; embeddings stay in HBM
  VisTransformNet                      :279-308     -> laff_fc_concat_act_bn: the W2VV++ concat towers, one segmented-K launch,
  MultiScaleTxtEncoder / MultiScaleTxtNet :552-726     the concatenated input never formed
  get_model                            :2501-2519

Differentiable in .train() mode (the autograd Functions live in model/autograd.py):
  TransformNet on a dense input, plane() included       _FcActFn       DESIGN.md section 4.20
  TransformNet on a device CSR input                     _FcGatherFn    section 4.24
  TransformNet.concat_train (a concat layer)             _FcConcatFn    section 4.24
  its dropout + BatchNorm1d stage with device_norm       _DropoutBnFn   section 4.25 (torch's own ops without device_norm)
  the fusion blocks (model/Attention.py)                                section 4.19
  VisMutiTransformNetPlusFrameFeat.frame_vector                         section 4.22
  the expert stage of the LAFF towers (expert embedding + l2norm)  _ExpertStageFn section 4.27
  the LAFF and FrameLAFF towers' prepare() / forward and the model's training step (enable_training, forward)   section 4.27
Inference only (_eval_only raises in training mode): TransformNet.concat_problem and a concat tower that no enable_training() armed, and the
FrameLAFF video tower's prepare() / forward until its model's enable_training() has armed it; retrieve() / predict() put the model in
eval mode.

Text encoders (GRU / BoW / W2V / CLIP, :311-549) are upstream of the path: features arrive pre-extracted in
`caption_feat_dict` (the reference already does this for frozen CLIP via 'CLIP_encoding', :497-498); any module
returning {'text_features': tensor} can be plugged into `txt_net.encoder.<name>`.
"""
import numpy as np

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import loss as _loss
from .. import ops
from .. import optim as _optim
from .Attention import Attention_1, JustAverage, Multi_head_MyApply_Attention, Multi_head_MyApply_selfAttention
from .autograd import (_csc_of, _DropoutBnFn, _ExpertStageFn, _FcActFn, _FcConcatFn, _FcConcatGroupedFn, _FcGatherFn, _fp32_params,  # noqa: F401  (kept importable from here)
                       _TileBnFn)

device = torch.device('cuda')
float16 = False
#: arithmetic of the FC projections: 'fp32' (v_mfma_f32_32x32x2_f32, bit-for-bit an fp32 FMA chain) or 'fp16x3'
#: (exact fp16 hi/lo operand split, 3 MFMA passes at the fp16 rate, ~2^-22 relative per product)
FC_PRECISION = 'fp32'


def _row_chunks(pending, limit_bytes=1 << 31):
    """The split-product GEMMs address an operand with 32-bit byte offsets (the C ABI refuses a packed operand of 4 GiB or more:
    300k x 4096 fp32 rows already exceed it).  Row blocks are independent, so an oversized problem is cut into row chunks that share
    its weights and write into views of its output -- same results, a few more tiles in the grouped launch."""
    out = []
    for q in pending:
        x = q['x']
        if not torch.is_tensor(x) or x.layout != torch.strided or x.dim() != 2:
            out.append(q)
            continue
        n, k = x.shape
        row_bytes = 4 * max(x.stride(0) if n > 1 else k, (k + 63) // 64 * 64)
        if n * row_bytes < limit_bytes:
            out.append(q)
            continue
        if q.get('out') is None:
            q['out'] = torch.empty((n, q['weight'].shape[0]), device=x.device, dtype=torch.float32)
        step = max(256, (limit_bytes // row_bytes) // 256 * 256)
        for a in range(0, n, step):
            out.append(dict(q, x=x[a:a + step], out=q['out'][a:a + step]))
    return out


def _loader_len(loader):
    ds = getattr(loader, 'dataset', None)
    try:
        return len(ds) if ds is not None else len(loader)
    except TypeError:
        return 1


def coalesce_batches(batches):
    """Concatenate the batch dicts of a loader into one: tensors / arrays along dim 0, lists and tuples end to end, nested dicts
    key by key, None stays None.  Raises TypeError / ValueError / RuntimeError when the batches do not line up."""
    if not batches:
        return None
    first = batches[0]
    if isinstance(first, dict):
        if any(not isinstance(b, dict) or b.keys() != first.keys() for b in batches):
            raise ValueError('batch dicts with different keys')
        return {k: coalesce_batches([b[k] for b in batches]) for k in first}
    if first is None:
        if any(b is not None for b in batches):
            raise ValueError('None mixed with values')
        return None
    if isinstance(first, torch.Tensor):
        return torch.cat(list(batches), dim=0)
    if isinstance(first, np.ndarray):
        return np.concatenate(list(batches), axis=0)
    if isinstance(first, (list, tuple)):
        return [x for b in batches for x in b]
    raise TypeError('cannot concatenate batch values of type %s' % type(first).__name__)


def run_fc(pending):
    """Launch every queued FC projection; returns their outputs in the order of `pending`.  Concat-tower problems (a 'segments' list:
    VisTransformNet / MultiScaleTxtNet) run as ONE segmented-K launch, in fp32 arithmetic whatever FC_PRECISION says (that kernel has
    no 16-bit operand route); the per-feature projections as before."""
    concat = [q for q in pending if 'segments' in q]
    if not concat:
        return _run_fc_features(pending)
    ops.fc_concat_act_bn_grouped(concat)
    rest = [q for q in pending if 'segments' not in q]
    done = dict(zip(map(id, rest), _run_fc_features(rest))) if rest else {}
    return [q['out'] if 'segments' in q else done[id(q)] for q in pending]


def _run_fc_features(pending):
    """fp32: one grouped GEMM.  fp16x3: oversized problems are cut into row chunks, then each problem goes to the strip form, the fused
    split or the materialised split: one launch per form that has problems."""
    if FC_PRECISION == 'fp32':
        return ops.fc_act_bn_grouped(pending)
    if FC_PRECISION != 'fp16x3':
        raise ValueError("FC_PRECISION must be 'fp32' or 'fp16x3'")
    strip, tiled = [], []
    for q in _row_chunks(pending):
        # 512-d inputs take the strip form (X stationary in registers: no row-scale pass, no split planes)
        (strip if q.get('strip') is not None and ops.fc_strip_eligible(q['x'], q['weight'].shape[0]) else tiled).append(q)
    # big launches with a narrow output take the fused split (inputs stay fp32 in HBM, split inside the GEMM: every column
    # tile of a row block repeats the conversion, 2x at D = 512 but 16x at D = 4096, where materialising the planes once is
    # cheaper: C5 33.2 ms fused vs 32.9 ms); small launches take the materialised split, whose 128x128 tiles fill the chip
    tiles = sum(((q['x'].shape[0] + 255) // 256) * ((q['weight_split'].N + 255) // 256) for q in tiled)
    fused = (tiles >= 512 and all(q['weight_split'].N <= 1024 for q in tiled) and
             all(ops.fused_split_eligible(q['x'], q['weight_split']) for q in tiled))
    outs = {}
    if strip:
        outs.update(zip(map(id, strip), ops.fc_act_bn_strip_grouped([dict(q, strip=q['strip']()) for q in strip])))
    if tiled:
        outs.update(zip(map(id, tiled), (ops.fc_act_bn_fused_grouped if fused else ops.fc_act_bn_split_grouped)(tiled)))
    return [outs[id(q)] if id(q) in outs else q['out'] for q in pending]      # a chunked problem: the chunks wrote its 'out'


def _initialize_weights(m):
    """Xavier init of Linear layers, identity BatchNorm (model/model.py:51-60)."""
    if type(m) == nn.Linear:
        nn.init.xavier_uniform_(m.weight)
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif type(m) == nn.BatchNorm1d:
        nn.init.ones_(m.weight)
        nn.init.zeros_(m.bias)


def to_device_and_float16(x):
    """model/model.py:63-67: despite its name the reference never casts to fp16."""
    return x.to(device=device, dtype=torch.float32)


def _eval_only(module):
    if module.training:
        raise NotImplementedError('laff_amd implements the inference path only; call .eval() '
                                  '(training is out of scope, SURVEY.md section 8f)')


# ------------------------------------------------------------------------------------------------------
# attention registry (model/model.py:70-208) -- only the variants on the path
# ------------------------------------------------------------------------------------------------------
_ATTENTION_1 = {  # name -> (with_ave, mul)   (model/model.py:94-97)
    'attention_noAverageMul_Ave': (True, False),
    'attention_noAveNoAverageMul': (False, False),
    'attention_averageMul': (True, True),
    'average_AverageMul_noAve': (False, True),
}


def get_attention_layer(attention_type, common_space_dim, encoder_num, opt):
    if attention_type in _ATTENTION_1:
        with_ave, mul = _ATTENTION_1[attention_type]
        return Attention_1(common_space_dim, with_ave=with_ave, mul=mul)
    if attention_type == 'just_average':
        return JustAverage()
    if attention_type == 'Multi_head_MyApply_Attention':
        heads = opt.multi_head_attention['heads']
        return Multi_head_MyApply_Attention(
            common_space_dim, heads, common_space_dim // heads,
            with_ave=opt.attention_param_each_head['with_ave'], mul=opt.attention_param_each_head['mul'],
            split_head=opt.attention_param_each_head['split_head'], l2norm_each_head=opt.attention_l2norm)
    if attention_type == 'my_self_attention':       # multi_head + official self-attention, the baseline LAFF is compared with
        heads = opt.multi_head_attention['heads']
        return Multi_head_MyApply_selfAttention(
            common_space_dim, heads, common_space_dim // heads, opt.multi_head_attention['dropout'],
            output_type=opt.my_self_attention_output_type, encoder_num=encoder_num, l2norm_each_head=opt.attention_l2norm, opt=opt)
    raise NotImplementedError("attention type '%s' is an ablation variant outside the LAFF hot path" % attention_type)


# ------------------------------------------------------------------------------------------------------
# a1/a2: TransformNet
# ------------------------------------------------------------------------------------------------------
def use_device_norm(module, on=True):
    """Sets device_norm on every TransformNet under `module` (itself included): their training-mode dropout + BatchNorm1d stage then runs
    on laff_dropout_bn_train instead of torch's F.dropout and BatchNorm1d.  Returns module."""
    for m in module.modules():
        if isinstance(m, TransformNet):
            m.device_norm = bool(on)
    return module


class TransformNet(nn.Module):
    """fc -> activation -> dropout (identity in eval) -> BatchNorm1d, as one GEMM with a fused epilogue.  device_norm: in training mode
    the dropout + BatchNorm1d stage runs as one launch of this library each way (_DropoutBnFn) instead of torch's own ops."""

    def __init__(self, fc_layers, opt=None, dropout=None, batch_norm=None, activation=None, fc=True, device_norm=False):
        super().__init__()
        if opt is not None:
            if batch_norm is None:
                batch_norm = opt.batch_norm
            if activation is None:
                activation = opt.activation
            if dropout is None:
                dropout = opt.dropout
        self.fc1 = nn.Linear(fc_layers[0], fc_layers[1]) if fc else None
        self.bn1 = nn.BatchNorm1d(fc_layers[1]) if batch_norm else None
        self.activation_name = activation if activation in ('tanh', 'relu', 'sigmoid') else None
        self.dropout_p = dropout if (dropout is not None and dropout > 1e-3) else None
        self.out_features = fc_layers[1]
        self.device_norm = bool(device_norm)
        self._derived = {}
        self.apply(_initialize_weights)

    def _cached(self, slot, tensors, make, extra=()):
        """What make() returned at the last call for `slot`, as long as no tensor of `tensors` (None entries are skipped) has a new
        data_ptr or a bumped _version and `extra` is the same; else make() now.  Every value derived from parameters is kept this way:
        an in-place update, an optimizer step, .to(device) and load_state_dict all show in one of the two."""
        key = tuple((t.data_ptr(), t._version) for t in tensors if t is not None) + extra
        hit = self._derived.get(slot)
        if hit is None or hit[0] != key:
            hit = self._derived[slot] = (key, make())
        return hit[1]

    def _bn_tensors(self):
        bn = self.bn1
        return () if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)

    def _bn_fold(self):
        bn = self.bn1
        scale = (bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)).contiguous()
        return scale, (bn.bias.detach() - bn.running_mean * scale).contiguous()

    def bn_affine(self, extra_shift=None):
        """Folded eval-mode BatchNorm1d: y*scale + shift (what aten's inference kernel computes)."""
        if self.bn1 is None:
            if extra_shift is None:
                return None, None
            return torch.ones_like(extra_shift), extra_shift.contiguous()
        scale, shift = self._cached('bn_affine', self._bn_tensors(), self._bn_fold)
        if extra_shift is not None:
            shift = (shift + extra_shift).contiguous()
        return scale, shift

    def weight_t(self):
        """fc1.weight transposed ([D_k, D]: one vocabulary entry = one contiguous row), cached until the weight changes."""
        w = self.fc1.weight
        return self._cached('weight_t', (w,), lambda: w.detach().t().contiguous())

    def weight_t_block(self, col, width):
        """Columns [col, col + width) of fc1.weight transposed ([width, D]): the block a sparse segment of a concat tower gathers from,
        cached until the weight changes."""
        w = self.fc1.weight
        blocks = self._cached('weight_t_blocks', (w,), dict)
        if (col, width) not in blocks:
            blocks[(col, width)] = w.detach()[:, col:col + width].t().contiguous()
        return blocks[(col, width)]

    def concat_problem(self, segments, pending=None):
        """This layer applied to torch.cat(segments, dim=1) without forming it (laff_fc_concat_act_bn): queued on `pending` for the
        caller's run_fc(), or run now.  segments: dense fp32 matrices and / or torch.sparse_csr ones, in column order.  Always fp32
        arithmetic, also with FC_PRECISION == 'fp16x3'.  Returns the (N, D) output (filled once the launch has run)."""
        _eval_only(self)
        segs, wt, col = [], {}, 0
        for j, x in enumerate(segments):
            if x.layout == torch.sparse_csr:
                x = x.to(device)
                wt[j] = self.weight_t_block(col, x.shape[1])
            else:
                x = to_device_and_float16(x)
            segs.append(x)
            col += x.shape[1]
        if col != self.fc1.in_features:
            raise ValueError('the concatenated input has %d columns, fc1 takes %d' % (col, self.fc1.in_features))
        scale, shift = self.bn_affine(None)
        out = torch.empty((segs[0].shape[0], self.out_features), device=segs[0].device, dtype=torch.float32)
        prob = dict(segments=segs, weight=self.fc1.weight.detach(), weight_t=wt,
                    bias=self.fc1.bias.detach() if self.fc1.bias is not None else None,
                    bn_scale=scale, bn_shift=shift, activation=self.activation_name, out=out)
        if pending is None:
            run_fc([prob])
        else:
            pending.append(prob)
        return out

    def weight_split(self):
        """fp16 hi/lo split of fc1.weight for FC_PRECISION == 'fp16x3', cached until the weight changes."""
        if FC_PRECISION != 'fp16x3':
            return None
        w = self.fc1.weight
        return self._cached('weight_split', (w,), lambda: ops.split_rows(w.detach()))

    def strip_weights(self):
        """fc1 + folded BatchNorm + activation packed for the strip-form FC (laff_fc_strip_pack), cached until a parameter changes."""
        w, b = self.fc1.weight, self.fc1.bias
        return self._cached('strip_weights', (w, b) + self._bn_tensors(),
                            lambda: ops.fc_strip_pack(w.detach(), None if b is None else b.detach(), *self.bn_affine(None),
                                                      self.activation_name),
                            (self.activation_name, ops.fc_strip_mfma(w.device)))

    def _forward_train(self, x, heads=1, extra_shift=None):
        """Training mode: fc1 + activation under autograd (_FcActFn), then torch's own dropout and training-mode BatchNorm1d (batch
        statistics, running-stat updates), each a single elementwise / column pass with its own autograd.  What has no backward here
        is refused by name.  Without an fc (the no-transform feature) there is a path with device_norm only: _forward_train_no_fc."""
        if self.fc1 is None and self.device_norm:
            return self._forward_train_no_fc(x, heads, extra_shift)
        if self.fc1 is None:
            raise NotImplementedError('training mode: a TransformNet without fc (fc=False%s) has no differentiable path; apply its '
                                      'BatchNorm upstream as a torch op' % (', tiled over %d heads' % heads if heads > 1 else ''))
        if x.layout != torch.strided and not (x.layout == torch.sparse_csr and x.is_cuda):
            raise NotImplementedError('training mode: a sparse (CSR) input is projected on the device only (laff_fc_gather_act_bn and '
                                      'laff_fc_gather_backward have no CPU path): move it to the device first')
        if extra_shift is not None:
            raise NotImplementedError('training mode: extra_shift (the expert embedding) is not differentiable here; add it upstream '
                                      'as a torch op')
        self._device_norm_supported()
        if x.layout == torch.sparse_csr:
            y = _FcGatherFn.apply(x, self.fc1.weight, self.fc1.bias, self.weight_t(), self.activation_name)
        else:
            y = _FcActFn.apply(x, self.fc1.weight, self.fc1.bias, self.activation_name)
        return self._after_activation_train(y)

    def _forward_train_no_fc(self, x, heads, extra_shift):
        """Training mode of the no-transform feature with device_norm: BatchNorm1d on batch statistics over x, or over x tiled `heads`
        times (x.repeat(1, heads), never formed: _TileBnFn, one launch each way, x receives its gradient summed over the heads).  An
        input of the layer's own width -- heads == 1, or forward() on a pre-repeated input -- takes _DropoutBnFn like an fc's output."""
        if extra_shift is not None:
            raise NotImplementedError('training mode: extra_shift (the expert embedding) is not differentiable here; add it upstream '
                                      'as a torch op')
        if self.activation_name is not None:
            raise NotImplementedError('activation without fc is never built by the reference towers')
        self._device_norm_supported()
        if x.layout != torch.strided or x.dim() != 2:
            raise NotImplementedError('training mode: a TransformNet without fc takes a dense 2-D feature, got layout %s with %d '
                                      'dimensions' % (x.layout, x.dim()))
        if not (heads > 1 and x.shape[1] * heads == self.out_features):
            if x.shape[1] != self.out_features:
                raise ValueError('a TransformNet without fc of width %d takes that width, or 1 / %d of it tiled over the heads; got %d '
                                 'columns' % (self.out_features, heads, x.shape[1]))
            return self._after_activation_device(x)
        bn = self.bn1
        if bn is None:
            raise NotImplementedError('training mode: a tiled TransformNet without fc and without BatchNorm is a plain repeat; the '
                                      'reference towers never build it')
        if self.dropout_p is not None:
            raise NotImplementedError('training mode: dropout (p=%g) on a TransformNet without fc tiled over %d heads is refused: the '
                                      'mask would differ per copy, and the reference never sets it' % (self.dropout_p, heads))
        y = _TileBnFn.apply(x, heads, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
        self._running_stats_written()
        return y

    def _running_stats_written(self):
        """A kernel wrote bn1's running statistics through raw pointers: their version counters are bumped here, or bn_affine's cache
        would serve the statistics of before the step to the next .eval() forward.  num_batches_tracked counts the forward, as torch
        does."""
        bn = self.bn1
        torch.autograd.graph.increment_version(bn.running_mean)
        torch.autograd.graph.increment_version(bn.running_var)
        bn.num_batches_tracked.add_(1)

    def _device_norm_supported(self):
        """device_norm: the BatchNorm1d settings that laff_dropout_bn_train does not compute are refused by name, before any launch."""
        bn = self.bn1
        if not self.device_norm or bn is None:
            return
        if bn.momentum is None:
            raise NotImplementedError('training mode with device_norm: bn1.momentum=None (a cumulative moving average) is not '
                                      'computed by laff_dropout_bn_train; set a momentum or device_norm=False')
        if not bn.affine:
            raise NotImplementedError('training mode with device_norm: bn1 with affine=False is not computed by '
                                      'laff_dropout_bn_train; set device_norm=False')
        if not bn.track_running_stats:
            raise NotImplementedError('training mode with device_norm: bn1 with track_running_stats=False is not computed by '
                                      'laff_dropout_bn_train; set device_norm=False')

    def _after_activation_train(self, y):
        if self.device_norm:
            return self._after_activation_device(y)
        if self.dropout_p is not None:
            y = F.dropout(y, self.dropout_p, training=True)
        return y if self.bn1 is None else self.bn1(y)

    def _after_activation_device(self, y):
        """The same stage as one launch each way (_DropoutBnFn)."""
        bn = self.bn1
        if bn is None:
            return y if self.dropout_p is None else _DropoutBnFn.apply(y, None, None, None, None, self.dropout_p, 0.0, 0.0)
        y = _DropoutBnFn.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.dropout_p, bn.momentum, bn.eps)
        self._running_stats_written()
        return y

    def concat_train(self, segments, grouped=False):
        """Training mode: this layer applied to torch.cat(segments, dim=1) without forming it, under autograd (_FcConcatFn), then
        torch's dropout and training-mode BatchNorm1d as in _forward_train.  segments: dense fp32 device matrices and / or device
        torch.sparse_csr ones, in column order; a dense segment that requires a gradient receives one.  concat_problem stays the
        inference path.  grouped: the backward is one ops.fc_concat_backward call (_FcConcatGroupedFn) instead of one call per
        segment -- the route of the W2VV++ towers."""
        if not self.training:
            raise RuntimeError('concat_train is the training-mode path; in eval mode use concat_problem')
        if self.fc1 is None:
            raise NotImplementedError('training mode: a TransformNet without fc (fc=False) has no differentiable path')
        self._device_norm_supported()
        segments = list(segments)
        for j, x in enumerate(segments):
            if not x.is_cuda or x.layout not in (torch.strided, torch.sparse_csr) or x.dim() != 2:
                raise NotImplementedError('training mode: segment %d must be a 2-D dense or sparse (CSR) matrix on the device' % j)
        col = sum(x.shape[1] for x in segments)
        if col != self.fc1.in_features:
            raise ValueError('the concatenated input has %d columns, fc1 takes %d' % (col, self.fc1.in_features))
        fn = _FcConcatGroupedFn if grouped else _FcConcatFn
        return self._after_activation_train(fn.apply(self, self.activation_name, self.fc1.weight, self.fc1.bias, *segments))

    def plane(self, x, heads=1, extra_shift=None, pending=None, head_dim=None):
        """(src, tile, scale, shift) for laff_fuse.  With an FC the projection either runs now or, when `pending`
        (a list) is given, is appended to it so that the caller launches all features' GEMMs as one grouped kernel.
        In training mode the projection runs at once under autograd (`pending` is not used) and the plane is plain and dense."""
        if self.training:
            return (self._forward_train(x, heads, extra_shift), False, None, None)
        scale, shift = self.bn_affine(extra_shift)
        if self.fc1 is not None and x.layout == torch.sparse_csr:
            # sparse feature (bag-of-words): gather-sum of columns of W instead of a dense N x |vocab| x D GEMM
            bias = self.fc1.bias.detach() if self.fc1.bias is not None else None
            if pending is not None and head_dim is not None and head_dim <= 512:
                # tower path: the gather runs INSIDE the fuse launch (the projected plane is never written / re-read)
                return (None, False, scale, shift, self.activation_name, (x.to(device), self.weight_t(), bias))
            y = ops.fc_gather_act_bn(x.to(device), self.weight_t(), bias, scale, shift, self.activation_name)
            return (y, False, None, None)
        x = to_device_and_float16(x)
        if self.fc1 is not None:
            prob = dict(x=x, weight=self.fc1.weight.detach(), weight_split=self.weight_split(),
                        bias=self.fc1.bias.detach() if self.fc1.bias is not None else None,
                        bn_scale=scale, bn_shift=shift, activation=self.activation_name)
            if (FC_PRECISION == 'fp16x3' and extra_shift is None and
                    self.fc1.in_features == 512 and self.out_features % 32 == 0):
                prob['strip'] = self.strip_weights        # packed lazily: only if the launch takes the strip form
            if pending is None:
                return (run_fc([prob])[0], False, None, None)
            y = prob['out'] = torch.empty((x.shape[0], self.out_features), device=x.device, dtype=torch.float32)
            pending.append(prob)
            return (y, False, None, None)
        if self.activation_name is not None:
            raise NotImplementedError('activation without fc is never built by the reference towers')
        tile = heads > 1 and x.shape[1] * heads == self.out_features
        return (x, tile, scale, shift)

    def forward(self, input_x):
        if self.training:
            return self._forward_train(input_x)
        src, tile, scale, shift = self.plane(input_x)[:4]
        if scale is None and not tile:
            return src
        out = ops.fuse([(src, tile, scale, shift)], 1, src.shape[1], None, None, None,
                       ops.attention_flags(just_average=True))
        return out.view(out.shape[0], -1)


class VisTransformNet(TransformNet):
    """The W2VV++ video tower (model/model.py:279-308): one TransformNet over the concatenated video features.  The features stay
    where they are: each is a segment of the K loop of one laff_fc_concat_act_bn launch."""

    def __init__(self, opt):
        super().__init__((int(np.sum(list(opt.vis_fc_layers[0].values()))), opt.vis_fc_layers[1]), opt)

    def prepare(self, vis_input, vis_frame_feat_dict_input=None, pending=None):
        """Queue the projection on `pending`; returns the closure that hands the embeddings over once run_fc() has run.  In training
        mode the route is open only once the owning model's enable_training() has armed the tower (training_armed): the projection then
        runs at once under autograd (_concat_tower_train) and the closure holds the differentiable embeddings."""
        segments = list(vis_input.values()) if isinstance(vis_input, dict) else [vis_input]     # dict order, as torch.cat(list(...))
        if self.training and getattr(self, 'training_armed', False):
            emb = _concat_tower_train(self, self, segments, grouped=True)
            return lambda: emb
        out = self.concat_problem(segments, pending)
        return lambda: out

    def forward(self, vis_input, txt_emb=None, vis_frame_feat_dict_input=None):
        return self.prepare(vis_input)()


def _concat_tower_train(tower, layer, segments, grouped):
    """The training route of a W2VV++ concat tower: its segments through layer.concat_train.  Dense segments
    go to the device as fp32; a CSR one that is on the device already is handed on as the object it is (it may carry its laff_csc).
    grouped: the backward is the one laff_fc_concat_backward call.  The video tower takes it; the text tower keeps the per-segment
    calls, which measured faster at its mix of a wide aligned segment, a CSR one and a narrow unaligned one (section 4.30)."""
    _train_on_device(tower)
    segs = []
    for x in segments:
        if x.layout != torch.sparse_csr:
            x = to_device_and_float16(x)
        elif not x.is_cuda:
            x = x.to(device)
        segs.append(x)
    return layer.concat_train(segs, grouped=grouped)


# ------------------------------------------------------------------------------------------------------
# a3/a4: video tower of 'LAFF' / 'w2vpp_mutivis_attention'
# ------------------------------------------------------------------------------------------------------
def _expert_rows(embedding, n):
    return None if embedding is None else embedding.weight.detach()[:n]


class _recording:
    """attention layers store their softmax weights (the reference's `self.weights`) only while this is active: on the tower path
    it is an extra store per launch that nobody but get_attention_weight() reads"""

    def __init__(self, *layers):
        self.layers = layers

    def __enter__(self):
        for l in self.layers:
            l.record_weights = True

    def __exit__(self, *a):
        for l in self.layers:
            l.record_weights = False


def _fuse(attention_layer, planes, heads, l2norm_planes=False):
    if hasattr(attention_layer, 'fuse_planes'):
        if l2norm_planes:
            return attention_layer.fuse_planes(planes, heads, l2norm_planes=True)
        return attention_layer.fuse_planes(planes, heads)
    raise NotImplementedError('attention layer %s is outside the LAFF hot path' % type(attention_layer).__name__)


def _train_on_device(module):
    """The towers' training routes run on the device only: a model on the CPU is refused by name before its first layer is reached."""
    p = next(module.parameters(), None)
    if p is not None and not p.is_cuda:
        raise NotImplementedError('training mode: the towers train on the device only (laff_amd has no CPU path); move the model to the '
                                  'GPU, or call .eval()')


def _fuse_train(attention_layer, planes, heads, expert_embedding, l2norm):
    """Training mode: the planes of a tower (plain and dense, as plane() hands them over under autograd) through its fusion block.
    Without experts and without l2norm they go to fuse_planes; with either they pass the expert stage in one launch each way
    (_ExpertStageFn: the expert table receives its gradient) and the block reads the stacked result in place."""
    if expert_embedding is None and not l2norm:
        return _fuse(attention_layer, planes, heads)
    srcs = [ops.dense_plane(p, i) for i, p in enumerate(planes)]
    expert = None if expert_embedding is None else expert_embedding.weight[:len(srcs)]
    return attention_layer(_ExpertStageFn.apply(bool(l2norm), expert, *srcs))


def _materialise(plane, heads, D):
    src, tile, scale, shift = plane[:4]
    act = plane[4] if len(plane) > 4 else None
    if scale is None and not tile and act is None:
        return src
    H = heads if tile else 1
    out = ops.fuse([plane], H, D // H, None, None, None, ops.attention_flags(just_average=True))
    return out.view(out.shape[0], D)


class VisMutiTransformNet(nn.Module):
    def __init__(self, opt, space_dict):
        super().__init__()
        if opt is None:
            return
        self.opt = opt
        self.vis_net_space_dict = space_dict
        self.common_space_dim = opt.vis_fc_layers[1]
        for each in space_dict.keys():
            if each not in opt.vis_no_transform:
                self.add_module(each, TransformNet((space_dict[each], opt.vis_fc_layers[1]), opt))
            else:
                self.add_module(each, TransformNet((space_dict[each], opt.vis_fc_layers[1]), None, dropout=None,
                                                   batch_norm=True, activation=False, fc=False))

    def planes(self, vis_input, expert=None, pending=None):
        if self.opt.vis_feat_add_concat and 'vis_feat_add_concat' not in vis_input:
            vis_input['vis_feat_add_concat'] = torch.cat([to_device_and_float16(v) for v in vis_input.values()], dim=1)
        heads = self.opt.multi_head_attention['heads']
        module_dict = dict(self.named_children())
        out = []
        for i, name in enumerate(self.vis_net_space_dict.keys()):
            vis_input[name] = to_device_and_float16(vis_input[name])     # in-place like the reference (:1817)
            h = heads if name in self.opt.vis_no_transform else 1
            out.append(module_dict[name].plane(vis_input[name], h, None if expert is None else expert[i], pending))
        return out

    def forward(self, vis_input, txt_emb=None, vis_frame_feat_dict_input=None):
        heads = self.opt.multi_head_attention['heads']
        pending = []
        planes = self.planes(vis_input, pending=pending)
        run_fc(pending)
        return {name: _materialise(p, heads, self.common_space_dim)
                for name, p in zip(self.vis_net_space_dict.keys(), planes)}


class VisMutiTransformNetAddAttnetion(nn.Module):
    def __init__(self, opt, space_dict):
        super().__init__()
        if opt is None:
            return
        self.opt = opt
        self.vis_net_space_dict = space_dict
        self.common_space_dim = opt.vis_fc_layers[1]
        self.VisMutiTransformNet = VisMutiTransformNet(opt, space_dict)
        self.attention_layer = get_attention_layer(self.opt.vis_attention, self.common_space_dim, len(space_dict), self.opt)
        self.expert_embedding = None
        self.expert_l2Norm = False
        if opt.vis_expert_embedding['expert']:
            self.expert_embedding = nn.Embedding(len(self.vis_net_space_dict), self.common_space_dim)
        if opt.vis_expert_embedding['l2norm']:
            self.expert_l2Norm = True          # l2norm(local_embs, dim=2) before the attention (model/model.py:1855-1856, 1872-1873)

    def prepare(self, vis_input, vis_frame_feat_dict_input=None, pending=None):
        """Queue this tower's FC projections on `pending`; returns the closure that fuses once they have run.  In training mode the
        projections run at once under autograd (`pending` is not used) and the closure holds the differentiable embeddings."""
        heads = self.opt.multi_head_attention['heads']
        if self.training:
            _train_on_device(self)
            emb = _fuse_train(self.attention_layer, self.VisMutiTransformNet.planes(vis_input), heads, self.expert_embedding,
                              self.expert_l2Norm)
            return lambda: emb
        planes = self.VisMutiTransformNet.planes(vis_input, _expert_rows(self.expert_embedding, len(self.vis_net_space_dict)),
                                                 pending)
        return lambda: _fuse(self.attention_layer, planes, self.opt.multi_head_attention['heads'], self.expert_l2Norm)

    def forward(self, vis_input, txt_emb=None, vis_frame_feat_dict_input=None):
        pending = []
        finish = self.prepare(vis_input, pending=pending)
        run_fc(pending)
        return finish()

    def get_attention_weight(self, vis_input, txt_emb=None):
        with _recording(self.attention_layer):
            self.forward(vis_input, txt_emb)
        return self.attention_layer.get_attention_weight()


# ------------------------------------------------------------------------------------------------------
# text tower
# ------------------------------------------------------------------------------------------------------
class PreExtractedEncoder(nn.Module):
    """Returns a pre-extracted text feature matrix from the caption dict (the reference's own convention for
    frozen CLIP, model/model.py:497-498, extended to every text feature)."""

    def __init__(self, key):
        super().__init__()
        self.key = key

    def forward(self, caption_feat_dict, task3=False):
        if self.key not in caption_feat_dict:
            raise KeyError("caption_feat_dict lacks '%s': text features are pre-extracted on this path; plug an encoder "
                           "module into txt_net.encoder to compute them on the fly" % self.key)
        return {'text_features': caption_feat_dict[self.key]}


ENCODER_KEYS = {'rnn_encoder': 'rnn_encoding', 'bert_encoder': 'bert_encoding', 'bow_encoder': 'bow_encoding',
                'w2v_encoder': 'w2v_encoding', 'CLIP_encoder': 'CLIP_encoding', 'NetVLAD_encoder': 'NetVLAD_encoding'}


def _build_text_encoders(module, opt, keys=ENCODER_KEYS):
    """What both text encoder classes hold: `space_dict` (encoder name -> feature width) in the reference's fixed order (model/model.py:
    572-613: rnn, bert, bow, w2v, CLIP, NetVLAD), the `encoder` module of PreExtractedEncoder placeholders, `encoder_name_list` and
    `txt_encoder_num`."""
    te = opt.text_encoding
    rnn = te['rnn_encoding']['name'].split('_', 1)[0]
    module.space_dict = {}
    if rnn == 'gru':
        module.space_dict['rnn_encoder'] = opt.rnn_size
    elif rnn == 'bigru':
        module.space_dict['rnn_encoder'] = opt.rnn_size * 2
    if te['bert_encoding']['name'] != 'noBert':
        module.space_dict['bert_encoder'] = opt.bert_size
    if 'no' not in te['bow_encoding']['name']:
        module.space_dict['bow_encoder'] = opt.t2v_bow.ndims
    if 'no' not in te['w2v_encoding']['name']:
        module.space_dict['w2v_encoder'] = opt.t2v_w2v.ndims
    if 'no' not in te['CLIP_encoding']['name']:
        module.space_dict['CLIP_encoder'] = opt.clip_opt['size']
    if 'no' not in te['NetVLAD_encoding']['name']:
        module.space_dict['NetVLAD_encoder'] = opt.t2v_w2v.ndims * opt.NetVLAD_opt['num_clusters']
    module.encoder = nn.Module()
    for name in module.space_dict:
        module.encoder.add_module(name, PreExtractedEncoder(keys[name]))
    module.encoder_name_list = list(module.space_dict.keys())
    module.txt_encoder_num = len(module.encoder_name_list)


class MultiScaleTxtEncoder(nn.Module):
    """The text encoders of the W2VV++ tower (model/model.py:552-700) under `encoder.<name>`, in the reference's fixed order rnn,
    bert, bow, w2v, CLIP, NetVLAD: PreExtractedEncoder placeholders, replaced by plugging a module that returns
    {'text_features': tensor} (laff_amd.txt2vec, clip_text, bert_text) into `encoder.<name>`.  A sparse-CSR bow feature stays sparse.
    (NetVLAD: the width is w2v dims x clusters, what the encoder emits; the reference's space_dict entry lacks the cluster factor.)"""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        _build_text_encoders(self, opt)

    def segments(self, caption_feat_dict, task3=False):
        """The encoders' outputs in encoder order: the segments of the concatenated text feature."""
        out = []
        for name in self.encoder_name_list:
            feats = getattr(self.encoder, name)(caption_feat_dict, task3=task3)['text_features']
            if feats.shape[1] != self.space_dict[name]:
                raise ValueError("text feature '%s' has %d columns, the config says %d" % (name, feats.shape[1], self.space_dict[name]))
            out.append(feats)
        return out

    def forward(self, caption_feat_dict, task3=False):
        """The concatenated feature itself, as the reference returns it (the tower does not go through this: MultiScaleTxtNet)."""
        return torch.cat([to_device_and_float16(f.to_dense() if f.layout == torch.sparse_csr else f)
                          for f in self.segments(caption_feat_dict, task3)], dim=1)


class MultiScaleTxtNet(nn.Module):
    """The W2VV++ text tower (model/model.py:703-726): `encoder` + one TransformNet `transformer` over the concatenated features,
    run as one segmented launch (laff_fc_concat_act_bn).  Sets opt.txt_fc_layers[0] to the summed width like the reference."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.encoder = MultiScaleTxtEncoder(opt)
        self.opt.txt_fc_layers[0] = int(sum(self.encoder.space_dict.values()))
        self.transformer = TransformNet(opt.txt_fc_layers, opt, opt.dropout, opt.batch_norm, opt.activation)

    def prepare(self, caption_feat_dict, pending=None, task3=False):
        """As VisTransformNet.prepare; an armed tower in training mode hands the encoders' segments to the layer's training route (the
        per-segment backward, _concat_tower_train): a device CSR bag of words stays sparse (with its laff_csc), a differentiable
        encoder's output receives its gradient."""
        if self.training and getattr(self, 'training_armed', False):
            emb = _concat_tower_train(self, self.transformer, self.encoder.segments(caption_feat_dict, task3), grouped=False)
            return lambda: emb
        out = self.transformer.concat_problem(self.encoder.segments(caption_feat_dict, task3), pending)
        return lambda: out

    def forward(self, caption_feat_dict, visual_emb=None, task3=False):
        return self.prepare(caption_feat_dict, task3=task3)()


class MultiScaleTxtEncoderAttention(nn.Module):
    ENCODER_KEYS = ENCODER_KEYS

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        _build_text_encoders(self, opt, self.ENCODER_KEYS)

        # transform layers (model/model.py:622-681)
        D = opt.txt_fc_layers[1]
        self.transform_layer = nn.Module()
        for name in ('rnn_encoder', 'bert_encoder', 'w2v_encoder', 'bow_encoder', 'CLIP_encoder', 'NetVLAD_encoder'):
            if name not in self.space_dict:
                continue
            dims = (self.space_dict[name], D)
            if name == 'bert_encoder':
                t = TransformNet(dims, None, opt.bert_transform_dropout, opt.bert_transform_batch_norm,
                                 opt.bert_transform_activation)
            elif name == 'CLIP_encoder':
                co = opt.clip_opt
                if 'CLIP_encoder' in opt.txt_no_transform:
                    t = TransformNet(dims, None, co['transform_dropout'], co['transform_batch_norm'], False, False)
                else:
                    t = TransformNet(dims, None, co['transform_dropout'], co['transform_batch_norm'],
                                     co['transform_activation'])
            else:
                t = TransformNet(dims, None, opt.dropout, opt.batch_norm, opt.activation)
            self.transform_layer.add_module(name + '_transform', t)
        self.attention_layer = get_attention_layer(opt.txt_attention, D, self.txt_encoder_num, opt)

        self.expert_embedding = None
        if opt.txt_expert_embedding['expert']:
            self.expert_embedding = nn.Embedding(len(self.space_dict), D)
        self.txt_expert_l2Norm = bool(opt.txt_expert_embedding['l2norm'])      # model/model.py:1660-1661, 1693-1694

    def _prepare_train(self, caption_feat_dict, task3):
        """Training mode: every encoder's feature through its transform layer under autograd (a device CSR feature takes the gather
        route, an encoder that is itself differentiable receives its gradient), then the fusion through _fuse_train."""
        heads = self.opt.multi_head_attention['heads']
        planes = []
        for name in self.encoder_name_list:
            feats = getattr(self.encoder, name)(caption_feat_dict, task3=task3)['text_features']
            if feats.layout != torch.sparse_csr:
                feats = to_device_and_float16(feats)
            elif not feats.is_cuda:                         # (a device CSR is handed on as the object it is: it may carry its laff_csc)
                feats = feats.to(device)
            h = heads if name in self.opt.txt_no_transform else 1
            planes.append(getattr(self.transform_layer, name + '_transform').plane(feats, h))
        return _fuse_train(self.attention_layer, planes, heads, self.expert_embedding, self.txt_expert_l2Norm)

    def prepare(self, caption_feat_dict, pending=None, task3=False):
        if self.training:
            _train_on_device(self)
            emb = self._prepare_train(caption_feat_dict, task3)
            return lambda: emb
        heads = self.opt.multi_head_attention['heads']
        expert = _expert_rows(self.expert_embedding, len(self.encoder_name_list))
        planes = []
        for i, name in enumerate(self.encoder_name_list):
            feats = getattr(self.encoder, name)(caption_feat_dict, task3=task3)['text_features']
            h = heads if name in self.opt.txt_no_transform else 1
            planes.append(getattr(self.transform_layer, name + '_transform').plane(
                feats, h, None if expert is None else expert[i], pending, head_dim=self.opt.txt_fc_layers[1] // heads
                if type(self.attention_layer).__name__ == 'Multi_head_MyApply_Attention' and
                self.attention_layer.split_head and not self.txt_expert_l2Norm else None))     # (a row norm needs the projected plane)
        return lambda: _fuse(self.attention_layer, planes, heads, self.txt_expert_l2Norm)

    def forward(self, caption_feat_dict, visual_emb=None, task3=False):
        pending = []
        finish = self.prepare(caption_feat_dict, pending, task3)
        run_fc(pending)
        return finish()

    def get_attention_weight(self, caption_feat_dict, visual_emb=None):
        with _recording(self.attention_layer):
            self.forward(caption_feat_dict, visual_emb)
        return self.attention_layer.get_attention_weight()


# ------------------------------------------------------------------------------------------------------
# a7: FrameLAFF video tower
# ------------------------------------------------------------------------------------------------------
class VisMutiTransformNetPlusFrameFeat(nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        # One TransformNet per input feature under the feature's own name (the state_dict keys of the reference: model/model.py:
        # 2101-2128): video-level features and, with frame_feat_input, the per-frame ones (pooled over frames first, frame_vector).
        # A feature listed in vis_no_transform keeps its width: BatchNorm only, no FC, no activation.
        dims = opt.vis_fc_layers[0]
        names = list(dims.keys())
        if opt.frame_feat_input:
            names += [f for f in opt.vid_frame_feats if f not in dims]
        D_out = opt.vis_fc_layers[1]
        self.vis_net_space_dict = space_dict = {f: opt.vis_fc_layers[0][f] for f in names}
        for f, width in space_dict.items():
            if f in opt.vis_no_transform:
                net = TransformNet((width, D_out), None, dropout=None, batch_norm=True, activation=False, fc=False)
            else:
                net = TransformNet((width, D_out), opt)
            self.add_module(f, net)
        D = opt.vis_fc_layers[1]
        self.vis_attention_layer = get_attention_layer(opt.vis_attention, D, len(space_dict), opt)
        self.frame_attention = nn.ModuleDict()
        for each in opt.vid_frame_feats:
            fd = opt.vis_fc_layers[0][each]
            att = get_attention_layer(opt.vis_frame_attention, fd, 1, opt)
            if not isinstance(att, Attention_1):
                raise NotImplementedError('frame attention must be an Attention_1 variant on this path')
            if opt.vis_frame_addFC:
                self.frame_attention[each] = nn.Sequential(nn.Linear(fd, fd), att)
            else:
                self.frame_attention[each] = nn.Sequential(att)

    def frame_vector(self, feat_name, frames, mask_tensor):
        """(B, Fmax, d) zero-padded frames -> (B, d): Attention_1 over frames for every video in one launch.

        Replaces the per-sample Python loop of model/model.py:2167-2173.  The reference's mask slice is a no-op, so
        padded frames take part in softmax / mean; without a frame FC they are exact zeros and are accounted for
        analytically from `lens`; with vis_frame_addFC the Linear turns them into the bias vector and all Fmax
        frames are processed.

        In training mode the method is differentiable: the frame Linear runs under _FcActFn, the attention
        under Attention_1.fuse_frames, so the frames, the Linear and the attention's embedding_common receive gradients."""
        seq = self.frame_attention[feat_name]
        att = seq[-1]
        frames = to_device_and_float16(frames).contiguous()
        B, Fmax, d = frames.shape
        lens = None
        if len(seq) == 2:
            fc = seq[0]
            if self.training:
                frames = _FcActFn.apply(frames.view(B * Fmax, d), fc.weight, fc.bias, None).view(B, Fmax, d)
            else:
                frames = ops.fc_act_bn(frames.view(B * Fmax, d), fc.weight.detach(), fc.bias.detach()).view(B, Fmax, d)
        else:
            lens = mask_tensor.to(device=frames.device).sum(dim=1).to(torch.int32).contiguous()
        return att.fuse_frames(frames, lens)

    def forward(self, vis_input, vis_frame_feat_dict_input, txt_emb=None):
        pending = []
        finish = self.prepare(vis_input, vis_frame_feat_dict_input, pending)
        run_fc(pending)
        return finish()

    def prepare(self, vis_input, vis_frame_feat_dict_input=None, pending=None):
        """In training mode the route is open only once the owning model's enable_training() has armed the tower (training_armed): a
        tower built on its own keeps the inference-only refusal.  Armed, every frame feature goes through frame_vector (differentiable),
        the projections run at once under autograd (`pending` is not used) and the closure holds the differentiable embeddings."""
        train = self.training
        if train and not getattr(self, 'training_armed', False):
            _eval_only(self)
        if train:
            _train_on_device(self)
            pending = None
        if self.opt.frame_feat_with_video_feat is False:
            vis_input = {}
        names = [k for k in vis_frame_feat_dict_input if k != 'mask_tensor']
        for feat_name in names:
            vis_frame_feat_dict_input[feat_name] = to_device_and_float16(vis_frame_feat_dict_input[feat_name])
        shapes = {tuple(vis_frame_feat_dict_input[k].shape) for k in names}
        if not train and len(names) > 1 and len(shapes) == 1 and not self.opt.vis_frame_addFC:
            # every frame feature of the tower in ONE launch (same shape, same attention type, shared lens)
            frames = [vis_frame_feat_dict_input[k].contiguous() for k in names]
            mask = vis_frame_feat_dict_input['mask_tensor'].to(device=frames[0].device)
            lens = None
            if mask.dtype != torch.float32 or mask.dim() != 2 or mask.stride(1) != 1:
                lens, mask = mask.sum(dim=1).to(torch.int32).contiguous(), None      # (any other mask type: the framework sums it)
            atts = [self.frame_attention[k][-1] for k in names]
            params = []
            for att in atts:
                w, b, gw = att._params()
                params.append((w.reshape(-1), b, gw))
            # (a float mask goes to the launch as it is: the launch takes lens = mask.sum(dim=1) itself)
            vecs = ops.frame_fuse_grouped(frames, lens, params, ops.attention_flags(atts[0].with_ave, atts[0].mul), mask=mask)
            for k, v in zip(names, vecs):
                vis_input[k] = v
        else:
            for feat_name in names:
                vis_input[feat_name] = self.frame_vector(feat_name, vis_frame_feat_dict_input[feat_name],
                                                         vis_frame_feat_dict_input['mask_tensor'])
        heads = self.opt.multi_head_attention['heads']
        module_dict = dict(self.named_children())
        planes = []
        for name in vis_input.keys():
            vis_input[name] = to_device_and_float16(vis_input[name])
            h = heads if name in self.opt.vis_no_transform else 1
            planes.append(module_dict[name].plane(vis_input[name], h, None, pending))
        if train:
            emb = _fuse(self.vis_attention_layer, planes, heads)
            return lambda: emb
        return lambda: _fuse(self.vis_attention_layer, planes, heads)

    def get_attention_weight(self, vis_input, vis_frame_feat_dict_input):
        self.forward(vis_input, vis_frame_feat_dict_input)
        name = [k for k in vis_frame_feat_dict_input.keys() if k != 'mask_tensor'][0]
        return self.frame_attention[name][-1].get_attention_weight()


# ------------------------------------------------------------------------------------------------------
# a9-a11: the cross-modal model
# ------------------------------------------------------------------------------------------------------
class W2VVPP(nn.Module):
    """The reference's W2VVPP family (model/model.py:791-1128): the inference surface, and the training step (enable_training, forward)
    for the LAFF towers and for the W2VV++ concat towers (section 4.30)."""

    #: operand precision of the similarity GEMM ('fp32' | 'fp16' | 'bf16' | 'fp16x3' | 'bf16x3')
    sim_precision = None

    def _init_vis_net(self, opt):
        self.vis_net = VisTransformNet(opt)

    def _init_txt_net(self, opt):
        if getattr(opt, 'txt_fc_same_with_vis_fc', False):
            raise NotImplementedError('txt_fc_same_with_vis_fc (one FC shared by both towers, model/model.py:764-768) is not supported')
        self.txt_net = MultiScaleTxtNet(opt)

    def __init__(self, opt):
        super().__init__()
        if opt is None:
            return
        self.opt = opt
        self._init_vis_net(opt)
        self._init_txt_net(opt)

    # -- the training step (model/model.py:791-1001, :1975-2048) ------------------------------------
    def _training_refusals(self):
        """What the step does not cover, by name, before any launch."""
        opt = self.opt
        if self._concat_towers():
            # the base class's compute_loss on 2-D embeddings (model/model.py:840-865): class W2VVPP, or W2VVPP_MutiVis with both concat
            if isinstance(self.vis_net, VisTransformNet) != isinstance(self.txt_net, MultiScaleTxtNet):
                raise NotImplementedError('training step: one concat tower beside one attention tower gives 2-D embeddings on one side and '
                                          'per-head ones on the other; the reference raises on the rank mismatch.  Make both towers '
                                          "'concat' or neither")
            if isinstance(self, W2VVPP_MultiHeadAttention):
                raise NotImplementedError("training step: key 'LAFF' with the concat towers scores its 2-D embeddings through "
                                          'get_txt2vis_matrix and criterion_with_score (model/model.py:2040-2042), and that score matrix '
                                          "is not differentiable here; train them under 'W2VVPP' or 'w2vpp_mutivis_attention'")
        if getattr(opt, 'negative', False):
            raise NotImplementedError('training step: opt.negative (cal_foward_neg and Margin2Loss, model/model.py:889-962) is not '
                                      'provided; set negative=False')
        if not getattr(opt, 'multi_space', True):
            raise NotImplementedError('training step: multi_space=False scores the heads through get_txt2vis_matrix, which is not '
                                      'differentiable here; set multi_space=True')
        if globals()['float16']:
            raise NotImplementedError('training step: float16 (autocast + GradScaler, model/model.py:970-989) has no counterpart here; '
                                      'the step is fp32')
        if self._concat_towers():
            p = next(self.parameters(), None)
            if p is not None and not p.is_cuda:
                raise NotImplementedError('training step: the concat towers train on the device only (laff_amd has no CPU path); move '
                                          'the model to the GPU, or use predict()')

    def _concat_towers(self):
        return isinstance(self.vis_net, VisTransformNet) or isinstance(self.txt_net, MultiScaleTxtNet)

    def enable_training(self, device_norm=True):
        """Everything the reference's constructor builds for training (model/model.py:1984-2030), kept out of __init__ so that a model
        built for inference allocates none of it: criterion, criterion_with_score, optimizer and lr_schedulers (laff_amd.optim: the clip
        by opt.grad_clip runs inside optimizer.step()), params, grad_clip, iters = 0.  device_norm: every TransformNet's training-mode
        dropout + BatchNorm1d stage runs on this library's kernels (use_device_norm); the no-transform feature trains only that way.
        Returns self."""
        self._training_refusals()
        opt = self.opt
        self.criterion = _loss.criterion_for(opt)
        self.criterion_with_score = _loss.MarginRankingLossWithScore(margin=opt.margin, max_violation=opt.max_violation,
                                                                     cost_style=opt.cost_style, direction=opt.direction)
        # the concat towers train under the reference's base class: Adam(params, lr) with torch's default eps (model/model.py:825), not
        # the multi-head class's eps=1e-4 (:2022)
        self.optimizer, self.lr_schedulers = _optim.optimizer_for(opt, self, **({'adam_eps': 1e-8} if self._concat_towers() else {}))
        self.params = list(self.parameters())
        self.grad_clip = opt.grad_clip
        self.iters = 0
        use_device_norm(self, device_norm)
        for net in (self.vis_net, self.txt_net):           # the towers whose training route opens for an armed model only
            if isinstance(net, (VisMutiTransformNetPlusFrameFeat, VisTransformNet, MultiScaleTxtNet)):
                net.training_armed = True
        return self

    def compute_loss(self, vis_embs, txt_embs, *unused):
        """(loss, {'triplet_loss': loss}) of a batch of embeddings, 2-D or (B, H, d) for the per-head sum (model/model.py:840-865,
        :2032-2048 with multi_space): loss.compute_loss on self.criterion.  The reference's trailing arguments are accepted and unused."""
        return _loss.compute_loss(self.criterion, vis_embs, txt_embs)

    def cal_foward(self, train_data):
        """Both towers and the loss of one batch (model/model.py:867-887): reads train_data['vis_feats'], ['captions'] and
        ['vis_frame_feat_dict'] (an empty dict means None), calls optimizer.zero_grad() where the reference does.  Returns
        (loss, loss_items).  The input dicts are written to, as in the reference: hand over fresh ones every step."""
        frames = train_data.get('vis_frame_feat_dict')
        if frames == {}:
            frames = None
        txt_embs = self.txt_net(train_data['captions'])
        vis_embs = self.vis_net(train_data['vis_feats'], txt_emb=txt_embs, vis_frame_feat_dict_input=frames)
        self.optimizer.zero_grad()
        return self.compute_loss(vis_embs, txt_embs, 0, 0, 0)

    def forward(self, train_data, epoch=None):
        """One training step (model/model.py:964-1001): iters += 1, cal_foward, loss.backward(), optimizer.step(); returns loss_items.
        fp32 only: the reference's float16 / autocast / GradScaler branch has no counterpart here.  The clip by grad_clip runs INSIDE
        optimizer.step() (laff_amd.optim): after a step .grad still holds the UNCLIPPED gradients and optimizer.total_norm their global
        norm, where the reference's clip_grad_norm_ scales .grad in place -- parameters and optimizer state are the reference's."""
        if getattr(self, 'optimizer', None) is None:
            self._training_refusals()
            raise NotImplementedError('training step: this model was built for inference; call enable_training() first (it builds the '
                                      'criterion and the optimizer)')
        self._training_refusals()
        if not self.training:
            raise RuntimeError('training step: the model is in eval mode; call .train() first')
        self.iters += 1
        loss, loss_items = self.cal_foward(train_data)
        loss.backward()
        self.optimizer.step()
        return loss_items

    @property
    def learning_rate(self):
        """The learning rate of every parameter group (model/model.py:1580-1586)."""
        return [group['lr'] for group in self.optimizer.param_groups]

    def lr_step(self, val_value):
        """StepLR once, ReduceLROnPlateau on val_value (model/model.py:1588-1595)."""
        self.lr_schedulers[0].step()
        self.lr_schedulers[1].step(val_value)

    # -- towers ---------------------------------------------------------------------------------------------
    def encode_video(self, vis_input, vis_frame_feat_dict=None):
        """Alias named by BASELINE.json; = self.vis_net(vis_input, vis_frame_feat_dict_input=...)."""
        with torch.no_grad():
            return self.vis_net(vis_input, vis_frame_feat_dict_input=vis_frame_feat_dict if vis_frame_feat_dict is not None else {})

    def encode_text(self, caption_feat_dict):
        with torch.no_grad():
            return self.txt_net(caption_feat_dict)

    # -- similarity -----------------------------------------------------------------------------------------
    @staticmethod
    def compute_sim(query_embs, retro_embs, measure='cosine', device=None):
        if measure not in ('cosine', 'hist'):
            raise NotImplementedError("measure '%s' is never configured on the path (base_config.py:92)" % measure)
        dev = device if device is not None else globals()['device']
        if measure == 'hist':
            return _loss.hist_sim(query_embs.to(dev), retro_embs.to(dev))
        return _loss.cosine_sim(query_embs.to(dev), retro_embs.to(dev), W2VVPP.sim_precision)

    def get_txt2vis_matrix(self, txt_embs, vis_embs, measure='cosine', precision=None):
        """2-D: cosine; 3-D: mean over heads of per-head cosine == one GEMM over the concatenated,
        per-head normalised embeddings divided by H.
        measure='hist': the generalised Jaccard measure, 2-D, or 3-D as the mean over heads of the per-head measure (eps 1e-14 as
        loss.hist_sim); one fp32 kernel on the embeddings as they are -- nothing is packed and `precision` is ignored."""
        if measure not in ('cosine', 'hist'):
            raise NotImplementedError("measure '%s'" % measure)
        if txt_embs.dim() != vis_embs.dim() or txt_embs.dim() not in (2, 3):
            raise ValueError('txt_embs %s / vis_embs %s' % (tuple(txt_embs.shape), tuple(vis_embs.shape)))
        if measure == 'hist':
            return ops.sim_hist(to_device_and_float16(txt_embs).contiguous(), to_device_and_float16(vis_embs).contiguous())
        precision = precision or self.sim_precision or _loss.DEFAULT_PRECISION
        heads = txt_embs.shape[1] if txt_embs.dim() == 3 else 1
        T = ops.pack_rows(to_device_and_float16(txt_embs).contiguous(), True, 1e-13, precision)
        V = ops.pack_rows(to_device_and_float16(vis_embs).contiguous(), True, 1e-13, precision)
        return ops.sim_gemm(T, V, heads=heads)

    # -- predict --------------------------------------------------------------------------------------------
    def _embed_videos(self, vis_loader):
        embs, idxs_list, vis_ids = [], [], []
        for output_dict in vis_loader:
            vis_input, idxs, batch_vis_ids = output_dict['vis_feat_dict'], output_dict['idxs'], output_dict['vis_ids']
            frame_dict = output_dict.get('vis_frame_feat_dict', {})
            idxs_list.append(list(idxs))
            embs.append(self.vis_net(vis_input, vis_frame_feat_dict_input=frame_dict))
            vis_ids.extend(batch_vis_ids)
        return torch.cat(embs, dim=0), idxs_list, vis_ids

    def _embed_texts(self, txt_loader):
        """txt_net over the batches of the text loader: (the embeddings of all captions, their ids)."""
        embs, txt_ids = [], []
        for caption_feat_dict, _, batch_txt_ids in txt_loader:
            embs.append(self.txt_net(caption_feat_dict))
            txt_ids.extend(batch_txt_ids)
        return torch.cat(embs, dim=0), txt_ids

    #: operand precision of retrieve() / predict() when none is given: the score matrix of the drop-in path goes to the host anyway
    #: (1.6 GB over PCIe at C4 is 40x the GEMM), so it takes the split-product GEMM whose scores are fp32-class (~2e-7) like the
    #: reference's own; bench.py / retrieval.evaluate choose their precision themselves
    predict_precision = 'fp16x3'
    #: retrieve() / predict() run each tower ONCE over all loader batches (False: one launch set per batch, like the reference's loop)
    coalesce_loader_batches = True
    #: ... for collections of at most this many videos / captions: the batches of a loader are concatenated in host memory first (the
    #: reference bounds host memory the same way: predict_batch above 5e4 videos, model/model.py:1081-1128)
    coalesce_max_items = 400000

    def _embed_whole(self, vis_loader, txt_loader):
        """Both towers once over the whole matrices: every FC projection of both towers in ONE grouped launch, one fuse launch per
        side -- instead of one launch set per loader batch (780 of them at C4 with the shipped batch size of 64,
        shell/retrieval_task.sh:161).  Loaders that can hand the matrices over do (`whole()`: laff_amd.data.Bulk*Loader); the batches of
        any other loader -- the reference's own DataLoaders -- are collected and concatenated first (`coalesce_batches`).  Row-wise
        arithmetic, so the embeddings are bit-identical to the per-batch route on tiles of the same kind.  Returns None when the
        batches cannot be concatenated (frame tensors padded to different lengths, foreign value types): per-batch route."""
        if hasattr(vis_loader, 'whole') and hasattr(txt_loader, 'whole'):
            out, (cap, _, txt_ids) = vis_loader.whole(), txt_loader.whole()
        else:
            # the loaders are walked ONCE: what was collected is handed back to the per-batch route when it cannot be concatenated
            # (errors raised by the loaders themselves propagate)
            vb, tb = list(vis_loader), list(txt_loader)
            self._collected_batches = (vb, tb)
            try:
                out = coalesce_batches(vb)
                cap, txt_ids = coalesce_batches([b[0] for b in tb]), [i for b in tb for i in b[2]]
            except (TypeError, ValueError, RuntimeError):
                return None
            if out is None or cap is None:
                return None
            self._collected_batches = None
        pending = []
        fin_v = self.vis_net.prepare(out['vis_feat_dict'], out.get('vis_frame_feat_dict', {}), pending)
        fin_t = self.txt_net.prepare(cap, pending)
        run_fc(pending)
        return fin_v(), [list(out['idxs'])], list(out['vis_ids']), fin_t(), list(txt_ids)

    def retrieve(self, txt_loader, vis_loader, measure='cosine', record_emb=False, precision=None):
        """Device-resident version of predict(): returns (S_device (Nt,Nv) fp32, txt_ids, vis_ids).

        When every caption id names its video the reference's way (`txt_id.split('#')[0]` in vis_ids, predictor.py:241), S is
        produced by the exact-rank pipeline: the text->video ranks counted from it (predictor.t2v_ranks, or an argsort on the host
        as the reference does) are the ranks of the exact cosine scores whatever the operand precision; they are also kept in
        `self.last_t2v_ranks`, and the pipeline's state in `self.last_rank_state` (exact video->text positions:
        predictor.retrieval_metrics(S, txt_ids, vis_ids, state=model.last_rank_state)).

        measure='hist': the embeddings are made the same way, S is ops.sim_hist of them; under the id protocol `last_t2v_ranks` are
        the ranks counted on that S itself (1 + the number of other videos scoring higher), and `last_rank_state` stays None."""
        if measure not in ('cosine', 'hist'):
            raise NotImplementedError("measure '%s'" % measure)
        self.eval()
        if not hasattr(self, 'video_all_embs'):
            self.video_all_embs = None
            self.video_idxs_list = []
        precision = precision or self.sim_precision or self.predict_precision
        with torch.no_grad():
            whole = None
            self._collected_batches = None
            vis_loader_given = vis_loader
            if (self.coalesce_loader_batches and (not record_emb or self.video_all_embs is None) and
                    0 < _loader_len(vis_loader) <= self.coalesce_max_items and 0 < _loader_len(txt_loader) <= self.coalesce_max_items):
                whole = self._embed_whole(vis_loader, txt_loader)
            if whole is None and self._collected_batches is not None:
                vis_loader, txt_loader = self._collected_batches       # walk what was collected, not the loaders a second time
                self._collected_batches = None
            if whole is not None:
                self.video_all_embs, self.video_idxs_list, self.vis_ids, txt_all, txt_ids = whole
            else:
                if not record_emb or self.video_all_embs is None:
                    self.video_all_embs, self.video_idxs_list, self.vis_ids = self._embed_videos(vis_loader)
                txt_all, txt_ids = self._embed_texts(txt_loader)
            cols = np.concatenate([np.asarray(i, dtype=np.int64) for i in self.video_idxs_list])
            vis_used = self.video_all_embs
            identity = np.array_equal(cols, np.arange(len(cols)))
            if not identity:   # the reference indexes the cached embeddings BY dataset index (:1066)
                vis_used = self.video_all_embs[torch.as_tensor(cols, device=self.video_all_embs.device)]
            if txt_all.dim() != vis_used.dim():      # a concat (2-D) side against a multi-head (3-D) one: as get_txt2vis_matrix
                raise ValueError('txt_embs %s / vis_embs %s' % (tuple(txt_all.shape), tuple(vis_used.shape)))
            self.last_t2v_ranks = None
            self.last_rank_state = None          # ops.RankState of the exact-rank pass: predictor.retrieval_metrics(S, ..., state=) ranks V2T exactly with it
            owner = None
            if identity and len(txt_ids) and len(self.vis_ids) == vis_used.shape[0]:
                from ..predictor import gt_columns
                try:
                    owner = gt_columns(txt_ids, self.vis_ids)
                except (IndexError, ValueError, AttributeError):
                    owner = None                 # ids do not follow the protocol: plain scores
            if measure == 'hist':
                S = self.get_txt2vis_matrix(txt_all, vis_used, measure)
                if owner is not None:
                    gt = torch.as_tensor(owner, dtype=torch.int32, device=S.device)
                    self.last_t2v_ranks = ops.rank_count(S, gt, ops.gather_gt(S, gt)) + 1
            elif owner is not None:
                gt = torch.as_tensor(owner, dtype=torch.int32, device=txt_all.device)
                Et, Ev = txt_all.contiguous(), vis_used.contiguous()
                # The pair list of the exact-rank pipeline overflows only on degenerate scores (thousands of videos inside one
                # query's error band).  This path goes to the host anyway, so the flag is read (one small synchronising copy) and
                # the pass repeated: first with an 8x larger list, then with hi/lo split operands (band ~1e-6 instead of ~4e-4).
                # Nothing is published from an overflowed pass.
                attempts = [(precision, None), (precision, 8 * ops.default_pair_cap(Et.shape[0]))]
                if precision not in ('fp16x3', 'bf16x3'):
                    attempts.append(('fp16x3', 8 * ops.default_pair_cap(Et.shape[0])))
                for prec, cap in attempts:
                    T = ops.pack_rows(to_device_and_float16(Et), True, 1e-13, prec)
                    V = ops.pack_rows(to_device_and_float16(Ev), True, 1e-13, prec)
                    S, count, st = ops.exact_ranks(Et, Ev, T, V, gt, pair_cap=cap)
                    if not st.overflowed():
                        break
                    del S, count, st
                else:
                    raise RuntimeError('laff_amd: the pair list of the exact-rank pipeline overflowed even with split operands and an 8x '
                                       'list (%d texts x %d videos): the scores are degenerate' % (Et.shape[0], Ev.shape[0]))
                self.last_t2v_ranks = count + 1
                if identity:
                    self.last_rank_state = st
            else:
                S = self.get_txt2vis_matrix(txt_all, vis_used, measure, precision)
            if not identity:
                full = torch.zeros((S.shape[0], len(vis_loader_given.dataset)), device=S.device, dtype=S.dtype)
                full[:, torch.as_tensor(cols, device=S.device)] = S
                S = full
        return S, txt_ids, self.vis_ids

    def predict(self, txt_loader, vis_loader, measure, record_emb=False):
        """Same contract as the reference (model/model.py:1018-1079): (np.float32[Nt,Nv] in loader row order,
        txt_ids, vis_ids).  Embeddings stay in HBM, all pairs are scored by one GEMM, one D2H copy at the end."""
        S, txt_ids, vis_ids = self.retrieve(txt_loader, vis_loader, measure, record_emb)
        return self._scores_to_host(S), txt_ids, vis_ids

    def _scores_to_host(self, S):
        """The score matrix as a numpy array: one asynchronous copy into a PINNED host buffer -- 1.6 GB at C4 take ~30 ms that way
        against ~200 ms through pageable memory.  The array owns that buffer; the buffer is taken again by the next call only once the
        caller has dropped the array (weak reference), so results never alias."""
        if not S.is_cuda or S.numel() < (1 << 20):
            return S.cpu().numpy()
        import weakref
        buf, ref = getattr(self, '_pinned_scores', None), getattr(self, '_pinned_scores_user', None)
        if buf is None or buf.numel() < S.numel() or (ref is not None and ref() is not None):
            self._pinned_scores = self._pinned_scores_user = None
            try:
                buf = torch.empty((S.numel(),), dtype=S.dtype, pin_memory=True)
            except RuntimeError:
                return S.cpu().numpy()
            self._pinned_scores = buf
        host = buf[:S.numel()].view(S.shape)
        host.copy_(S, non_blocking=True)
        torch.cuda.current_stream(S.device).synchronize()
        out = host.numpy()
        self._pinned_scores_user = weakref.ref(out)
        return out

    def predict_batch(self, txt_loader, vis_loader, measure, record_emb=False):
        """The reference switches to a re-embedding loop above 5e4 videos to bound host memory (:1081-1128);
        with 288 GB of HBM the single-pass path covers it, results are identical."""
        return self.predict(txt_loader, vis_loader, measure, False)

    # -- re-ranked predict ----------------------------------------------------------------------------------
    #: queries whose candidate blocks (K x K similarities + re-ranking workspace) are alive at once
    rerank_chunk_bytes = 1 << 30

    def _rerank_predict(self, rerank_rows, txt_loader, vis_loader, measure, t2i_matrix, topK, reranking_weight, return_blocks):
        if measure != 'cosine':
            raise NotImplementedError("measure '%s'" % measure)
        self.eval()
        precision = self.sim_precision or self.predict_precision
        with torch.no_grad():
            Ev, idxs_list, _ = self._embed_videos(vis_loader)
            cols = np.concatenate([np.asarray(i, dtype=np.int64) for i in idxs_list])
            Et, _ = self._embed_texts(txt_loader)
            out = torch.as_tensor(np.asarray(t2i_matrix), dtype=torch.float32).to(Ev.device).contiguous().clone()
            Nt, Nv = out.shape
            if Et.shape[0] != Nt or len(cols) != Nv or not np.array_equal(np.sort(cols), np.arange(Nv)):
                raise ValueError('t2i_matrix is %d x %d; the loaders give %d captions and %d videos' % (Nt, Nv, Et.shape[0], len(cols)))
            if not np.array_equal(cols, np.arange(Nv)):               # embeddings by t2i_matrix column (= dataset index)
                by_col = torch.empty_like(Ev)
                by_col[torch.as_tensor(cols, device=Ev.device)] = Ev
                Ev = by_col
            K = min(int(topK), Nv)
            cand, _ = ops.topk_rows(out, K)
            cand = cand.long()
            per_query = 4 * K * K + 8 * K * min(K + 1, 2048)
            step = max(1, int(self.rerank_chunk_bytes // per_query))
            one = torch.ones((1, 1), device=Ev.device, dtype=torch.float32)
            blocks = ([], [])
            for r0 in range(0, Nt, step):
                problems = []
                for r in range(r0, min(Nt, r0 + step)):
                    Ec = Ev[cand[r]].contiguous()
                    s = self.get_txt2vis_matrix(Et[r:r + 1].contiguous(), Ec, measure, precision)
                    gg = self.get_txt2vis_matrix(Ec, Ec, measure, precision)
                    problems.append((s.contiguous(), one, gg.contiguous()))
                for r, (s, _, gg), rr in zip(range(r0, r0 + len(problems)), problems, rerank_rows(problems)):
                    out[r, cand[r]] = (s + reranking_weight * rr)[0]
                    if return_blocks:
                        blocks[0].append(s[0].cpu().numpy())
                        blocks[1].append(gg.cpu().numpy())
            res = _loss.l2norm(out).cpu().numpy()
        if return_blocks:
            return res, cand.cpu().numpy(), np.stack(blocks[0]), np.stack(blocks[1])
        return res

    def predict_rerank(self, txt_loader, vis_loader, measure, t2i_matrix, topK=3000, k1=20, reranking_weight=2, return_blocks=False):
        """The reference's predict_rerank (model/model.py:1131-1201) on the device.  For every query row r of t2i_matrix: cand = its
        K = min(topK, Nv) best columns (descending), s = the similarity of text r to the candidates, gg = the candidates against
        themselves (both by get_txt2vis_matrix's route at predict()'s precision), and
        out[r, cand] = s + reranking_weight * ReRank.re_ranking(s, [[1]], gg, k1=k1); the other columns keep t2i_matrix's values; rows
        are then L2-normalised.  Returns np.float32 [Nt, Nv]; with return_blocks=True (our addition, for small shapes) also
        cand [Nt, K], s [Nt, K] and gg [Nt, K, K] as consumed.

        Two deliberate deviations from the reference: it addresses the query as `i * j + j` (batch i, row j), which is the intended
        row only within the first text batch -- the global row index is used here; and its per-query subset loader does not run
        against its own current loader format -- the video embeddings are computed once, as predict() does, and the candidates'
        rows gathered on the device."""
        from . import ReRank
        return self._rerank_predict(lambda ps: ReRank.re_ranking_batched(ps, k1=k1), txt_loader, vis_loader, measure, t2i_matrix, topK,
                                    reranking_weight, return_blocks)

    def predict_rerank_tkb_simple(self, txt_loader, vis_loader, measure, t2i_matrix, topK=3000, k1=20, reranking_weight=2,
                                  return_blocks=False):
        """The reference's predict_rerank_tkb_simple (model/model.py:1203-1275): as predict_rerank, with
        ReRank.re_ranking_tkb_simple(s, [[1]], gg, topK=topK, k1=k1) as the re-ranking term (same two deviations)."""
        from . import ReRank
        return self._rerank_predict(lambda ps: [ReRank.re_ranking_tkb_simple(s, qq, gg, topK=topK, k1=k1) for s, qq, gg in ps],
                                    txt_loader, vis_loader, measure, t2i_matrix, topK, reranking_weight, return_blocks)


class W2VVPP_MutiVis(W2VVPP):
    def _init_txt_net(self, opt):
        if opt.txt_attention == 'concat':
            return super()._init_txt_net(opt)
        self.txt_net = MultiScaleTxtEncoderAttention(opt)

    def _init_vis_net(self, opt):
        if opt.vis_attention == 'concat':
            return super()._init_vis_net(opt)
        self.vis_net = VisMutiTransformNetAddAttnetion(opt, opt.vis_fc_layers[0])

    def change_raw_global_emb_weight(self):
        """Linear decay of gw, once per epoch in the reference (model/model.py:1910-1941).  Like the reference it only looks
        for an attribute called `attention_layer`: the FrameLAFF video tower (`vis_attention_layer`) is never decayed."""
        for net, rate in ((self.txt_net, self.opt.txt_attention_global_decay_rate),
                          (self.vis_net, self.opt.vis_attention_global_decay_rate)):
            layer = getattr(net, 'attention_layer', None)
            if layer is not None and hasattr(layer, 'get_raw_global_emb_weight'):
                layer.change_raw_global_emb_weight(max(0.0, rate - 1 + layer.get_raw_global_emb_weight()))


class W2VVPP_MultiHeadAttention(W2VVPP_MutiVis):
    def get_txt2vis_matrix_each_head(self, txt_embs, vis_embs, measure='cosine'):
        return torch.stack([self.get_txt2vis_matrix(txt_embs[:, h, :].contiguous(), vis_embs[:, h, :].contiguous(), measure)
                            for h in range(txt_embs.shape[1])], dim=0)

    def predict_each_head(self, txt_loader, vis_loader, measure):
        """(H, Nt, Nv) per-head score cubes (model/model.py:2058-2098)."""
        self.eval()
        with torch.no_grad():
            vis_all, idxs_list, vis_ids = self._embed_videos(vis_loader)
            txt_all, txt_ids = self._embed_texts(txt_loader)
            scores = self.get_txt2vis_matrix_each_head(txt_all, vis_all, measure)
        return scores.cpu().numpy(), txt_ids, vis_ids


class W2VVPP_MutiVisFrameFeat(W2VVPP_MutiVis):
    def _init_vis_net(self, opt):
        self.vis_net = VisMutiTransformNetPlusFrameFeat(opt)


def get_model(name, device_, config):
    """Registry of the reference (model/model.py:2501-2519); keys outside the hot path are refused."""
    global device
    global float16
    device = torch.device(device_)
    float16 = config.float16
    NAME_TO_MODELS = {
        'W2VVPP': W2VVPP,
        'FrameLAFF': W2VVPP_MutiVisFrameFeat,
        'w2vpp_mutivis_attention': W2VVPP_MutiVis,
        'LAFF': W2VVPP_MultiHeadAttention,
    }
    if name == 'End2EndClip':
        raise NotImplementedError("model '%s' is outside the LAFF hot path (SURVEY.md section 2)" % name)
    assert name in NAME_TO_MODELS, '%s not supported.' % name
    model_ = NAME_TO_MODELS[name](config)
    model_ = model_.float().to(device)
    return model_
