"""Fusion blocks of the reference's model/Attention.py that lie on the hot path, same class names, constructor
arguments, parameter names (state_dict keys) and output shapes; forward() runs the `laff_fuse` HIP kernel.  In training mode
(`module.train()`) the blocks are differentiable: the same forward kernel under torch.autograd, `laff_fuse_backward` behind it
(_FuseFn below).

  Attention_1                    /root/reference/model/Attention.py:40-105
  Multi_head_MyApply_Attention   /root/reference/model/Attention.py:473-552
  JustAverage                    /root/reference/model/Attention.py:26-37
  Multi_head_MyApply_selfAttention   /root/reference/model/Attention.py:317-470   (`laff_selfattn_fuse` and its backward,
                                 _SelfAttnFn below): the multi-head self-attention baseline of the paper

The other 12 variants of that file are ablation baselines never selected by the shipped scripts
 and are not provided.
"""
import torch
import torch.nn as nn

from .. import ops


def _planes_of(local_embs):
    """(N, L, D) stacked tensor -> list of per-feature strided row views (no copy)."""
    if local_embs.dim() != 3:
        raise ValueError('local_embs must be (batch, L, embed_dim)')
    if local_embs.stride(2) != 1:
        local_embs = local_embs.contiguous()
    return [(local_embs[:, l, :], False, None, None) for l in range(local_embs.shape[1])]


class _FuseFn(torch.autograd.Function):
    """ops.fuse over plain dense fp32 planes with ops.fuse_backward as its backward: (E (N, H, d), softmax weights (N, H, L) or None).
    The planes come either as `stacked`, one (N, L, D) tensor whose slices are read in place and whose gradient is written in place,
    or one by one in `planes` (then stacked is None).  w and b receive gradients, gw does not (the reference reads it through
    .item(), model/Attention.py:96).  Once differentiable."""

    @staticmethod
    def forward(ctx, H, d, flags, w, b, gw, stacked, *planes):
        srcs = [stacked[:, l, :] for l in range(stacked.shape[1])] if stacked is not None else list(planes)
        for t in srcs + [t for t in (w, b, gw) if t is not None]:
            if t.dtype != torch.float32:
                raise TypeError('the differentiable fusion is fp32 only, got %s' % t.dtype)
        just_average = bool(flags & ops.ATT_JUST_AVERAGE)
        res = ops.fuse([(t.detach(), False, None, None) for t in srcs], H, d, w, b, gw, flags, return_weights=not just_average)
        E, aw = (res, None) if just_average else res
        ctx.save_for_backward(*[t for t in (w, b, gw, stacked) if t is not None], *planes)
        ctx.meta = (H, d, flags, w is not None, b is not None, gw is not None, stacked is not None, len(planes))
        if aw is not None:
            ctx.mark_non_differentiable(aw)
        return E, aw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_E, _grad_weights=None):
        H, d, flags, has_w, has_b, has_gw, has_stacked, nplanes = ctx.meta
        saved = list(ctx.saved_tensors)
        w = saved.pop(0) if has_w else None
        b = saved.pop(0) if has_b else None
        gw = saved.pop(0) if has_gw else None
        stacked = saved.pop(0) if has_stacked else None
        want = has_w and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        out = d_stacked = None
        if has_stacked:
            d_stacked = torch.empty_like(stacked, memory_format=torch.contiguous_format)
            srcs = [stacked[:, l, :] for l in range(stacked.shape[1])]
            out = [d_stacked[:, l, :] for l in range(stacked.shape[1])]
        else:
            srcs = saved
        dxs, dw, db = ops.fuse_backward(srcs, H, d, w, b, gw, flags, grad_E, want_param_grads=want, out=out)
        return (None, None, None, dw.view_as(w) if want else None, db.view_as(b) if want else None, None, d_stacked) + \
            (tuple(dxs) if not has_stacked else ())


class _FrameFuseFn(torch.autograd.Function):
    """ops.frame_fuse over (B, Fmax, d) fp32 frames with ops.frame_fuse_backward as its backward: V (B, d), the very bits of
    ops.frame_fuse.  Saves the frames, lens and the parameters; the forward is recomputed in the backward launch.  w and b receive
    gradients (b's is zero), gw does not.  Rows of the frames' gradient at or past a video's length are zeros.  Once differentiable."""

    @staticmethod
    def forward(ctx, flags, lens, w, b, gw, frames):
        for t in (frames, w, b) + ((gw,) if gw is not None else ()):
            if t.dtype != torch.float32:
                raise TypeError('the differentiable frame attention is fp32 only, got %s' % t.dtype)
        frames, wd, bd = frames.detach().contiguous(), w.detach().contiguous(), b.detach().contiguous()
        V = ops.frame_fuse(frames, lens, wd, bd, gw, flags)
        ctx.save_for_backward(frames, wd, bd, *[t for t in (gw, lens) if t is not None])
        ctx.meta = (flags, gw is not None, lens is not None)
        return V

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_V):
        flags, has_gw, has_lens = ctx.meta
        saved = list(ctx.saved_tensors)
        frames, w, b = saved[:3]
        gw = saved[3] if has_gw else None
        lens = saved[-1] if has_lens else None
        want = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        dfs, dws, dbs = ops.frame_fuse_backward([frames], lens, [(w, b, gw)], flags, [grad_V], want_param_grads=want)
        return None, None, dws[0] if want else None, dbs[0] if want else None, None, dfs[0]


def _train_stacked(local_embs):
    """(N, L, D) whose slices the kernels can read in place, as the training-mode forward hands it to _FuseFn: unit inner stride, pitches
    that are multiples of 4 floats and a 16-byte aligned base -- the rule ops.fuse_backward applies to grad_E; anything else is copied."""
    if local_embs.dim() != 3:
        raise ValueError('local_embs must be (batch, L, embed_dim)')
    ok = local_embs.stride(2) == 1 and local_embs.stride(0) % 4 == 0 and local_embs.stride(1) % 4 == 0 and local_embs.data_ptr() % 16 == 0
    return local_embs if ok or not local_embs.numel() else local_embs.contiguous()


def _train_sources(planes, l2norm_planes):
    """The tensors of `planes` when every one of them is plain and dense -- what the training-mode forward accepts."""
    if l2norm_planes:
        raise NotImplementedError('training mode: the backward of the fusion has no row_scale (l2norm_planes); normalise the planes '
                                  'upstream with torch ops')
    return [ops.dense_plane(p, i) for i, p in enumerate(planes)]


def _full_width(plane, heads, D):
    """a tiled plane (src (N, D / heads), tile, scale, shift) written out as (N, D): repeat over heads + the folded affine"""
    out = ops.fuse([plane], heads, D // heads, None, None, None, ops.attention_flags(just_average=True))
    return out.view(out.shape[0], D)


class JustAverage(nn.Module):
    def forward(self, local_embs, raw_global_emb=None):
        if self.training:
            x = _train_stacked(local_embs)
            return _FuseFn.apply(1, x.shape[2], ops.attention_flags(just_average=True), None, None, None, x)[0].view(x.shape[0], x.shape[2])
        return self.fuse_planes(_planes_of(local_embs))

    def fuse_planes(self, planes, heads=1, l2norm_planes=False):
        if self.training:
            srcs = _train_sources(planes, l2norm_planes)
            D = srcs[0].shape[1]
            return _FuseFn.apply(1, D, ops.attention_flags(just_average=True), None, None, None, None, *srcs)[0].view(-1, D)
        H = heads if any(p[1] for p in planes) else 1
        D = planes[0][0].shape[1] * (heads if planes[0][1] else 1)
        out = ops.fuse(planes, H, D // H, None, None, None, ops.attention_flags(just_average=True), l2norm_planes=l2norm_planes)
        return out.view(out.shape[0], D)


class Attention_1(nn.Module):
    """softmax_L(Linear(d,1)(c)) weighted sum over the L fused features (+ gw * mean), then l2norm(eps=0)."""

    def __init__(self, embed_dim, with_ave=True, mul=False):
        super().__init__()
        self.with_ave = with_ave
        self.mul = mul
        self.embed_dim = embed_dim
        self.embedding_common = nn.Sequential(nn.Linear(embed_dim, 1))
        self.weights = 0
        self.global_emb_weight_net = nn.Linear(1, 1, False)
        self.change_raw_global_emb_weight(1)

    def get_raw_global_emb_weight(self):
        return self.global_emb_weight_net.weight.item()

    def change_raw_global_emb_weight(self, new_value):
        self.global_emb_weight_net.weight.data.fill_(new_value)

    def get_attention_weight(self):
        return torch.as_tensor(self.weights).clone().detach().cpu()

    def _params(self):
        lin = self.embedding_common[0]
        return (lin.weight.detach().reshape(1, -1).contiguous(), lin.bias.detach().reshape(1).contiguous(),
                self.global_emb_weight_net.weight.detach().reshape(1).contiguous())

    def fuse_planes(self, planes, heads=1, l2norm_planes=False, record_weights=None):
        """record_weights: also store the softmax weights (the reference's `self.weights` side output, Attention.py:90,97).  The
        tower path leaves it off unless `self.record_weights` is set (get_attention_weight does): it is an extra N x L store per
        launch that only that consumer reads."""
        if self.training:
            return self._fuse_train(None, _train_sources(planes, l2norm_planes), record_weights)
        w, b, gw = self._params()
        flags = ops.attention_flags(self.with_ave, self.mul)
        if heads > 1 and any(p[1] for p in planes):
            # a no-transform feature repeated over `heads` (model/model.py:1822-1823) in front of a single-head attention: this block
            # sees all heads * d columns as one vector, so the tiled plane is materialised to full width first
            planes = [(_full_width(p, heads, self.embed_dim), False, None, None) if p[1] else p for p in planes]
        packed = getattr(self, 'emit_packed', None)       # 'fp16' | 'bf16': also emit the GEMM operand (last_packed)
        rec = getattr(self, 'record_weights', False) if record_weights is None else record_weights
        # rank_side (ops.FusedPrepare.video / .text, set for one pass by its owner): laff_rank_prepare's work for these rows rides along
        side = getattr(self, 'rank_side', None) if packed else None
        res = ops.fuse(planes, 1, self.embed_dim, w, b, gw, flags, return_weights=rec, packed_precision=packed,
                       l2norm_planes=l2norm_planes, rank_side=side)
        res = res if isinstance(res, tuple) else (res,)
        E = res[0]
        self.last_packed = res[-1] if packed else None
        if rec:
            aw = res[1][:, 0, :]
            if self.with_ave:   # what the reference stashes in that case (Attention.py:97)
                aw = aw + gw / aw.shape[1]
            self.weights = aw
        return E.view(E.shape[0], self.embed_dim)

    def _fuse_train(self, stacked, srcs, record_weights):
        """Training mode: the block under autograd (_FuseFn) over a stacked (N, L, D) tensor or over plain dense planes.  The
        parameters go in as they are (w and b receive gradients), gw detached; emit_packed / rank_side are not read."""
        lin = self.embedding_common[0]
        gw = self.global_emb_weight_net.weight.detach().reshape(1)
        E, aw = _FuseFn.apply(1, self.embed_dim, ops.attention_flags(self.with_ave, self.mul), lin.weight.reshape(1, -1),
                              lin.bias.reshape(1), gw, stacked, *srcs)
        self.last_packed = None
        if getattr(self, 'record_weights', False) if record_weights is None else record_weights:
            aw = aw.detach()[:, 0, :]
            self.weights = aw + gw / aw.shape[1] if self.with_ave else aw
        return E.view(E.shape[0], self.embed_dim)

    def fuse_frames(self, frames, lens=None):
        """This block over the frames of each video, (B, Fmax, d) zero padded -> (B, d), in one launch (ops.frame_fuse): what the
        reference's loop over the batch computes (model/model.py:2167-2173).  lens: int32 (B,), frames at or past it count as zeros.
        In training mode the call is differentiable (_FrameFuseFn): the frames and embedding_common receive gradients, gw is detached;
        the values are the eval-mode bits."""
        ops._dev(frames, 'frames')
        if frames.dim() != 3 or frames.shape[2] != self.embed_dim:
            raise ValueError('frames must be (B, Fmax, %d), got shape %s' % (self.embed_dim, tuple(frames.shape)))
        flags = ops.attention_flags(self.with_ave, self.mul)
        if not self.training:
            w, b, gw = self._params()
            return ops.frame_fuse(frames.contiguous(), lens, w.reshape(-1), b, gw, flags)
        lin = self.embedding_common[0]
        return _FrameFuseFn.apply(flags, lens, lin.weight.reshape(-1), lin.bias.reshape(1),
                                  self.global_emb_weight_net.weight.detach().reshape(1), frames)

    def forward(self, local_embs, raw_global_emb=None):
        if raw_global_emb is not None:
            raise NotImplementedError('raw_global_emb is never passed on the retrieval path '
                                      '(and is undefined in the reference when mul=False)')
        if self.training:
            return self._fuse_train(_train_stacked(local_embs), [], True)
        return self.fuse_planes(_planes_of(local_embs), record_weights=True)


class Multi_head_MyApply_Attention(nn.Module):
    """H independent Attention_1 blocks over head slices of the common space -> (batch, H, dim_per_head)."""

    def __init__(self, embed_dim, multi_heads=None, dim_per_head=None, with_ave=True, mul=True, split_head=True,
                 l2norm_each_head=False):
        super().__init__()
        if embed_dim is None:
            return
        self.dim_per_head = dim_per_head
        self.multi_heads = multi_heads
        self.split_head = split_head
        if self.split_head:
            assert dim_per_head == embed_dim // multi_heads
        else:
            dim_per_head = embed_dim
        self.head_dim = dim_per_head
        self.with_ave, self.mul = with_ave, mul
        self.attention_layer = nn.Sequential()
        for i in range(multi_heads):
            self.attention_layer.add_module(str(i), Attention_1(dim_per_head, with_ave=with_ave, mul=mul))
        self.layer_norm = nn.LayerNorm(dim_per_head)   # declared and unused, as in the reference (:504)
        self.l2norm_each_head = l2norm_each_head
        self._packed = None

    def _params(self):
        ps = [p for h in range(self.multi_heads) for p in self.attention_layer[h].parameters()]
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if self._packed is None or self._packed[0] != key:
            w = torch.stack([self.attention_layer[h].embedding_common[0].weight.detach().reshape(-1)
                             for h in range(self.multi_heads)]).contiguous()
            b = torch.cat([self.attention_layer[h].embedding_common[0].bias.detach().reshape(1)
                           for h in range(self.multi_heads)]).contiguous()
            gw = torch.cat([self.attention_layer[h].global_emb_weight_net.weight.detach().reshape(1)
                            for h in range(self.multi_heads)]).contiguous()
            self._packed = (key, w, b, gw)
        return self._packed[1:]

    def fuse_planes(self, planes, heads=None, l2norm_planes=False, record_weights=None):
        if self.training:
            return self._fuse_train(None, _train_sources(planes, l2norm_planes), record_weights)
        w, b, gw = self._params()
        flags = ops.attention_flags(self.with_ave, self.mul, self.l2norm_each_head, self.split_head)
        packed = getattr(self, 'emit_packed', None)       # 'fp16' | 'bf16': also emit the GEMM operand (last_packed)
        rec = getattr(self, 'record_weights', False) if record_weights is None else record_weights
        side = getattr(self, 'rank_side', None) if packed else None
        res = ops.fuse(planes, self.multi_heads, self.head_dim, w, b, gw, flags, return_weights=rec, packed_precision=packed,
                       l2norm_planes=l2norm_planes, rank_side=side)
        res = res if isinstance(res, tuple) else (res,)
        E = res[0]
        self.last_packed = res[-1] if packed else None
        if rec:
            aw = res[1]
            for h in range(self.multi_heads):
                a = aw[:, h, :]
                self.attention_layer[h].weights = a + gw[h] / a.shape[1] if self.with_ave else a
        return E

    def _fuse_train(self, stacked, srcs, record_weights):
        """Training mode: the block under autograd (_FuseFn).  w and b are stacked from the heads' parameters WITHOUT detach, so
        autograd hands every head's embedding_common[0].weight / .bias its slice; gw is detached (no gradient, as in the reference);
        emit_packed / rank_side are not read."""
        heads = [self.attention_layer[h] for h in range(self.multi_heads)]
        w = torch.stack([a.embedding_common[0].weight.reshape(-1) for a in heads])
        b = torch.cat([a.embedding_common[0].bias.reshape(1) for a in heads])
        gw = torch.cat([a.global_emb_weight_net.weight.detach().reshape(1) for a in heads])
        flags = ops.attention_flags(self.with_ave, self.mul, self.l2norm_each_head, self.split_head)
        E, aw = _FuseFn.apply(self.multi_heads, self.head_dim, flags, w, b, gw, stacked, *srcs)
        self.last_packed = None
        if getattr(self, 'record_weights', False) if record_weights is None else record_weights:
            aw = aw.detach()
            for h, a in enumerate(heads):
                a.weights = aw[:, h, :] + gw[h] / aw.shape[2] if self.with_ave else aw[:, h, :]
        return E

    def forward(self, local_embs, raw_global_emb=None, attn_mask=None):
        if self.training:
            return self._fuse_train(_train_stacked(local_embs), [], True)
        return self.fuse_planes(_planes_of(local_embs), record_weights=True)

    def get_raw_global_emb_weight(self):
        return self.attention_layer[0].global_emb_weight_net.weight.item()

    def change_raw_global_emb_weight(self, new_value):
        for i in range(self.multi_heads):
            self.attention_layer[i].global_emb_weight_net.weight.data.fill_(new_value)

    def get_attention_weight(self, head=0):
        return self.attention_layer[head].get_attention_weight().detach()


class _SelfAttnFn(torch.autograd.Function):
    """ops.selfattn_fuse over plain dense fp32 planes with ops.selfattn_fuse_backward as its backward: E (N, H, d), or the stacked tokens
    (N, L, H * d) for the 'Attention_1' output type.  The planes come as `stacked`, one (N, L, D) tensor whose slices are read in place
    and whose gradient is written in place, or one by one in `planes` (then stacked is None).  gamma and beta (the shared LayerNorm)
    receive gradients.  Saves the inputs only: the backward launch recomputes the forward.  Once differentiable."""

    @staticmethod
    def forward(ctx, H, d, output_type, l2norm_each_head, gamma, beta, stacked, *planes):
        srcs = [stacked[:, l, :] for l in range(stacked.shape[1])] if stacked is not None else list(planes)
        for t in srcs + [gamma, beta]:
            if t.dtype != torch.float32:
                raise TypeError('the differentiable self-attention fusion is fp32 only, got %s' % t.dtype)
        out = ops.selfattn_fuse([t.detach() for t in srcs], H, d, gamma.detach().contiguous(), beta.detach().contiguous(), output_type,
                                l2norm_each_head)
        ctx.save_for_backward(gamma, beta, *([stacked] if stacked is not None else []), *planes)
        ctx.meta = (H, d, output_type, l2norm_each_head, stacked is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        H, d, output_type, l2n, has_stacked = ctx.meta
        gamma, beta, *saved = ctx.saved_tensors
        want = ctx.needs_input_grad[4] or ctx.needs_input_grad[5]
        out = d_stacked = None
        if has_stacked:
            stacked = saved[0]
            d_stacked = torch.empty_like(stacked, memory_format=torch.contiguous_format)
            srcs = [stacked[:, l, :] for l in range(stacked.shape[1])]
            out = [d_stacked[:, l, :] for l in range(stacked.shape[1])]
        else:
            srcs = saved
        dxs, dgamma, dbeta = ops.selfattn_fuse_backward(srcs, H, d, gamma.detach().contiguous(), beta.detach().contiguous(), output_type,
                                                        l2n, grad, want_param_grads=want, out=out)
        return (None, None, None, None, dgamma, dbeta, d_stacked) + (tuple(dxs) if not has_stacked else ())


class Multi_head_MyApply_selfAttention(nn.Module):
    """Multi-head self-attention over the L fused features, q = k = v = the head slices, residual + one LayerNorm(dim_per_head) shared
    by all heads, then the pooling `output_type` names -> (batch, H, dim_per_head), not L2-normalised (except under 'Attention_1',
    where head h of the L outputs goes through Attention_list[h]).  Constructor arguments, parameter names and output shapes are the
    reference's.  Refused by name: the output types 'cls_embedding' and 'concat', 'random' in training mode, attention dropout > 0 in
    training mode, dim_per_head < multi_heads (the reference's scale (d // H) ** -0.5 divides by zero)."""

    fused_pack = False        # the rows are not unit-norm and no 16-bit operand rides on this launch: dist.HipBackend packs them itself

    def __init__(self, embed_dim, multi_heads=None, dim_per_head=None, dropout_rate=None, output_type='mean', encoder_num=0,
                 l2norm_each_head=False, opt=None):
        super().__init__()
        if dropout_rate is None:
            dropout_rate = 0.0
        assert dim_per_head == embed_dim // multi_heads
        if output_type in ('cls_embedding', 'concat'):
            raise NotImplementedError("my_self_attention output type '%s' has upstream parameters of its own and is not provided" %
                                      output_type)
        if output_type not in ops.SELFATTN_OUTPUT_TYPES:
            raise NotImplementedError('my_self_attention output type %r is not provided (provided: %s)' %
                                      (output_type, ', '.join(ops.SELFATTN_OUTPUT_TYPES)))
        if dim_per_head < multi_heads:
            raise ValueError('my_self_attention: dim_per_head=%d < multi_heads=%d: the scale (dim_per_head // multi_heads) ** -0.5 '
                             'divides by zero' % (dim_per_head, multi_heads))
        self.dim_per_head = dim_per_head
        self.multi_heads = multi_heads
        self.dropout_rate = float(dropout_rate)
        self.layer_norm = nn.LayerNorm(dim_per_head)
        self.l2norm_each_head = l2norm_each_head
        self.output_type = output_type
        if output_type == 'Attention_1':
            self.Attention_list = nn.ModuleList()
            for _ in range(multi_heads):
                if opt is None:
                    self.Attention_list.append(Attention_1(dim_per_head))
                else:
                    self.Attention_list.append(Attention_1(dim_per_head, with_ave=opt.attention_param_each_head['with_ave'],
                                                           mul=opt.attention_param_each_head['mul']))

    def _training_refusals(self):
        if self.output_type == 'random':
            raise NotImplementedError("my_self_attention output type 'random' draws from Python's random in training mode and is not "
                                      "provided there (in eval it is the mean)")
        if self.dropout_rate > 0:
            raise NotImplementedError('my_self_attention: attention dropout %g in training mode is not provided (the shipped configs '
                                      'set 0.0)' % self.dropout_rate)
        if not self.layer_norm.weight.is_cuda:
            raise NotImplementedError('training mode: my_self_attention trains on the device only (laff_amd has no CPU path); move the '
                                      'model to the GPU, or call .eval()')

    def _tail(self, tokens, record_weights):
        """'Attention_1': head h of the stacked tokens (N, L, H * d) through Attention_list[h], the existing fusion launch on the
        tokens in place -> (N, H, d).  In training mode under _FuseFn (every head's embedding_common receives its slice of dw, db)."""
        heads = list(self.Attention_list)
        a0 = heads[0]
        flags = ops.attention_flags(a0.with_ave, a0.mul)
        train = self.training
        keep = (lambda p: p) if train else (lambda p: p.detach())
        w = torch.stack([keep(a.embedding_common[0].weight).reshape(-1) for a in heads])
        b = torch.cat([keep(a.embedding_common[0].bias).reshape(1) for a in heads])
        gw = torch.cat([a.global_emb_weight_net.weight.detach().reshape(1) for a in heads])
        if train:
            E, aw = _FuseFn.apply(self.multi_heads, self.dim_per_head, flags, w, b, gw, tokens)
            aw = aw.detach()
        else:
            E, aw = ops.fuse(_planes_of(tokens), self.multi_heads, self.dim_per_head, w, b, gw, flags, return_weights=True)
        if record_weights:
            for h, a in enumerate(heads):
                a.weights = aw[:, h, :] + gw[h] / aw.shape[2] if a.with_ave else aw[:, h, :]
        return E

    def _run(self, stacked, srcs, record_weights):
        rec = getattr(self, 'record_weights', False) if record_weights is None else record_weights
        H, d = self.multi_heads, self.dim_per_head
        if self.training:
            self._training_refusals()
            out = _SelfAttnFn.apply(H, d, self.output_type, bool(self.l2norm_each_head), self.layer_norm.weight, self.layer_norm.bias,
                                    stacked, *srcs)
        else:
            planes = srcs if stacked is None else [stacked[:, l, :] for l in range(stacked.shape[1])]
            out = ops.selfattn_fuse(planes, H, d, self.layer_norm.weight.detach(), self.layer_norm.bias.detach(), self.output_type,
                                    bool(self.l2norm_each_head))
        return self._tail(out, rec) if self.output_type == 'Attention_1' else out

    def fuse_planes(self, planes, heads=None, l2norm_planes=False, record_weights=None):
        """The block over a tower's plane descriptors.  Training: plain dense planes under autograd (l2norm_planes and expert rows go
        through the expert stage upstream).  Eval: a plane that is tiled, carries a folded affine, a deferred activation, a gather or
        the row norm of l2norm_planes is written out first (one just-average launch of the existing fusion kernel per such plane)."""
        if self.training:
            return self._run(None, _train_sources(planes, l2norm_planes), record_weights)
        D = self.multi_heads * self.dim_per_head
        srcs = []
        for p in planes:
            p = p if isinstance(p, tuple) else (p, False, None, None)
            plain = not p[1] and p[2] is None and p[3] is None and all(x is None for x in p[4:])
            if plain and not l2norm_planes:
                srcs.append(p[0])
            else:
                out = ops.fuse([p], self.multi_heads, self.dim_per_head, None, None, None, ops.attention_flags(just_average=True),
                               l2norm_planes=l2norm_planes)
                srcs.append(out.view(out.shape[0], D))
        return self._run(None, srcs, record_weights)

    def forward(self, local_embs, raw_global_emb=None, attn_mask=None):
        if attn_mask is not None:
            raise NotImplementedError('attn_mask is never passed on the retrieval path')
        return self._run(_train_stacked(local_embs), [], True)

    def get_raw_global_emb_weight(self):
        if hasattr(self, 'Attention_list'):
            return self.Attention_list[0].get_raw_global_emb_weight()
        return 0

    def change_raw_global_emb_weight(self, new_value):
        if hasattr(self, 'Attention_list'):
            for a in self.Attention_list:
                a.change_raw_global_emb_weight(new_value)
        return 0

    def get_attention_weight(self):
        if not hasattr(self, 'Attention_list'):
            raise Exception('SelfAttention weights is not applied')
        weights = None
        for a in self.Attention_list:
            w = a.get_attention_weight()
            weights = w if weights is None else weights + w
        return weights / self.multi_heads
