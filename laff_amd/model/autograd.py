"""The autograd layer of the FC projection: the torch.autograd.Functions that TransformNet's training mode and the frame Linear run
under (DESIGN.md sections 4.20, 4.24, 4.25, 4.26, 4.27).  Each is one forward launch of the library with its backward launches behind it, forms only
the gradients that needs_input_grad asks for, and is once differentiable.

The ops are reached as attributes of the `ops` module at call time: tests wrap them there and count the calls."""
import torch

from .. import ops


def _fp32(t, name):
    if t is not None and t.dtype != torch.float32:
        raise TypeError('the differentiable projection is fp32 only, %s is %s' % (name, t.dtype))


def _fp32_params(weight, bias):
    _fp32(weight, 'fc1.weight')
    _fp32(bias, 'fc1.bias')


def _dense_input(x):
    """A dense input as the forward launch and the backward read it: detached, and dense when its inner stride is not 1 (a row pitch is
    read in place)."""
    x = x.detach()
    if x.dim() == 2 and x.numel() and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _detached(t):
    return None if t is None else t.detach()


def _csc_of(x):
    """The transposed pattern of a device CSR input: the one its encoder attached (txt2vec.BoWTxtEncoder(with_csc=True)), else
    transposed on the device now (a stable sort, no host synchronisation)."""
    csc = getattr(x, 'laff_csc', None)
    return tuple(csc) if csc is not None else ops.csr_transpose(x)


class _FcActFn(torch.autograd.Function):
    """a = act(x @ weight.T + bias) on laff_fc_act_bn (the fp32 route, whatever FC_PRECISION says) with ops.fc_backward as its backward.
    Saves x, weight and the output a: act' is a function of a for every activation of the reference.  No dx launch for pre-extracted
    features."""

    @staticmethod
    def forward(ctx, x, weight, bias, activation):
        _fp32(x, 'the input')
        _fp32_params(weight, bias)
        x = _dense_input(x)
        a = ops.fc_act_bn(x, weight.detach(), _detached(bias), None, None, activation)
        ctx.save_for_backward(x, weight, a)
        ctx.activation, ctx.has_bias = activation, bias is not None
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_a):
        x, weight, a = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db = ops.fc_backward(x, weight.detach(), a, grad_a, ctx.activation, want_dx=need[0], want_dw=need[1],
                                     want_db=ctx.has_bias and need[2])
        return dx, dw, db, None


class _FcGatherFn(torch.autograd.Function):
    """a = act(x @ weight.T + bias) for a device torch.sparse_csr x: laff_fc_gather_act_bn on the layer's cached weight_t() forward,
    ops.fc_gather_backward behind it.  Saves the transposed pattern (CSC) and the output a; dw comes back in weight's own shape,
    contiguous, so that laff_amd.optim steps it as it is; x gets no gradient (counts).  The forward keeps the kernel's fused activation:
    its output met the training tests' rule with room."""

    @staticmethod
    def forward(ctx, x, weight, bias, weight_t, activation):
        _fp32_params(weight, bias)
        a = ops.fc_gather_act_bn(x, weight_t, _detached(bias), None, None, activation)
        ctx.save_for_backward(a, *_csc_of(x))
        ctx.activation, ctx.has_bias, ctx.x_shape = activation, bias is not None, tuple(x.shape)
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_a):
        a, *csc = ctx.saved_tensors
        need = ctx.needs_input_grad
        dw, db = ops.fc_gather_backward(tuple(csc), ctx.x_shape[0], ctx.x_shape[1], a, grad_a, ctx.activation,
                                        want_dw=need[1], want_db=ctx.has_bias and need[2])
        return None, dw, db, None, None


def _saved_segments(csr_shapes, saved):
    """(shape, segment) per segment of a concat layer from what its forward saved: a CSR segment's (N, width) with its
    (colptr, rows, values) -- 3 saved tensors --, None with the dense matrix -- 1 saved tensor -- for a dense one."""
    at = 0
    for shape in csr_shapes:
        n = 1 if shape is None else 3
        yield shape, saved[at] if shape is None else tuple(saved[at:at + 3])
        at += n


class _FcConcatFn(torch.autograd.Function):
    """a = act(sum_s x_s @ weight[:, c_s : c_s + w_s].T + bias) over dense device fp32 segments and / or device torch.sparse_csr ones:
    the one laff_fc_concat_act_bn launch forward (no BatchNorm stage), and behind it one call per segment on the column windows of
    weight and of ONE (D, K) gradient buffer -- pitched views, no copies: ops.fc_backward for a dense segment (dx only where that
    segment needs a gradient), ops.fc_gather_backward for a CSR one.  The windows cover dw, so nothing is zero-filled.  db is formed
    exactly once, by the FIRST segment's call.  `layer` is the TransformNet whose weight_t_block() the sparse segments gather from."""

    @staticmethod
    def forward(ctx, layer, activation, weight, bias, *segments):
        _fp32_params(weight, bias)
        segs, wt, shapes, saved, col = [], {}, [], [], 0
        for j, x in enumerate(segments):
            width = x.shape[1]
            if x.layout == torch.sparse_csr:
                wt[j] = layer.weight_t_block(col, width)
                shapes.append(tuple(x.shape))
                saved += list(_csc_of(x))
            else:
                _fp32(x, 'segment %d' % j)
                x = _dense_input(x)
                shapes.append(None)
                saved.append(x)
            segs.append(x)
            col += width
        a = ops.fc_concat_act_bn(segs, weight.detach(), _detached(bias), None, None, activation, weight_t=wt)
        ctx.save_for_backward(weight, a, *saved)
        ctx.activation, ctx.has_bias, ctx.csr_shapes = activation, bias is not None, shapes
        return a

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_a):
        weight, a, *saved = ctx.saved_tensors
        need = ctx.needs_input_grad
        w = weight.detach()
        dw = torch.empty_like(w, memory_format=torch.contiguous_format) if need[2] else None
        db = torch.empty((w.shape[0],), device=w.device, dtype=torch.float32) if ctx.has_bias and need[3] else None
        dxs, col = [], 0
        for j, (shape, x) in enumerate(_saved_segments(ctx.csr_shapes, saved)):
            first_db = db if j == 0 else None
            width = x.shape[1] if shape is None else shape[1]
            window = None if dw is None else dw[:, col:col + width]
            if shape is not None:
                ops.fc_gather_backward(x, shape[0], width, a, grad_a, ctx.activation, want_dw=dw is not None,
                                       want_db=first_db is not None, out=(window, first_db))
                dxs.append(None)
            else:
                dxs.append(ops.fc_backward(x, w[:, col:col + width], a, grad_a, ctx.activation, want_dx=need[4 + j],
                                           want_dw=dw is not None, want_db=first_db is not None, out=(None, window, first_db))[0])
            col += width
        return (None, None, dw, db) + tuple(dxs)


class _FcConcatGroupedFn(_FcConcatFn):
    """_FcConcatFn's forward with ONE ops.fc_concat_backward call behind it: a launch writes the column
    windows of dw for all dense segments and db, a launch the dx of every dense segment that needs a gradient, and a CSR segment's
    window is one gather launch inside the same call.  The training route of the W2VV++ video tower (TransformNet.concat_train with
    grouped=True); _FcConcatFn stays what concat_train runs by default, what the text tower takes and what this one is compared with."""

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_a):
        weight, a, *saved = ctx.saved_tensors
        need = ctx.needs_input_grad
        segs, want_dx = [], []
        for j, (shape, x) in enumerate(_saved_segments(ctx.csr_shapes, saved)):
            segs.append(x)
            want_dx.append(shape is None and need[4 + j])
        dxs, dw, db = ops.fc_concat_backward(segs, weight.detach(), a, grad_a, ctx.activation, want_dx=want_dx, want_dw=need[2],
                                             want_db=ctx.has_bias and need[3])
        return (None, None, dw, db) + tuple(dxs)


class _DropoutBnFn(torch.autograd.Function):
    """y = BatchNorm1d(dropout(a)) in training mode on laff_dropout_bn_train, ops.dropout_bn_train_backward behind it (DESIGN.md
    section 4.25).  The dropout mask is a function of (seed, row, column): the seed is saved, the mask and the dropped activations are
    not, and a is the tensor that _FcActFn saved already.  running_mean / running_var are updated in place by the kernel.  weight
    None: no BatchNorm stage."""

    @staticmethod
    def forward(ctx, a, weight, bias, running_mean, running_var, p, momentum, eps):
        a = a.detach()
        # a fresh seed per forward from torch's device generator: torch.manual_seed governs it, nothing synchronises, and a captured
        # step draws a new one on every replay
        seed = torch.empty(1, dtype=torch.int64, device=a.device).random_() if p else None
        y, mean, invstd = ops.dropout_bn_train(a, p or 0.0, seed, _detached(weight), _detached(bias), running_mean, running_var,
                                               momentum, eps)
        ctx.save_for_backward(a, weight, seed, mean, invstd)
        ctx.p = p or 0.0
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        a, weight, seed, mean, invstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        bn = weight is not None
        da, dgamma, dbeta = ops.dropout_bn_train_backward(grad_y, a, ctx.p, seed, _detached(weight), mean, invstd,
                                                          want_da=need[0], want_dgamma=bn and need[1], want_dbeta=bn and need[2])
        return da, dgamma, dbeta, None, None, None, None, None


class _TileBnFn(torch.autograd.Function):
    """y = BatchNorm1d(heads * C)(x.repeat(1, heads)) in training mode on laff_tile_bn_train, ops.tile_bn_train_backward behind it
    (DESIGN.md section 4.26): the no-transform feature of the LAFF towers.  The tiled input is never formed; the statistics are saved per
    input column.  x receives its gradient summed over the heads (the frame attention trains through it); a pre-extracted feature
    needs none, and its launch walks no row twice.  running_mean / running_var are updated in place by the kernel."""

    @staticmethod
    def forward(ctx, x, heads, weight, bias, running_mean, running_var, momentum, eps):
        _fp32(x, 'the input')
        x = _dense_input(x)
        y, mean, invstd = ops.tile_bn_train(x, heads, weight.detach(), bias.detach(), running_mean, running_var, momentum, eps)
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.heads = heads
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, mean, invstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dgamma, dbeta = ops.tile_bn_train_backward(grad_y, x, ctx.heads, weight.detach(), mean, invstd, want_dx=need[0],
                                                       want_dgamma=need[2], want_dbeta=need[3])
        return dx, None, dgamma, dbeta, None, None, None, None


class _ExpertStageFn(torch.autograd.Function):
    """The expert stage of a tower in training mode on laff_expert_stage_train, ops.expert_stage_train_backward behind it (DESIGN.md
    section 4.27): stacked[n, l, :] = l2norm(planes[l][n, :] + expert[l, :]) over all columns, either part optional, one launch each way
    for all planes.  Returns the stacked (N, L, D) tensor that the fusion reads in place.  Every plane receives its gradient (one
    launch writes them all), the expert table its column sums when it asks for them.  Saves the planes and the row norms, not the
    output."""

    @staticmethod
    def forward(ctx, l2norm, expert, *planes):
        for i, t in enumerate(planes):
            _fp32(t, 'plane %d' % i)
        _fp32(expert, 'the expert table')
        planes = [_dense_input(t) for t in planes]
        e = None if expert is None else expert.detach()
        stacked, rnorm = ops.expert_stage_train(planes, e, l2norm)
        ctx.save_for_backward(*[t for t in (e, rnorm) if t is not None], *planes)
        ctx.meta = (bool(l2norm), e is not None)
        return stacked

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_stacked):
        l2norm, has_expert = ctx.meta
        saved = list(ctx.saved_tensors)
        e = saved.pop(0) if has_expert else None
        rnorm = saved.pop(0) if l2norm else None
        dxs, d_expert = ops.expert_stage_train_backward(grad_stacked, saved, e, l2norm, rnorm,
                                                        want_d_expert=has_expert and ctx.needs_input_grad[1])
        return (None, d_expert) + tuple(dxs)
