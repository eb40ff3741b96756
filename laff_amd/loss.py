"""loss.l2norm / loss.cosine_sim / loss.hist_sim / loss.jaccard_sim of the reference (/root/reference/loss.py:8-65) on the HIP kernels."""
import torch

from . import ops

#: operand precision of the similarity GEMM; 'fp16' meets the 1e-4 cosine contract, 'fp16x3' is ~1e-7.
DEFAULT_PRECISION = 'fp16'


def l2norm(X, eps=1e-13, dim=1):
    """X / (sqrt(sum X^2 along dim) + eps + 1e-14); dim must be the last axis of a 2-D/3-D tensor."""
    if (X.dim() == 2 and dim in (1, -1)) or (X.dim() == 3 and dim in (2, -1)):
        # pack_rows never allocates less than 16 bytes: a result of fewer than four floats is the front of its buffer
        return ops.pack_rows(X.contiguous(), True, eps, 'fp32', 1.0).buf[:4 * X.numel()].view(torch.float32).view(X.shape)
    raise NotImplementedError('l2norm along dim=%d of a %d-D tensor is outside the hot path' % (dim, X.dim()))


def cosine_sim(query, retrio, precision=None):
    """l2norm(query) @ l2norm(retrio).T  (loss.py:30-34): re-normalises both operands like the reference."""
    precision = precision or DEFAULT_PRECISION
    q = ops.pack_rows(query.contiguous(), True, 1e-13, precision)
    r = ops.pack_rows(retrio.contiguous(), True, 1e-13, precision)
    return ops.sim_gemm(q, r, heads=1)


def hist_sim(im, s, eps=1e-14):
    """sum min(im, s) / (sum max(im, s) + eps) of every row of im against every row of s (loss.py:43-50).  The reference's version
    expands both sides by im's row count and so only works on square input; any (N_im, N_s) is accepted here."""
    return ops.sim_hist(im, s, 1, eps)


def jaccard_sim(query, retrieval_base, eps=1e-8):
    """The same measure as the reference's per-query loop states it (loss.py:53-65): (N_query, N_base)."""
    return ops.sim_hist(query, retrieval_base, 1, eps)


# ---- training loss ---------------------------------------------------------------------------
class _MarginRankingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, im, margin, max_violation, cost_style, direction):
        need = s.requires_grad or im.requires_grad
        loss, d_s, d_im = ops.margin_loss(s.detach(), im.detach(), margin, max_violation, cost_style, direction, want_grad=need)
        ctx.save_for_backward(d_s, d_im) if need else None
        ctx.has_grad = need
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.has_grad:
            return (None,) * 6
        d_s, d_im = ctx.saved_tensors
        return grad_out * d_s, grad_out * d_im, None, None, None, None


class MarginRankingLoss(torch.nn.Module):
    """loss.MarginRankingLoss (/root/reference/loss.py:68-135) with measure='cosine': forward(s, im) on (B, d) inputs as the
    reference, or on (B, H, d) for the per-head sum of model/model.py:2032-2048 in one call.  Forward and backward run in
    liblaff_hip.so (laff_margin_loss); the module plugs into autograd."""

    def __init__(self, margin=0, measure='cosine', max_violation=False, cost_style='sum', direction='bidir', device=None):
        super().__init__()
        # measure='hist' stays refused: the scores exist (hist_sim above), the margin loss on them and its backward do not
        if measure != 'cosine':
            raise NotImplementedError("only measure='cosine' is on the path ('hist' is the Jaccard variant of task 2)")
        self.margin, self.max_violation, self.cost_style, self.direction = margin, max_violation, cost_style, direction

    def forward(self, s, im):
        return _MarginRankingFn.apply(s, im, self.margin, self.max_violation, self.cost_style, self.direction)


class _DualSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, im, temp):
        need = s.requires_grad or im.requires_grad
        loss, d_s, d_im = ops.dsl_loss(s.detach(), im.detach(), temp, want_grad=need)
        ctx.save_for_backward(d_s, d_im) if need else None
        ctx.has_grad = need
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.has_grad:
            return (None,) * 3
        d_s, d_im = ctx.saved_tensors
        return grad_out * d_s, grad_out * d_im, None


class DualSoftmaxLoss(torch.nn.Module):
    """loss.DualSoftmaxLoss (/root/reference/loss.py:291-310): forward(s, im, temp=1000) on (B, d) inputs as the reference, or on
    (B, H, d) for the per-head sum of model/model.py:2032-2048 in one call.  Forward and backward run in liblaff_hip.so
    (laff_dsl_loss); the module plugs into autograd."""

    def forward(self, s, im, temp=1000):
        if not (torch.is_grad_enabled() and (s.requires_grad or im.requires_grad)):       # e.g. under torch.no_grad(): forward only
            return ops.dsl_loss(s.detach(), im.detach(), temp, want_grad=False)[0]
        return _DualSoftmaxFn.apply(s, im, temp)


class _MarginScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, margin, max_violation, cost_style, direction):
        need = score.requires_grad
        loss, d_score = ops.margin_loss_scores(score.detach(), margin, max_violation, cost_style, direction, want_grad=need)
        ctx.save_for_backward(d_score) if need else None
        ctx.has_grad = need
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.has_grad:
            return (None,) * 5
        d_score, = ctx.saved_tensors
        return grad_out * d_score, None, None, None, None


class MarginRankingLossWithScore(torch.nn.Module):
    """loss.MarginRankingLossWithScore (/root/reference/loss.py:138-200): forward(score) on a (B, B) score matrix the caller formed;
    cost_s compares along the rows, cost_im along the columns.  Runs in liblaff_hip.so (laff_margin_loss_scores), on autograd."""

    def __init__(self, margin=0, max_violation=False, cost_style='sum', direction='bidir', device=None):
        super().__init__()
        self.margin, self.max_violation, self.cost_style, self.direction = margin, max_violation, cost_style, direction

    def forward(self, score):
        if not (torch.is_grad_enabled() and score.requires_grad):
            return ops.margin_loss_scores(score.detach(), self.margin, self.max_violation, self.cost_style, self.direction,
                                          want_grad=False)[0]
        return _MarginScoreFn.apply(score, self.margin, self.max_violation, self.cost_style, self.direction)


def criterion_for(opt, device=None):
    """The criterion that opt.loss selects (model/model.py:1988-2000): 'mrl' -> MarginRankingLoss from opt.margin, opt.measure,
    opt.max_violation, opt.cost_style and opt.direction; 'dsl' -> DualSoftmaxLoss."""
    if opt.loss == 'mrl':
        return MarginRankingLoss(margin=opt.margin, measure=opt.measure, max_violation=opt.max_violation, cost_style=opt.cost_style,
                                 direction=opt.direction, device=device)
    if opt.loss == 'dsl':
        return DualSoftmaxLoss()
    if opt.loss == 'CELoss':
        raise NotImplementedError("loss='CELoss': the reference's own CrossEntropyLoss.forward raises TypeError (loss.py:278 passes "
                                  'temp to a cal_loss that does not take it), so there is no behaviour to reproduce')
    raise Exception('Not such loss.')


def compute_loss_with_score(criterion_with_score, scores):
    """The other branch of W2VVPP_MultiHeadAttention.compute_loss (model/model.py:2040-2042): the embeddings are not multi-space 3-D,
    the caller forms the text-to-video score matrix and criterion_with_score (MarginRankingLossWithScore) is applied to it.
    Returns (loss, {'triplet_loss': loss})."""
    loss = criterion_with_score(scores)
    return loss, {'triplet_loss': loss}


def compute_loss(criterion, vis_embs, txt_embs):
    """W2VVPP_MultiHeadAttention.compute_loss with multi_space=True (model/model.py:2032-2048): one criterion per head, summed.
    Returns (loss, {'triplet_loss': loss})."""
    if vis_embs.dim() != txt_embs.dim() or vis_embs.dim() not in (2, 3):
        raise Exception('vis_embs dims are not equal to txt_embs dims')
    loss = criterion(txt_embs, vis_embs)
    return loss, {'triplet_loss': loss}
