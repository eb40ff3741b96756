"""The last two stages of the reference's training step (model/model.py:964-1001) on the library's kernels: clip_grad_norm_ and
optimizer.step().

    clip_grad_norm_(parameters, max_norm)      torch.nn.utils.clip_grad_norm_ in two launches
    Adam, RMSprop                              torch.optim.Optimizer subclasses whose step() is one norm launch and one update launch
    optimizer_for(opt, model)                  the reference's optimizer and lr schedulers (model/model.py:2008-2028)

State layout, param_groups and state_dict are torch's, so the torch lr schedulers drive these optimizers as they are and a state_dict
moves between them and torch.optim.Adam / RMSprop in both directions.  There is no CPU path and no fallback to torch's step.
"""
import torch
from torch.optim import Optimizer

from . import ops

__all__ = ['clip_grad_norm_', 'Adam', 'RMSprop', 'optimizer_for']


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _checked_grad(p, who):
    """p.grad as the kernels take it (device fp32, contiguous -- a copy when it is not), refusing what they do not cover."""
    g = p.grad
    if g.is_sparse:
        raise NotImplementedError('%s: sparse gradients are not supported' % who)
    if g.dtype != torch.float32:
        raise TypeError('%s: gradients must be torch.float32, got %s' % (who, g.dtype))
    if not g.is_cuda:
        raise RuntimeError('%s: gradients must be CUDA (ROCm) tensors: laff_amd has no CPU path' % who)
    return g if g.is_contiguous() else g.contiguous()


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) for the L2 norm: every .grad is scaled in place by
    min(1, max_norm / (total_norm + 1e-6)) and the total norm comes back as a 0-d device tensor (error_if_nonfinite=False: a
    non-finite norm makes the gradients non-finite).  Parameters whose grad is None are skipped.  Two launch sets: the float64 partial
    sums of the squares, then the scaling.  norm_type other than 2 is refused."""
    if float(norm_type) != 2.0:
        raise ValueError('clip_grad_norm_: norm_type=%r is not supported, only norm_type=2' % (norm_type,))
    parameters = [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)        # any iterable, a generator included
    held = [p.grad for p in parameters if p.grad is not None]
    if not held:
        return torch.tensor(0.0)
    grads = [_checked_grad(p, 'clip_grad_norm_') for p in parameters if p.grad is not None]
    ws, partials = ops.grad_sqnorm(grads)
    total = ops.grad_scale(grads, max_norm, ws, partials)
    for g, c in zip(held, grads):
        if c is not g:                     # a non-contiguous grad was scaled in a dense copy
            g.copy_(c)
    return total


class _StepOptimizer(Optimizer):
    """What Adam and RMSprop share: the refusals, the lazily created state in torch's layout and the launch sets of a step."""
    _kind = None
    _states = ()
    _refused = ()          # (key, refused when this holds, message)

    def __init__(self, params, defaults, grad_clip):
        if not float(grad_clip) >= 0.0:
            raise ValueError('%s: grad_clip=%r must be >= 0' % (type(self).__name__, grad_clip))
        self.grad_clip = float(grad_clip)
        self.total_norm = None             # 0-d device tensor: the global norm of the last clipped step
        self._ws = None
        self._seen = {}                    # parameter -> the state tensors _advance has held to the kernels' contract
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    def _check_group(self, group):
        name = type(self).__name__
        for key, bad, what in self._refused:
            if key in group and bad(group[key]):
                raise ValueError('%s: %s=%r is not supported: %s' % (name, key, group[key], what))
        if not 0.0 <= group['lr']:
            raise ValueError('%s: lr=%r must be >= 0' % (name, group['lr']))
        if not 0.0 <= group['eps']:
            raise ValueError('%s: eps=%r must be >= 0' % (name, group['eps']))
        if not 0.0 <= group['weight_decay']:
            raise ValueError('%s: weight_decay=%r must be >= 0' % (name, group['weight_decay']))

    def _check_param(self, p):
        name = type(self).__name__
        if p.dtype != torch.float32:
            raise TypeError('%s: parameters must be torch.float32, got %s' % (name, p.dtype))
        if not p.is_contiguous():
            raise ValueError('%s: parameters must be contiguous, got shape %s strides %s' % (name, tuple(p.shape), p.stride()))

    def _hyper(self, group):
        raise NotImplementedError

    def _advance(self, ps):
        """Creates missing state in torch's layout, adds 1 to every 'step' and returns [(step value, state tensors)] per parameter.
        The 'step' scalars live on the host, as torch keeps them: one foreach call advances them and one stack reads them all back, so
        what a launch uses is always what the state holds.  State tensors are held to the kernels' contract when first seen (and
        again when load_state_dict has put other tensors there)."""
        name = type(self).__name__
        if not ps:
            return []
        steps = []
        for p in ps:
            st = self.state[p]
            if len(st) == 0:
                st['step'] = torch.tensor(0.0, dtype=torch.float32)
                for key in self._states:
                    st[key] = torch.zeros_like(p, memory_format=torch.preserve_format)
            steps.append(st['step'])
        torch._foreach_add_(steps, 1)
        if any(s.is_cuda for s in steps):  # a state_dict of a capturable / fused torch optimizer keeps them on the device
            values = [int(s.item()) for s in steps]
        else:
            values = [int(v) for v in torch.stack(steps).tolist()]
        out = []
        for p, value in zip(ps, values):
            st = self.state[p]
            states = self._seen.get(p)
            if states is None or not all(a is st[key] for a, key in zip(states, self._states)):
                states = [st[key] for key in self._states]
                for key, t in zip(self._states, states):
                    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == p.shape and t.device == p.device):
                        raise ValueError("%s: state '%s' must be a contiguous fp32 tensor of its parameter's shape and device, got %s %s on %s"
                                         % (name, key, t.dtype, tuple(t.shape), t.device))
                self._seen[p] = states
            out.append((value, states))
        return out

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        if _capturing():
            raise RuntimeError('%s.step() cannot be captured into a graph: step and lr are launch arguments, a replay would repeat '
                               'the captured ones' % name)
        work = []                          # per group: (group, params, grads)
        for group in self.param_groups:
            self._check_group(group)
            ps, gs = [], []
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                if not (g.is_cuda and p.is_cuda and not g.is_sparse and g.dtype == torch.float32 and p.dtype == torch.float32
                        and p.is_contiguous() and g.is_contiguous() and g.device == p.device):
                    self._check_param(p)                   # names what is wrong
                    g = _checked_grad(p, name)             # (or makes a strided gradient dense)
                    if not p.is_cuda:
                        raise RuntimeError('%s: parameters must be CUDA (ROCm) tensors: laff_amd has no CPU path' % name)
                    if g.device != p.device:
                        raise ValueError('%s: a gradient on %s belongs to a parameter on %s' % (name, g.device, p.device))
                ps.append(p)
                gs.append(g)
            work.append((group, ps, gs))
        every = [g for _, _, gs in work for g in gs]
        if not every:
            return loss
        clip = self.grad_clip > 0.0
        partials = 0
        if clip:                           # the norm runs once, over every group's gradients
            need = 8 * ops.optim_plan([g.numel() for g in every])[3]
            if self._ws is None or self._ws.numel() < need or self._ws.device != every[0].device:
                self._ws = torch.empty(max(need, 16), dtype=torch.uint8, device=every[0].device)
            _, partials = ops.grad_sqnorm(every, self._ws)
            if self.total_norm is None or self.total_norm.device != every[0].device:
                self.total_norm = torch.zeros((), dtype=torch.float32, device=every[0].device)
        for group, ps, gs in work:
            by_step = {}                   # one update launch set per distinct step value of the group
            for p, g, (step, states) in zip(ps, gs, self._advance(ps)):
                by_step.setdefault(step, []).append((p, g, states))
            for step, items in by_step.items():
                ops.optim_step(self._kind, [p for p, _, _ in items], [g for _, g, _ in items], [st[0] for _, _, st in items],
                               [st[1] for _, _, st in items] if len(self._states) > 1 else None, step=step,
                               max_norm=self.grad_clip if clip else 0.0, workspace=self._ws if clip else None, partials=partials,
                               total_norm_out=self.total_norm if clip else None, checked=True, **self._hyper(group))
                # the kernel wrote through raw pointers: the version counters are bumped here (no launch), as an in-place torch op would,
                # or whatever a module derived from a parameter (TransformNet._cached, the packed attention weights) would outlive the step
                torch.autograd.graph.increment_version([p for p, _, _ in items] + [t for _, _, st in items for t in st])
        return loss


_NO_FLAG = (('maximize', bool, 'the step descends'),
            ('capturable', bool, 'step and lr are launch arguments (DESIGN.md 4.21)'),
            ('differentiable', bool, 'the step is not recorded by autograd'),
            ('foreach', bool, 'the step runs on laff_optim_step, not on an implementation of torch'),
            ('fused', bool, 'the step runs on laff_optim_step, not on an implementation of torch'))


class Adam(_StepOptimizer):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) whose step() runs on laff_optim_step, plus grad_clip.

    With grad_clip > 0 step() clips by the global L2 norm of ALL groups' gradients inside the update: the parameters, exp_avg and
    exp_avg_sq it leaves are those of torch.nn.utils.clip_grad_norm_(params, grad_clip) followed by torch's step, but .grad is left as
    it was (the scaled gradient only exists in registers); the norm is kept in .total_norm (0-d device tensor).  lr is read from
    param_groups at every call, so torch's lr schedulers work unchanged; state is created on the first step in torch's layout ('step' a
    CPU fp32 scalar, 'exp_avg', 'exp_avg_sq'), so state_dict() / load_state_dict() interchange with torch.optim.Adam.  grad_clip is a
    constructor argument, not part of the state_dict.

    Refused, naming the argument: amsgrad, maximize, capturable, differentiable, foreach, fused, decoupled_weight_decay; parameters
    that are not contiguous fp32 device tensors; sparse gradients (NotImplementedError); a capturing stream."""
    _kind = 'adam'
    _states = ('exp_avg', 'exp_avg_sq')
    _refused = (('amsgrad', bool, 'the maximum of the second moments is not kept'),) + _NO_FLAG + (
        ('decoupled_weight_decay', bool, 'weight decay enters the gradient'),
        ('betas', lambda b: not (0.0 <= b[0] < 1.0 and 0.0 <= b[1] < 1.0), 'both must lie in [0, 1)'))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, grad_clip=0.0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults, grad_clip)

    def _hyper(self, group):
        return dict(lr=group['lr'], beta1=group['betas'][0], beta2=group['betas'][1], eps=group['eps'], weight_decay=group['weight_decay'])


class RMSprop(_StepOptimizer):
    """torch.optim.RMSprop(params, lr, alpha, eps, weight_decay) with momentum 0, not centered, whose step() runs on laff_optim_step,
    plus grad_clip (see Adam: the clip is by the global norm of all groups and leaves .grad as it was).  State: 'step' and
    'square_avg', interchangeable with torch.optim.RMSprop through state_dict().

    Refused, naming the argument: momentum != 0, centered, maximize, capturable, differentiable, foreach; parameters that are not
    contiguous fp32 device tensors; sparse gradients (NotImplementedError); a capturing stream."""
    _kind = 'rmsprop'
    _states = ('square_avg',)
    _refused = (('momentum', lambda m: m != 0, 'there is no momentum buffer'),
                ('centered', bool, 'the mean of the gradients is not kept')) + _NO_FLAG + (
        ('alpha', lambda a: not 0.0 <= a < 1.0, 'it must lie in [0, 1)'),)

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, capturable=False, foreach=None,
                 maximize=False, differentiable=False, grad_clip=0.0):
        defaults = dict(lr=lr, momentum=momentum, alpha=alpha, eps=eps, centered=centered, weight_decay=weight_decay,
                        capturable=capturable, foreach=foreach, maximize=maximize, differentiable=differentiable)
        super().__init__(params, defaults, grad_clip)

    def _hyper(self, group):
        return dict(lr=group['lr'], beta2=group['alpha'], eps=group['eps'], weight_decay=group['weight_decay'])


def optimizer_for(opt, model, adam_eps=1e-4):
    """The reference's optimizer and schedulers (model/model.py:2008-2028) for `model`: parameters whose name contains 'BertModel',
    'csn_model' or 'ClipModel' form a second group at opt.lr / 20; opt.optimizer 'adam' -> Adam(lr, eps=adam_eps: the multi-head
    class's 1e-4, :2022; the base class keeps torch's 1e-8, :825), 'rmsprop' ->
    RMSprop(lr), both clipping at opt.grad_clip inside the step.  Returns (optimizer, [StepLR(step_size=1, gamma=opt.lr_decay_rate),
    ReduceLROnPlateau(mode='max', factor=0.5, patience=2)])."""
    special, usual = [], []
    for name, p in model.named_parameters():
        (special if ('BertModel' in name or 'csn_model' in name or 'ClipModel' in name) else usual).append(p)
    params = [{'params': usual}, {'params': special, 'lr': opt.lr / 20}]
    if opt.optimizer == 'adam':
        optimizer = Adam(params, lr=opt.lr, eps=adam_eps, grad_clip=opt.grad_clip)
    elif opt.optimizer == 'rmsprop':
        optimizer = RMSprop(params, lr=opt.lr, grad_clip=opt.grad_clip)
    else:
        raise Exception('Not such optimizer: %r' % (opt.optimizer,))
    schedulers = [torch.optim.lr_scheduler.StepLR(optimizer, step_size=1, gamma=opt.lr_decay_rate),
                  torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='max', factor=0.5, patience=2)]
    return optimizer, schedulers
