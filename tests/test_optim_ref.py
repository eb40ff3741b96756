"""Host checks of the optimizer step: the float64 formulas of tests/optim_ref.py against torch's own clip_grad_norm_ and
optimizers in float64, laff_optim_plan (which needs no GPU), what laff_amd.optim refuses, optimizer_for and the state_dict interchange."""
import types

import numpy as np
import pytest
import torch

import optim_ref as R

SHAPES = [(5, 3), (7,), (1,), (2, 3, 4)]


def _problem(seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
    grads = [[torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-3, 1, (1,), generator=g)) for s in SHAPES]
             for _ in range(5)]
    return params, grads


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_formulas_equal_torch_in_float64(kind, wd):
    params, grads = _problem(5)
    max_norm = 0.5 * min(R.total_norm([g.numpy() for g in gs]) for gs in grads)               # clipping active at every step
    tp = [torch.nn.Parameter(p.clone()) for p in params]
    if kind == 'adam':
        opt = torch.optim.Adam(tp, lr=1e-2, betas=(0.9, 0.999), eps=1e-4, weight_decay=wd)
    else:
        opt = torch.optim.RMSprop(tp, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=wd)
    p = [t.numpy().copy() for t in params]
    s1 = [np.zeros_like(t) for t in p]
    s2 = [np.zeros_like(t) for t in p]
    for step, gs in enumerate(grads, 1):
        for t, g in zip(tp, gs):
            t.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        gn = [g.numpy() for g in gs]
        mine = R.total_norm(gn)
        assert abs(mine - float(total)) <= 1e-13 * mine
        c = R.clip_coef(mine, max_norm)
        assert c < 1.0
        for t, g in zip(tp, gn):                                                              # the clipped gradients themselves
            np.testing.assert_allclose(t.grad.numpy(), c * g, rtol=0, atol=1e-13 * np.abs(g).max())
        if kind == 'adam':
            p, s1, s2 = R.adam(p, gn, s1, s2, 1e-2, 0.9, 0.999, 1e-4, wd, step, c)
        else:
            p, s1 = R.rmsprop(p, gn, s1, 1e-2, 0.99, 1e-8, wd, c)
    for mine, t in zip(p, tp):
        err = np.abs(mine - t.detach().numpy()).max() / np.abs(t.detach().numpy()).max()
        print('%s wd=%g: %.2e' % (kind, wd, err))
        assert err <= 1e-13
    keys = ('exp_avg', 'exp_avg_sq') if kind == 'adam' else ('square_avg',)
    for key, mine in zip(keys, (s1, s2)):
        for a, t in zip(mine, tp):
            r = opt.state[t][key].numpy()
            assert np.abs(a - r).max() <= 1e-13 * np.abs(r).max()


def test_clip_coef_edges():
    assert R.clip_coef(4.0, 0.0) == 1.0 and R.clip_coef(4.0, 8.0) == 1.0
    assert R.clip_coef(4.0, 2.0) == 2.0 / (4.0 + 1e-6)
    assert np.isnan(R.clip_coef(float('nan'), 2.0))
    assert R.clip_coef(float('inf'), 2.0) == 0.0


def test_plan_needs_no_gpu():
    from laff_amd import ops
    chunk, capacity, norm, partials, update, cap = ops.optim_plan([])
    assert chunk > 0 and capacity > 0 and cap > 0 and chunk % 4 == 0
    assert (norm, partials, update) == (0, 0, 0)
    assert ops.optim_plan([1])[2:5] == (1, 1, 1)
    assert ops.optim_plan([0, 0])[2:5] == (0, 0, 0)                                           # empty tensors take no table entry
    assert ops.optim_plan([3] * capacity)[2:5] == (1, capacity, 1)
    assert ops.optim_plan([3] * (capacity + 1))[2:5] == (2, capacity + 1, 2)
    assert ops.optim_plan([3] * capacity + [0, 0])[2:5] == (1, capacity, 1)
    assert ops.optim_plan([chunk - 1, chunk, chunk + 1, 3 * chunk + 5])[2:5] == (1, 1 + 1 + 2 + 4, 1)
    # more chunks than blocks: the grid is capped and strides, and so are the partials
    assert ops.optim_plan([cap * chunk])[2:5] == (1, cap, 1)
    assert ops.optim_plan([cap * chunk + 3])[2:5] == (1, cap, 1)
    assert ops.optim_plan([cap * chunk + 3, 5])[2:5] == (1, cap, 1)
    with pytest.raises(RuntimeError, match='n=-1'):
        ops.optim_plan([4, -1])


def _param(shape=(4, 3), dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.zeros(shape, dtype=dtype))
    if grad:
        p.grad = torch.ones(shape, dtype=dtype)
    return p


def test_refusals_name_what_is_missing(monkeypatch):
    from laff_amd import optim
    for flag in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'foreach', 'fused', 'decoupled_weight_decay'):
        with pytest.raises(ValueError, match='Adam: %s=True is not supported' % flag):
            optim.Adam([_param()], **{flag: True})
    for flag in ('centered', 'maximize', 'capturable', 'differentiable', 'foreach'):
        with pytest.raises(ValueError, match='RMSprop: %s=True is not supported' % flag):
            optim.RMSprop([_param()], **{flag: True})
    with pytest.raises(ValueError, match='RMSprop: momentum=0.9 is not supported'):
        optim.RMSprop([_param()], momentum=0.9)
    with pytest.raises(ValueError, match='betas'):
        optim.Adam([_param()], betas=(0.9, 1.0))
    with pytest.raises(ValueError, match='alpha'):
        optim.RMSprop([_param()], alpha=1.0)
    with pytest.raises(ValueError, match='grad_clip'):
        optim.Adam([_param()], grad_clip=-1.0)
    # a flag that arrives later, through param_groups or a loaded state_dict, is refused by step()
    late = optim.Adam([_param()])
    late.param_groups[0]['amsgrad'] = True
    with pytest.raises(ValueError, match='amsgrad=True'):
        late.step()
    for cls in (optim.Adam, optim.RMSprop):
        name = cls.__name__
        with pytest.raises(TypeError, match='%s: parameters must be torch.float32' % name):
            cls([_param(dtype=torch.float64)]).step()
        strided = torch.nn.Parameter(torch.zeros(3, 4).t())
        strided.grad = torch.ones(4, 3)
        with pytest.raises(ValueError, match='%s: parameters must be contiguous' % name):
            cls([strided]).step()
        sparse = _param((4, 3), grad=False)
        sparse.grad = torch.eye(4, 3).to_sparse()
        with pytest.raises(NotImplementedError, match='%s: sparse gradients' % name):
            cls([sparse]).step()                                                                  # refused before the device is looked at
        with pytest.raises(RuntimeError, match='%s: .* must be CUDA .* no CPU path' % name):
            cls([_param()]).step()
        # nothing to do is not refused: no gradient anywhere
        assert cls([_param(grad=False)]).step() is None
        assert cls([_param(grad=False)]).step(lambda: 3.0) == 3.0                             # the closure's value comes back
        monkeypatch.setattr(optim, '_capturing', lambda: True)
        with pytest.raises(RuntimeError, match=r'%s\.step\(\) cannot be captured' % name):
            cls([_param()]).step()
        monkeypatch.undo()
    with pytest.raises(ValueError, match='norm_type=1 is not supported'):
        optim.clip_grad_norm_([_param()], 1.0, norm_type=1)
    with pytest.raises(ValueError, match='norm_type=inf'):
        optim.clip_grad_norm_([_param()], 1.0, norm_type=float('inf'))
    with pytest.raises(NotImplementedError, match='clip_grad_norm_: sparse'):
        optim.clip_grad_norm_([sparse], 1.0)
    with pytest.raises(RuntimeError, match='clip_grad_norm_: .* no CPU path'):
        optim.clip_grad_norm_([_param()], 1.0)
    with pytest.raises(RuntimeError, match='clip_grad_norm_: .* no CPU path'):                # any iterable, as torch: a generator is
        optim.clip_grad_norm_((p for p in [_param(grad=False), _param()]), 1.0)               # read once and still reaches the refusal
    with pytest.raises(RuntimeError, match='clip_grad_norm_: .* no CPU path'):
        optim.clip_grad_norm_(_with_grads(torch.nn.Linear(3, 2)).parameters(), 1.0)      # model.parameters(), the usual call
    assert float(optim.clip_grad_norm_([_param(grad=False)], 1.0)) == 0.0                     # torch's answer without gradients


def _with_grads(module):
    for p in module.parameters():
        p.grad = torch.ones_like(p)
    return module


def test_ops_refuse_cpu_tensors_and_unknown_kinds():
    from laff_amd import ops
    t = torch.zeros(4)
    with pytest.raises(RuntimeError, match=r'grads\[0\] must be a CUDA'):                      # a non-tensor entry is named, first or not
        ops.grad_sqnorm([None])
    with pytest.raises(RuntimeError, match=r'params\[0\] must be a CUDA'):
        ops.optim_step('adam', [3.0], [t], [t], [t], lr=1e-3, step=1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.grad_sqnorm([t])
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.grad_scale([t], 1.0, None, 0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.optim_step('adam', [t], [t], [t], [t], lr=1e-3, step=1)
    with pytest.raises(ValueError, match="unknown optimizer kind 'sgd'"):
        ops.optim_step('sgd', [t], [t], [t], [t], lr=1e-3, step=1)


class _Towers(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3)
        self.ClipModel_proj = torch.nn.Linear(3, 2, bias=False)


@pytest.mark.parametrize('name', ['adam', 'rmsprop'])
def test_optimizer_for_is_the_references(name):
    from laff_amd import optim
    model = _Towers()
    opt = types.SimpleNamespace(optimizer=name, lr=1e-3, grad_clip=2.0, lr_decay_rate=0.9)
    o, sched = optim.optimizer_for(opt, model)
    assert isinstance(o, torch.optim.Optimizer) and type(o) is (optim.Adam if name == 'adam' else optim.RMSprop)
    usual, special = o.param_groups
    assert [p is q for p, q in zip(usual['params'], (model.fc.weight, model.fc.bias))] == [True, True]
    assert len(special['params']) == 1 and special['params'][0] is model.ClipModel_proj.weight
    assert usual['lr'] == 1e-3 and special['lr'] == 1e-3 / 20
    assert usual['eps'] == (1e-4 if name == 'adam' else 1e-8)
    assert o.grad_clip == 2.0
    assert type(sched[0]) is torch.optim.lr_scheduler.StepLR and type(sched[1]) is torch.optim.lr_scheduler.ReduceLROnPlateau
    assert sched[0].step_size == 1 and sched[0].gamma == 0.9
    assert sched[1].mode == 'max' and sched[1].factor == 0.5 and sched[1].patience == 2
    sched[0].step()                                                                          # what the next step() reads
    assert o.param_groups[0]['lr'] == pytest.approx(0.9e-3, rel=1e-12) and o.param_groups[1]['lr'] == pytest.approx(0.9e-3 / 20, rel=1e-12)
    for bad in range(4):
        sched[1].step(0.0)                                                                   # no improvement: the plateau halves lr
    assert o.param_groups[0]['lr'] < 0.9e-3
    with pytest.raises(Exception, match='sgd'):
        optim.optimizer_for(types.SimpleNamespace(optimizer='sgd', lr=1e-3, grad_clip=2.0, lr_decay_rate=0.9), model)


@pytest.mark.parametrize('name', ['Adam', 'RMSprop'])
def test_state_dict_interchanges_with_torch(name):
    from laff_amd import optim
    kw = dict(lr=3e-3, eps=1e-4, weight_decay=0.01)
    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    theirs = getattr(torch.optim, name)([{'params': ps[:1]}, {'params': ps[1:], 'lr': 1e-4}], **kw)
    for p in ps:
        p.grad = torch.randn_like(p)
    theirs.step()
    theirs.step()
    sd = theirs.state_dict()
    mine = getattr(optim, name)([{'params': ps[:1]}, {'params': ps[1:]}], lr=1.0)
    mine.load_state_dict(sd)
    assert [g['lr'] for g in mine.param_groups] == [3e-3, 1e-4] and mine.param_groups[0]['eps'] == 1e-4
    keys = ('exp_avg', 'exp_avg_sq') if name == 'Adam' else ('square_avg',)
    for p in ps:
        assert float(mine.state[p]['step']) == 2.0 and not mine.state[p]['step'].is_cuda
        for k in keys:
            assert torch.equal(mine.state[p][k], theirs.state[p][k])
    back = getattr(torch.optim, name)([{'params': ps[:1]}, {'params': ps[1:]}], lr=1.0)
    back.load_state_dict(mine.state_dict())
    a, b = back.state_dict(), sd
    assert a['param_groups'] == b['param_groups']
    assert sorted(a['state']) == sorted(b['state'])
    for i in a['state']:
        assert sorted(a['state'][i]) == sorted(b['state'][i])
        for k in a['state'][i]:
            assert torch.equal(a['state'][i][k], b['state'][i][k])
    back.step()                                                                              # torch's step runs on what came back
    # a fresh optimizer's own state_dict has torch's group keys, so torch takes it as well
    fresh = getattr(optim, name)(ps, **kw).state_dict()
    want = getattr(torch.optim, name)(ps, **kw).state_dict()
    assert fresh['param_groups'] == want['param_groups'] and fresh['state'] == {}
