"""laff_tile_bn_train, its backward, the ops and TransformNet(fc=False, device_norm=True) on the MI355X.

The contract is an equality of bits: Y, running_mean, running_var, dgamma and dbeta are those of ops.dropout_bn_train(_backward) with
p = 0 on the materialised x.repeat(1, H), and save_mean[c] / save_invstd[c] are that run's entries h C + c for every h.  dX, which the
materialised route forms per copy, is checked against the float64 graph (torch's BatchNorm1d over x.repeat(1, H) on the CPU) under the
rule of tests/train_ref.py: max |device - float64| / max |float64| <= max(4 e32, TOL_UNIT), e32 the same error of the same graph in
float32 CPU torch.
"""
import functools

import pytest
import torch

import fc_bwd_ref
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
EPS = 1e-5
ROWS = 256                                                 # rows of a chunk (asserted against the plan below)
# (N, C, H, layout of train_ref.pitch)
CASES = [(2, 4, 2, 'dense'), (7, 36, 3, 'pitch4'),
         (8, 30, 2, 'pitch3'),                             # the element-wise path
         (256, 32, 8, 'dense'),                            # the largest uncut N
         (257, 36, 2, 'offset'),                           # a one-row second chunk
         (300, 64, 4, 'window')]


def _id(c):
    return 'N%d-C%d-H%d-%s' % c


def _momentum(c):
    return 0.1 if (c[0] + c[1]) % 2 else 0.5


def _graph(dtype, cs):
    """BatchNorm1d(H C) in training mode over x.repeat(1, H) as a CPU torch graph in `dtype`, driven backwards by dy."""
    N, C, H, _ = cs['c']
    norm = torch.nn.BatchNorm1d(H * C, eps=EPS, momentum=cs['momentum']).to(dtype).train()
    with torch.no_grad():
        norm.weight.copy_(cs['gamma'])
        norm.bias.copy_(cs['beta'])
        norm.running_mean.copy_(cs['rm'])
        norm.running_var.copy_(cs['rv'])
    x = cs['x'].clone().to(dtype).requires_grad_(True)
    y = norm(x.repeat(1, H))
    y.backward(cs['dy'].to(dtype))
    out = dict(y=y, dx=x.grad, dgamma=norm.weight.grad, dbeta=norm.bias.grad, running_mean=norm.running_mean, running_var=norm.running_var)
    return {k: v.detach().double() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _case(c):
    """The fp32 operands of a case on the CPU and the float64 / float32 graphs -- computed once, shared, never written."""
    N, C, H, _ = c
    g = torch.Generator().manual_seed(N * 1000003 + C * 1009 + H)
    x = torch.randn(N, C, generator=g)
    dy = torch.randn(N, H * C, generator=g)
    gamma, beta = torch.randn(H * C, generator=g), torch.randn(H * C, generator=g)
    rm, rv = torch.randn(H * C, generator=g), torch.rand(H * C, generator=g) + 0.5
    if C >= 4:
        x[:, 1] = 30.0 + 0.01 * torch.randn(N, generator=g)           # mean 30, standard deviation 0.01: an E[x^2] - mean^2 kernel fails here
        x[:, 2] = 0.0                                                  # a constant column: invstd = 1 / sqrt(eps)
        gamma[3] = 0.0                                                 # head 0 of column 3 passes nothing back, the other heads do
    cs = dict(c=c, x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, momentum=_momentum(c))
    cs['ref'], cs['f32'] = _graph(torch.float64, cs), _graph(torch.float32, cs)
    return cs


def _vec(t, layout, held):
    buf, view = TR.out_vec(t.numel(), aligned=layout in ('dense', 'pitch4'))
    view.copy_(t)
    held.append((buf, view))
    return view


def _run(c, want=(True, True, True), layout=None):
    """Forward and backward through the ops with every operand and output inside NaN frames of the case's layout; the outputs by name
    on the CPU (absent backward outputs: None) after the frames were checked."""
    from laff_amd import ops
    cs = _case(c)
    N, C, H, lay = c
    lay = layout or lay
    held = []

    def mat(t):
        held.append(TR.place(t, lay))
        return held[-1][1]

    def vec(t):
        return _vec(t, lay, held)
    x, dy = mat(cs['x']), mat(cs['dy'])
    y = mat(torch.full((N, H * C), NAN))
    gamma, beta, rm, rv = vec(cs['gamma']), vec(cs['beta']), vec(cs['rm']), vec(cs['rv'])
    sm, si = vec(torch.full((C,), NAN)), vec(torch.full((C,), NAN))
    res = ops.tile_bn_train(x, H, gamma, beta, rm, rv, cs['momentum'], EPS, out=(y, sm, si))
    assert res[0].data_ptr() == y.data_ptr() and res[1].data_ptr() == sm.data_ptr() and res[2].data_ptr() == si.data_ptr()
    dx = mat(torch.full((N, C), NAN)) if want[0] else None
    dg, db = (vec(torch.full((H * C,), NAN)) if want[1] else None), (vec(torch.full((H * C,), NAN)) if want[2] else None)
    back = ops.tile_bn_train_backward(dy, x, H, gamma, sm, si, *want, out=(dx, dg, db))
    assert all((r is None) == (not w) for r, w in zip(back, want))
    out = dict(y=y, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv, dx=back[0], dgamma=back[1], dbeta=back[2])
    torch.cuda.synchronize()
    for buf, view in held:
        assert TR.untouched_around(buf, view), 'a write outside a buffer or into the slack of a pitch'
    for k, t in out.items():
        assert t is None or not t.isnan().any(), '%s: an element was not written (or read a NaN)' % k
    assert torch.equal(x.cpu(), cs['x']) and torch.equal(dy.cpu(), cs['dy']) and torch.equal(gamma.cpu(), cs['gamma'])
    return {k: (None if t is None else t.detach().cpu().clone()) for k, t in out.items()}


@functools.lru_cache(maxsize=None)
def _materialised(c):
    """The route the contract names: ops.dropout_bn_train(_backward) with p = 0 on x.repeat(1, H), dense."""
    from laff_amd import ops
    cs = _case(c)
    N, C, H, _ = c
    xr = cs['x'].to(DEV).repeat(1, H)
    gamma, rm, rv = cs['gamma'].to(DEV), cs['rm'].to(DEV), cs['rv'].to(DEV)
    y, sm, si = ops.dropout_bn_train(xr, 0.0, None, gamma, cs['beta'].to(DEV), rm, rv, cs['momentum'], EPS)
    da, dg, db = ops.dropout_bn_train_backward(cs['dy'].to(DEV), xr, 0.0, None, gamma, sm, si)
    out = dict(y=y, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv, da=da, dgamma=dg, dbeta=db)
    return {k: t.cpu() for k, t in out.items()}


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_bits_of_the_materialised_route_and_dx_vs_float64(c):
    from laff_amd import ops
    N, C, H, layout = c
    assert ops.tile_bn_train_plan(ROWS, 8, 2)[0] == 1 and ops.tile_bn_train_plan(ROWS + 1, 8, 2)[0] == 2
    cs, want = _case(c), _materialised(c)
    got = _run(c)
    for k in ('y', 'running_mean', 'running_var', 'dgamma', 'dbeta'):
        assert torch.equal(got[k], want[k]), '%s: not the bits of the materialised route' % k
    for h in range(H):
        assert torch.equal(got['save_mean'], want['save_mean'][h * C:(h + 1) * C])
        assert torch.equal(got['save_invstd'], want['save_invstd'][h * C:(h + 1) * C])
    worst = TR.compare({k: got[k] for k in ('dx', 'y', 'dgamma', 'dbeta', 'running_mean', 'running_var')}, cs['ref'], cs['f32'], _id(c))
    print('%s worst err / bound %.3f' % (_id(c), worst))
    if C >= 4:
        assert got['save_mean'][2] == 0 and got['save_invstd'][2] == torch.tensor(1.0 / EPS ** 0.5, dtype=torch.float32)
        assert all(got['dgamma'][h * C + 2] == 0 for h in range(H))
    # two runs: equal bits
    again = _run(c)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # the other kernels (16-byte where the case is element-wise, and the other way round): equal bits
    other = _run(c, layout='pitch3' if layout in ('dense', 'pitch4') else 'dense')
    assert all(torch.equal(got[k], other[k]) for k in got)
    # each nullable output absent in turn, then dbeta alone: the others keep their bits
    for want3 in ((False, True, True), (True, False, True), (True, True, False), (False, False, True)):
        part = _run(c, want3)
        for w, k in zip(want3, ('dx', 'dgamma', 'dbeta')):
            assert (part[k] is None) == (not w)
            assert part[k] is None or torch.equal(part[k], got[k]), '%s changes when %s are formed' % (k, want3)
    none = _run(c, (False, False, False))
    assert none['dx'] is None and none['dgamma'] is None and none['dbeta'] is None


def test_refusals_of_the_ops():
    from laff_amd import ops
    v, x = torch.ones(14, device=DEV), torch.ones(4, 7, device=DEV)
    with pytest.raises(RuntimeError, match='N >= 2'):
        ops.tile_bn_train(x[:1], 2, v, v, v.clone(), v.clone(), 0.1, EPS)
    with pytest.raises(TypeError):
        ops.tile_bn_train(x.double(), 2, v, v, v.clone(), v.clone(), 0.1, EPS)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.tile_bn_train(x.cpu(), 2, v, v, v.clone(), v.clone(), 0.1, EPS)
    with pytest.raises(ValueError):
        ops.tile_bn_train(x, 3, v, v, v.clone(), v.clone(), 0.1, EPS)               # 14 channels are not 3 x 7
    with pytest.raises(ValueError, match='tiled over 2 heads'):
        ops.tile_bn_train_backward(torch.ones(4, 7, device=DEV), x, 2, v, v[:7].clone(), v[:7].clone())
    with pytest.raises(TypeError):
        ops.tile_bn_train_backward(torch.ones(4, 14, device=DEV).half(), x, 2, v, v[:7].clone(), v[:7].clone())


@pytest.mark.parametrize('c', CASES + [(257, 36, 2, 'dense')], ids=_id)        # every case, and the cut shape on the 16-byte kernels
def test_graph_capture_replays_the_eager_bits(c):
    """A forward plus backward captured on one stream, every operand and output in the case's layout, replays to the eager bits."""
    from laff_amd import ops
    cs = _case(c)
    N, C, H, layout = c
    held = []

    def mat(t):
        held.append(TR.place(t, layout))
        return held[-1][1]

    def vec(t):
        return _vec(t, layout, held)
    x, dy, gamma, beta = mat(cs['x']), mat(cs['dy']), vec(cs['gamma']), vec(cs['beta'])

    def step(rm, rv, outs):
        y, sm, si = ops.tile_bn_train(x, H, gamma, beta, rm, rv, cs['momentum'], EPS, out=outs[:3])
        ops.tile_bn_train_backward(dy, x, H, gamma, sm, si, out=outs[3:])

    def buffers():
        return [mat(torch.full((N, H * C), NAN)), vec(torch.full((C,), NAN)), vec(torch.full((C,), NAN)), mat(torch.full((N, C), NAN)),
                vec(torch.full((H * C,), NAN)), vec(torch.full((H * C,), NAN))]
    eager, rm_e, rv_e = buffers(), vec(cs['rm']), vec(cs['rv'])
    step(rm_e, rv_e, eager)
    outs, rm_g, rv_g = buffers(), vec(cs['rm']), vec(cs['rv'])
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        step(rm_g, rv_g, outs)
    assert torch.equal(rm_g.cpu(), cs['rm']) and outs[0].isnan().all()              # capturing runs nothing
    gr.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(outs + [rm_g, rv_g], eager + [rm_e, rv_e]))
    assert all(TR.untouched_around(buf, view) for buf, view in held), 'a write outside a buffer or into the slack of a pitch'
    want = _materialised(c)
    assert torch.equal(outs[0].cpu(), want['y']) and torch.equal(outs[4].cpu(), want['dgamma']) and torch.equal(outs[5].cpu(), want['dbeta'])
    assert torch.equal(rm_g.cpu(), want['running_mean']) and torch.equal(rv_g.cpu(), want['running_var'])


# ---- TransformNet(fc=False, batch_norm=True, device_norm=True) -----------------------------------------------------------------------
def _net(C, H, seed, dropout=None):
    from laff_amd.model.model import TransformNet
    torch.manual_seed(seed)
    net = TransformNet((C, H * C), dropout=dropout, batch_norm=True, activation=False, fc=False, device_norm=True)
    with torch.no_grad():
        net.bn1.weight.normal_(1.0, 0.3)
        net.bn1.bias.normal_(0.0, 0.3)
        net.bn1.running_mean.normal_(0.0, 0.3)
        net.bn1.running_var.uniform_(0.5, 1.5)
    return net


def _module_graphs(net, x, dE, H):
    state = {k: v.detach().clone() for k, v in net.bn1.state_dict().items()}
    out = []
    for dtype in (torch.float64, torch.float32):
        norm = torch.nn.BatchNorm1d(dE.shape[1], eps=net.bn1.eps, momentum=net.bn1.momentum).to(dtype).train()
        norm.load_state_dict(state)
        xs = x.clone().to(dtype).requires_grad_(True)
        y = norm(xs.repeat(1, H))
        y.backward(dE.to(dtype))
        assert int(norm.num_batches_tracked) == 1
        out.append({k: v.detach().double() for k, v in {
            'y': y, 'x.grad': xs.grad, 'bn1.weight.grad': norm.weight.grad, 'bn1.bias.grad': norm.bias.grad,
            'running_mean': norm.running_mean, 'running_var': norm.running_var}.items()})
    return out


@pytest.mark.parametrize('N, C, H', [(33, 36, 4), (300, 30, 2), (33, 132, 1)], ids=str)
def test_no_transform_layer_in_training_mode(N, C, H, monkeypatch):
    from laff_amd import ops
    net = _net(C, H, 21)
    x, dE = 2.0 * torch.randn(N, C) + 0.5, torch.randn(N, H * C)
    ref, f32 = _module_graphs(net, x, dE, H)
    net = net.to(DEV).train()
    calls = []
    for name in ('tile_bn_train', 'dropout_bn_train'):
        def spy(*a, _real=getattr(ops, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    xd = x.to(DEV).requires_grad_(True)
    pending = []
    src, tile, scale, shift = net.plane(xd, heads=H, pending=pending)
    assert pending == [] and tile is False and scale is None and shift is None and src.requires_grad and tuple(src.shape) == (N, H * C)
    assert calls == ['tile_bn_train' if H > 1 else 'dropout_bn_train']            # one launch, the tiled input is never formed
    src.backward(dE.to(DEV))
    assert int(net.bn1.num_batches_tracked) == 1
    got = {'y': src, 'x.grad': xd.grad, 'bn1.weight.grad': net.bn1.weight.grad, 'bn1.bias.grad': net.bn1.bias.grad,
           'running_mean': net.bn1.running_mean, 'running_var': net.bn1.running_var}
    TR.compare(got, ref, f32, 'N%d C%d H%d' % (N, C, H))


def test_only_the_wanted_gradients_are_formed(monkeypatch):
    from laff_amd import ops
    net = _net(36, 4, 22).to(DEV).train()
    x, dE = torch.randn(33, 36, device=DEV), torch.randn(33, 144, device=DEV)
    calls, real = [], ops.tile_bn_train_backward

    def spy(*args, **kw):
        calls.append({k: kw[k] for k in ('want_dx', 'want_dgamma', 'want_dbeta')})
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'tile_bn_train_backward', spy)
    y = net.plane(x, heads=4)[0]                                                   # a pre-extracted feature: no dx
    assert sorted(t.numel() for t in y.grad_fn.saved_tensors) == [36, 36, 144, 33 * 36]
    y.backward(dE)
    net.bn1.weight.requires_grad_(False)
    net.plane(x.clone().requires_grad_(True), heads=4)[0].backward(dE)
    assert calls == [dict(want_dx=False, want_dgamma=True, want_dbeta=True), dict(want_dx=True, want_dgamma=False, want_dbeta=True)]


def test_eval_after_a_training_step_sees_the_new_statistics():
    from laff_amd.model.model import _materialise
    C, H, N = 36, 4, 33
    net = _net(C, H, 23).to(DEV)
    x = (2.0 * torch.randn(N, C) + 0.5).to(DEV)
    net.eval()
    with torch.no_grad():
        before = _materialise(net.plane(x, heads=H), H, H * C).clone()             # fills bn_affine's cache with the initial statistics
    net.train()
    net.plane(x, heads=H)
    net.eval()
    with torch.no_grad():
        after = _materialise(net.plane(x, heads=H), H, H * C)
    norm = torch.nn.BatchNorm1d(H * C).double().eval()
    norm.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.cpu() for k, v in net.bn1.state_dict().items()})
    with torch.no_grad():
        want = norm(x.cpu().double().repeat(1, H))
    assert fc_bwd_ref.rel_err(before.cpu(), want) > 1e-3
    err = fc_bwd_ref.rel_err(after.cpu(), want)
    print('eval after a training step: %.3e' % err)
    assert err <= TR.TOL_UNIT
