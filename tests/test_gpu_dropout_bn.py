"""laff_dropout_bn_train, its backward, the two ops and TransformNet(device_norm=True) on the MI355X.

Rule (tests/train_ref.py): per tensor, max |device - float64| / max |float64| <= max(4 e32, TOL_UNIT).  The reference is
the float64 restatement of tests/dropout_bn_ref.py on the very fp32 inputs handed to the device and the exact mask, recomputed on the
host from the seed; e32 is the same error of the same graph in float32 CPU torch (a * mask * scale -> BatchNorm1d in training mode ->
backward; save_mean / save_invstd: what torch.native_batch_norm saves from that forward) with the same mask.  The backward's reference
reads the fp32 save_mean / save_invstd that the backward is given.  The mask itself is compared exactly.
"""
import functools

import numpy as np
import pytest
import torch

import dropout_bn_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
TOL_UNIT = TR.TOL_UNIT
EPS = 1e-5
SEEDS = (0x0123456789abcdef, 11, 12345678901234567)
ROWS = 256                                                 # rows of a chunk (asserted against the plan below)
SHAPES = [(2, 1), (3, 5), (33, 132), (130, 36), (257, 260), (128, 512), (64, 4096),
          (ROWS + 1, 40),                                  # the smallest N the plan cuts, beside (257, 260): a last chunk of one row
          (600, 12)]                                       # three chunks
MODES = [('bn', 0.0), ('bn', 0.2), ('drop', 0.5)]
LAYOUTS = ('dense', 'pitch4', 'pitch3', 'offset')
# the seeds and shapes whose host masks were looked at beforehand (within 2.1 standard deviations, no constant column)
FIXED_SEED = {(33, 132, 0.2): SEEDS[0], (130, 36, 0.2): SEEDS[1], (257, 260, 0.5): SEEDS[2]}


def _id(c):
    return 'N%d-D%d-%s-p%g' % (c[0], c[1], c[2], c[3])


CASES = [(N, D, kind, p) for (N, D) in SHAPES for (kind, p) in MODES]


def _seed(c):
    N, D, kind, p = c
    return FIXED_SEED.get((N, D, p), SEEDS[(N + D) % 3])


def _momentum(c):
    return 0.1 if (c[0] + c[1]) % 2 else 0.5


def _place(frames, t, layout):
    """A device copy of the 2-D CPU tensor t in `layout` inside a NaN frame; the pitch's slack is part of the frame's inside and is
    checked separately (_slack_intact)."""
    rows, cols = t.shape
    ld, off = TR.pitch(cols, layout)
    flat = frames.floats(rows * ld + 4)
    flat.fill_(NAN)
    view = torch.as_strided(flat, (rows, cols), (ld, 1), flat.storage_offset() + off)
    view.copy_(t)
    assert (view.data_ptr() % 16 == 4) == (layout == 'offset')
    return flat, view


def _vec(frames, t, layout):
    """A [D] vector inside a NaN frame; 'offset' puts its base 4 bytes past a 16-byte boundary."""
    n = t.numel()
    flat = frames.floats(n + 4)
    flat.fill_(NAN)
    lo = 1 if layout == 'offset' else 0
    view = flat[lo:lo + n]
    view.copy_(t)
    return flat, view


def _slack_intact(held):
    """Whether every float of each framed buffer outside its (strided) view is NaN still."""
    for flat, view in held:
        chk = flat.clone()
        torch.as_strided(chk, view.shape, view.stride(), view.storage_offset() - flat.storage_offset()).fill_(NAN)
        if not chk.isnan().all():
            return False
    return True


@functools.lru_cache(maxsize=None)
def _case(c):
    """The fp32 operands of a case on the CPU, the exact mask, the float64 reference and e32 per tensor -- computed once, shared, never
    written."""
    N, D, kind, p = c
    bn = kind == 'bn'
    g = torch.Generator().manual_seed(N * 1000003 + D * 1009 + int(p * 10))
    a = torch.randn(N, D, generator=g)
    a[a == 0] = 1.0
    dy = torch.randn(N, D, generator=g)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    rm, rv = torch.randn(D, generator=g), torch.rand(D, generator=g) + 0.5
    cols = {}
    if bn and D >= 5:
        cols = dict(offset=1, dead=2, negative=3, zero=4)
        a[:, 1] = 30.0 + 0.01 * torch.randn(N, generator=g)          # mean 30, standard deviation 0.01: an E[u^2] - mean^2 kernel fails here
        a[:, 2] = 0.0                                                 # a dead ReLU unit
        gamma[3], gamma[4] = -abs(gamma[3]) - 0.1, 0.0
    seed, momentum = _seed(c), _momentum(c)
    keep = R.keep_mask(seed, N, D, p)
    f = R.forward(a, keep, p, gamma if bn else None, beta, rm, rv, momentum, EPS)
    ref = dict(y=f['y'])
    mean32 = invstd32 = None
    if bn:
        mean32, invstd32 = torch.from_numpy(f['mean']).float(), torch.from_numpy(f['invstd']).float()
        ref.update(save_mean=f['mean'], save_invstd=f['invstd'], running_mean=f['running_mean'], running_var=f['running_var'])
    da, dgamma, dbeta = R.backward(dy, a, keep, p, gamma if bn else None, mean32, invstd32)
    ref.update(da=da)
    if bn:
        ref.update(dgamma=dgamma, dbeta=dbeta)
    # e32: the same graph in float32 CPU torch with the same mask
    at = a.clone().requires_grad_(True)
    u32 = at * torch.from_numpy(keep) * float(R.scale32(p)) if p else at * 1.0
    e32 = {}
    if bn:
        norm = torch.nn.BatchNorm1d(D, eps=EPS, momentum=momentum).train()
        with torch.no_grad():
            norm.weight.copy_(gamma)
            norm.bias.copy_(beta)
            norm.running_mean.copy_(rm)
            norm.running_var.copy_(rv)
        # the statistics torch saves for its backward, from the same float32 forward (its running statistics go to copies)
        _, mean_t, invstd_t = torch.native_batch_norm(u32.detach(), gamma, beta, rm.clone(), rv.clone(), True, momentum, EPS)
        y32 = norm(u32)
        y32.backward(dy)
        got32 = dict(y=y32, da=at.grad, dgamma=norm.weight.grad, dbeta=norm.bias.grad, running_mean=norm.running_mean, running_var=norm.running_var,
                     save_mean=mean_t, save_invstd=invstd_t)
    else:
        u32.backward(dy)
        got32 = dict(y=u32, da=at.grad)
    # the backward's reference reads the fp32 statistics it is handed; e32 of the gradients is the float32 graph against the float64 one
    # with float64 statistics, its own error included
    full = R.backward(dy, a, keep, p, gamma if bn else None, f.get('mean'), f.get('invstd'))
    ref64 = dict(ref, da=full[0], dgamma=full[1], dbeta=full[2])
    for k, t in got32.items():
        e32[k] = R.rel_err(t, ref64[k])
    return dict(c=c, a=a, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, keep=keep, seed=seed, momentum=momentum, mean32=mean32,
                invstd32=invstd32, ref=ref, e32=e32, cols=cols, bn=bn)


def _bound(cs, name):
    return max(4.0 * cs['e32'].get(name, 0.0), TOL_UNIT)


def _seed_tensor(seed):
    return torch.tensor([seed], dtype=torch.int64, device=DEV)


def _run(c, layout, want=(True, True, True), seed=None):
    """Forward and backward through the ops with every operand and output inside NaN frames of the case's layout.  Returns the outputs
    by name (absent backward outputs: None) after the frames were checked."""
    from laff_amd import ops
    cs = _case(c)
    N, D, kind, p = c
    bn = cs['bn']
    fr = TR.Frames(16)
    held = []

    def mat(t):
        held.append(_place(fr, t, layout))
        return held[-1][1]

    def vec(t):
        held.append(_vec(fr, t, layout))
        return held[-1][1]
    a, dy = mat(cs['a']), mat(cs['dy'])
    y, da = mat(torch.full((N, D), NAN)), (mat(torch.full((N, D), NAN)) if want[0] else None)
    sd = _seed_tensor(cs['seed'] if seed is None else seed) if p else None
    out = {}
    if bn:
        gamma, beta, rm, rv = vec(cs['gamma']), vec(cs['beta']), vec(cs['rm']), vec(cs['rv'])
        sm, si = vec(torch.full((D,), NAN)), vec(torch.full((D,), NAN))
        res = ops.dropout_bn_train(a, p, sd, gamma, beta, rm, rv, cs['momentum'], EPS, out=(y, sm, si))
        assert res[0].data_ptr() == y.data_ptr() and res[1].data_ptr() == sm.data_ptr() and res[2].data_ptr() == si.data_ptr()
        out.update(y=y, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv)
        # the backward is handed the reference's statistics rounded to fp32: its check does not inherit the forward's error
        mean_in, inv_in = vec(cs['mean32']), vec(cs['invstd32'])
        dg, db = (vec(torch.full((D,), NAN)) if want[1] else None), (vec(torch.full((D,), NAN)) if want[2] else None)
        res = ops.dropout_bn_train_backward(dy, a, p, sd, gamma, mean_in, inv_in, *want, out=(da, dg, db))
        out.update(da=res[0], dgamma=res[1], dbeta=res[2])
        assert all((r is None) == (not w) for r, w in zip(res, want))
    else:
        res = ops.dropout_bn_train(a, p, sd, None, None, None, None, 0.1, EPS, out=y)
        assert res[0].data_ptr() == y.data_ptr() and res[1] is None and res[2] is None
        out.update(y=y)
        res = ops.dropout_bn_train_backward(dy, a, p, sd, None, None, None, want[0], False, False, out=(da, None, None))
        out.update(da=res[0])
    torch.cuda.synchronize()
    assert fr.intact(), 'a write outside a buffer'
    assert _slack_intact(held), 'a write into the slack of a pitch'
    for k, t in out.items():
        assert t is None or not t.isnan().any(), '%s: an element was not written (or read a NaN)' % k
    assert torch.equal(a.cpu(), cs['a']) and torch.equal(dy.cpu(), cs['dy'])
    return {k: (None if t is None else t.detach().cpu().clone()) for k, t in out.items()}


def _check(c, layout, got):
    cs = _case(c)
    for k, ref in cs['ref'].items():
        if got.get(k) is None:
            continue
        err, bound = R.rel_err(got[k], ref), _bound(cs, k)
        print('%s %-6s %-12s err %.3e  fp32 CPU %.3e  bound %.3e' % (_id(c), layout, k, err, cs['e32'].get(k, 0.0), bound))
        assert err <= bound, (k, layout, err, bound)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_kernels_vs_float64(c):
    from laff_amd import ops
    assert ops.dropout_bn_train_plan(ROWS, 8)[0] == 1 and ops.dropout_bn_train_plan(ROWS + 1, 8)[0] == 2
    cs = _case(c)
    N, D, kind, p = c
    keep, first = cs['keep'], None
    if p and N * D >= 1000:
        kept = float(keep.mean())
        sd = ((1.0 - p) * p / keep.size) ** 0.5
        print('%s kept %.4f, %.2f standard deviations from %.2f' % (_id(c), kept, abs(kept - (1.0 - p)) / sd, 1.0 - p))
        assert abs(kept - (1.0 - p)) <= 5.0 * sd
    for layout in LAYOUTS:
        got = _run(c, layout)
        _check(c, layout, got)
        a = cs['a'].numpy()
        if kind == 'drop':
            # the mask itself, exactly: inputs without zeros, so y == 0 where the host mask drops and nowhere else; a kept element is
            # a * fp32(1 / (1 - p)) bit for bit; da likewise from dy
            y, da = got['y'].numpy(), got['da'].numpy()
            assert np.array_equal(y == 0, ~keep), 'the device mask is not the host mask'
            assert np.array_equal(y[keep], (a * R.scale32(p))[keep])
            assert np.array_equal(da == 0, ~keep | (cs['dy'].numpy() == 0)) and np.array_equal(da[keep], (cs['dy'].numpy() * R.scale32(p))[keep])
        elif p:
            # through the BatchNorm stage the mask shows in da: exactly zero where dropped
            assert (got['da'].numpy()[~keep] == 0).all()
        if cs['cols']:
            dead, zero = cs['cols']['dead'], cs['cols']['zero']
            # var == 0: invstd = 1 / sqrt(eps), y == beta exactly, and dgamma == 0 exactly (xhat is exactly zero); da there is
            # gamma invstd (dy - mean dy) where kept -- checked against float64 above, and it is NOT zero
            assert np.array_equal(got['y'].numpy()[:, dead], np.broadcast_to(cs['beta'].numpy()[dead], (N,)))
            assert got['save_mean'][dead] == 0 and got['save_invstd'][dead] == np.float32(1.0 / np.sqrt(EPS))
            assert got['dgamma'][dead] == 0
            # gamma == 0: nothing flows back, exactly
            assert (got['da'].numpy()[:, zero] == 0).all()
        if first is None:
            first = got
        else:
            for k, t in got.items():                      # the layout changes the kernel (16-byte or element-wise), not a bit
                assert torch.equal(t, first[k]), '%s differs between the layouts dense and %s' % (k, layout)


@pytest.mark.parametrize('c', [CASES[3 * 2 + 1], CASES[3 * 3 + 1], CASES[3 * 4 + 1], CASES[3 * 7]], ids=_id)
def test_each_output_absent_in_turn(c):
    full = _run(c, 'pitch4')
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        got = _run(c, 'pitch4', want)
        for i, k in enumerate(('da', 'dgamma', 'dbeta')):
            assert (got[k] is None) == (i == skip)
            if got[k] is not None:
                assert torch.equal(got[k], full[k]), '%s changes when output %d is absent' % (k, skip)
    only = _run(c, 'pitch4', (False, False, True))
    assert only['da'] is None and only['dgamma'] is None and torch.equal(only['dbeta'], full['dbeta'])
    none = _run(c, 'pitch4', (False, False, False))
    assert none['da'] is None and none['dgamma'] is None and none['dbeta'] is None


@pytest.mark.parametrize('c', [CASES[3 * 2 + 1], CASES[3 * 4 + 1], CASES[3 * 4 + 2], CASES[3 * 5 + 1]], ids=_id)
def test_one_seed_the_same_bits_two_seeds_two_masks(c):
    first, again = _run(c, 'dense'), _run(c, 'dense')
    assert all(torch.equal(first[k], again[k]) for k in first)
    other = _run(c, 'dense', seed=_case(c)['seed'] + 1)
    N, D, kind, p = c
    host = R.keep_mask(_case(c)['seed'] + 1, N, D, p)
    assert not np.array_equal(host, _case(c)['keep'])
    if kind == 'drop':
        assert np.array_equal(other['y'].numpy() == 0, ~host)
    else:
        assert (other['da'].numpy()[~host] == 0).all() and not torch.equal(other['y'], first['y'])


def test_empty_batch_without_statistics_touches_nothing():
    from laff_amd import ops
    res = ops.dropout_bn_train(torch.empty(0, 7, device=DEV), 0.5, _seed_tensor(3), None, None, None, None, 0.1, EPS)
    assert tuple(res[0].shape) == (0, 7) and res[1] is None
    da = ops.dropout_bn_train_backward(torch.empty(0, 7, device=DEV), torch.empty(0, 7, device=DEV), 0.5, _seed_tensor(3), None, None, None,
                                       True, False, False)[0]
    assert tuple(da.shape) == (0, 7)
    v = torch.ones(7, device=DEV)
    with pytest.raises(RuntimeError, match='N >= 2'):
        ops.dropout_bn_train(torch.ones(1, 7, device=DEV), 0.0, None, v, v, v.clone(), v.clone(), 0.1, EPS)
    with pytest.raises(TypeError):
        ops.dropout_bn_train(torch.ones(4, 7, device=DEV).double(), 0.0, None, v, v, v.clone(), v.clone(), 0.1, EPS)
    with pytest.raises(TypeError):
        ops.dropout_bn_train_backward(torch.ones(4, 7, device=DEV), torch.ones(4, 7, device=DEV).half(), 0.0, None, v, v, v)


def test_graph_capture_replays_the_eager_bits():
    from laff_amd import ops
    c = (257, 260, 'bn', 0.2)                              # cut in two: two launches each way, partials in the workspace
    cs = _case(c)
    N, D = c[:2]
    a, dy = cs['a'].to(DEV), cs['dy'].to(DEV)
    gamma, beta = cs['gamma'].to(DEV), cs['beta'].to(DEV)
    sd = _seed_tensor(cs['seed'])

    def step(rm, rv, outs):
        y, sm, si = ops.dropout_bn_train(a, 0.2, sd, gamma, beta, rm, rv, cs['momentum'], EPS, out=outs[:3])
        ops.dropout_bn_train_backward(dy, a, 0.2, sd, gamma, sm, si, out=outs[3:])

    def buffers():
        return [torch.full((N, D), NAN, device=DEV), torch.full((D,), NAN, device=DEV), torch.full((D,), NAN, device=DEV),
                torch.full((N, D), NAN, device=DEV), torch.full((D,), NAN, device=DEV), torch.full((D,), NAN, device=DEV)]
    eager, rm_e, rv_e = buffers(), cs['rm'].to(DEV), cs['rv'].to(DEV)
    step(rm_e, rv_e, eager)
    outs, rm_g, rv_g = buffers(), cs['rm'].to(DEV), cs['rv'].to(DEV)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        step(rm_g, rv_g, outs)
    assert torch.equal(rm_g.cpu(), cs['rm'])               # capturing runs nothing
    gr.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(outs + [rm_g, rv_g], eager + [rm_e, rv_e]))
    _check(c, 'graph', dict(y=outs[0].cpu(), save_mean=outs[1].cpu(), save_invstd=outs[2].cpu(), running_mean=rm_g.cpu(), running_var=rv_g.cpu()))
    # a new seed in the same word: the replay reads it
    sd.fill_(cs['seed'] + 1)
    gr.replay()
    torch.cuda.synchronize()
    assert (outs[3].cpu().numpy()[~R.keep_mask(cs['seed'] + 1, N, D, 0.2)] == 0).all() and not torch.equal(outs[0], eager[0])


# ---- TransformNet(device_norm=True) -------------------------------------------------------------------------------------------------
class _SeedSpy:
    """Wraps ops.dropout_bn_train: keeps the seed tensors the module handed to it."""

    def __init__(self, monkeypatch):
        from laff_amd import ops
        self.seeds, self.calls = [], 0
        real = ops.dropout_bn_train

        def spy(a, p, seed, *args, **kw):
            self.calls += 1
            self.seeds.append(None if seed is None else seed.clone())
            return real(a, p, seed, *args, **kw)
        monkeypatch.setattr(ops, 'dropout_bn_train', spy)

    def last(self):
        return None if self.seeds[-1] is None else int(self.seeds[-1].item())


CONFIGS = [(True, 'tanh', 0.0), (True, 'relu', 0.0), (False, 'sigmoid', 0.0), (False, None, 0.0), (False, 'tanh', 0.2), (True, 'tanh', 0.2)]


@pytest.mark.parametrize('batch_norm, activation, dropout', CONFIGS, ids=lambda v: str(v))
def test_transform_net_device_norm(batch_norm, activation, dropout, monkeypatch):
    from laff_amd.model.model import TransformNet
    torch.manual_seed(11)
    N = 33
    net = TransformNet((68, 132), batch_norm=batch_norm, activation=activation, dropout=dropout, device_norm=True)
    with torch.no_grad():
        net.fc1.bias.normal_(0.0, 0.1)
    W, b = net.fc1.weight.detach().clone(), net.fc1.bias.detach().clone()
    x, dE = torch.randn(N, 68), torch.randn(N, 132)
    net = net.to(DEV).train()
    spy = _SeedSpy(monkeypatch)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    assert y.requires_grad and tuple(y.shape) == (N, 132)
    assert spy.calls == (1 if batch_norm or dropout else 0)             # neither stage: nothing to launch
    y.backward(dE.to(DEV))
    keep = None
    if dropout:
        keep = R.keep_mask(spy.last(), N, 132, dropout)                 # from the seed, not off the output
        kept = float(keep.mean())
        assert abs(kept - (1.0 - dropout)) <= 5.0 * ((1.0 - dropout) * dropout / keep.size) ** 0.5, kept
        if not batch_norm:
            assert np.array_equal(y.detach().cpu().numpy() == 0, ~keep)
    ref = TR.layer_graph(torch.float64, W, b, x, dE, activation, batch_norm, keep, dropout)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, activation, batch_norm, keep, dropout)
    got = {'y': y, 'x.grad': xd.grad, 'fc1.weight.grad': net.fc1.weight.grad, 'fc1.bias.grad': net.fc1.bias.grad}
    if batch_norm:
        got.update({'bn1.weight.grad': net.bn1.weight.grad, 'bn1.bias.grad': net.bn1.bias.grad, 'running_mean': net.bn1.running_mean,
                    'running_var': net.bn1.running_var})
        assert int(net.bn1.num_batches_tracked) == 1
    TR.compare(got, ref, f32)
    # plane(): the same route, plain and dense; `pending` is not used
    pending = []
    src, tile, scale, shift = net.plane(xd.detach(), heads=2, pending=pending)
    assert pending == [] and tile is False and scale is None and shift is None and src.requires_grad
    assert spy.calls == (2 if batch_norm or dropout else 0)


def test_only_the_wanted_gradients_are_formed(monkeypatch):
    from laff_amd import ops
    from laff_amd.model.model import TransformNet
    torch.manual_seed(12)
    net = TransformNet((68, 132), batch_norm=True, activation='tanh', dropout=0.2, device_norm=True).to(DEV).train()
    x, dE = torch.randn(33, 68, device=DEV), torch.randn(33, 132, device=DEV)
    calls, saved = [], []
    real = ops.dropout_bn_train_backward

    def spy(*args, **kw):
        calls.append({k: kw[k] for k in ('want_da', 'want_dgamma', 'want_dbeta')})
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'dropout_bn_train_backward', spy)
    y = net(x)
    # what stays alive between forward and backward: a (which _FcActFn holds anyway), weight, the seed and two [D] vectors -- no mask, no U
    held = [t for t in y.grad_fn.saved_tensors if t is not None]
    assert sorted(t.numel() for t in held) == [1, 132, 132, 132, 33 * 132]
    a_saved = [t for t in held if t.numel() == 33 * 132][0]
    assert a_saved.data_ptr() == y.grad_fn.next_functions[0][0].saved_tensors[2].data_ptr()
    y.backward(dE)
    net.bn1.weight.requires_grad_(False)
    net(x).backward(dE)
    assert calls == [dict(want_da=True, want_dgamma=True, want_dbeta=True), dict(want_da=True, want_dgamma=False, want_dbeta=True)]


def test_concat_train_passes_through_the_same_stage(monkeypatch):
    from laff_amd.model.model import TransformNet
    torch.manual_seed(13)
    N, widths, D = 33, (20, 48), 132
    net = TransformNet((sum(widths), D), batch_norm=True, activation='tanh', dropout=0.2, device_norm=True)
    W, b = net.fc1.weight.detach().clone(), net.fc1.bias.detach().clone()
    dense = torch.randn(N, widths[0])
    counts = (torch.rand(N, widths[1]) < 0.1).float() * torch.randint(1, 3, (N, widths[1])).float()
    dE = torch.randn(N, D)
    net = net.to(DEV).train()
    spy = _SeedSpy(monkeypatch)
    xd = dense.to(DEV).requires_grad_(True)
    y = net.concat_train([xd, counts.to_sparse_csr().to(DEV)])
    y.backward(dE.to(DEV))
    assert spy.calls == 1 and int(net.bn1.num_batches_tracked) == 1
    keep = R.keep_mask(spy.last(), N, D, 0.2)
    x = torch.cat([dense, counts], dim=1)
    ref = TR.layer_graph(torch.float64, W, b, x, dE, 'tanh', True, keep, 0.2)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, 'tanh', True, keep, 0.2)
    got = {'y': y, 'fc1.weight.grad': net.fc1.weight.grad, 'fc1.bias.grad': net.fc1.bias.grad, 'bn1.weight.grad': net.bn1.weight.grad,
           'bn1.bias.grad': net.bn1.bias.grad, 'running_mean': net.bn1.running_mean, 'running_var': net.bn1.running_var}
    TR.compare(got, ref, f32)
    err = R.rel_err(xd.grad.cpu(), ref['x.grad'][:, :widths[0]])
    assert err <= max(4.0 * R.rel_err(f32['x.grad'][:, :widths[0]], ref['x.grad'][:, :widths[0]]), TOL_UNIT)


def test_eval_after_a_training_step_sees_the_new_statistics():
    from laff_amd.model.model import TransformNet
    torch.manual_seed(14)
    N = 33
    net = TransformNet((68, 132), batch_norm=True, activation='tanh', dropout=0.0, device_norm=True).to(DEV)
    x = (2.0 * torch.randn(N, 68) + 0.5).to(DEV)
    net.eval()
    with torch.no_grad():
        before = net(x).clone()                            # fills bn_affine's cache with the initial statistics
    net.train()
    net(x)
    net.eval()
    with torch.no_grad():
        after = net(x)
    lin = torch.nn.Linear(68, 132).double()
    norm = torch.nn.BatchNorm1d(132).double().eval()
    with torch.no_grad():
        lin.weight.copy_(net.fc1.weight)
        lin.bias.copy_(net.fc1.bias)
        norm.running_mean.copy_(net.bn1.running_mean)
        norm.running_var.copy_(net.bn1.running_var)
        want = norm(torch.tanh(lin(x.cpu().double())))
    assert not torch.allclose(net.bn1.running_var.cpu(), torch.ones(132)) and R.rel_err(before.cpu(), want) > 1e-3
    err = R.rel_err(after.cpu(), want)
    print('eval after a training step: %.3e' % err)
    assert err <= TOL_UNIT


@pytest.mark.parametrize('batch_norm, dropout', [(True, 0.2), (False, 0.2), (True, 0.0)], ids=str)
def test_default_route_is_torchs_own_bit_for_bit(batch_norm, dropout):
    import torch.nn.functional as F
    from laff_amd.model.model import TransformNet, _FcActFn
    torch.manual_seed(15)
    net = TransformNet((68, 132), batch_norm=batch_norm, activation='tanh', dropout=dropout).to(DEV).train()
    assert net.device_norm is False
    x, dE = torch.randn(33, 68, device=DEV), torch.randn(33, 132, device=DEV)
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def straight(xg):
        a = _FcActFn.apply(xg, net.fc1.weight, net.fc1.bias, 'tanh')
        if dropout:
            a = F.dropout(a, dropout, training=True)
        return net.bn1(a) if batch_norm else a

    def run(route):
        net.load_state_dict(state)
        net.zero_grad()
        torch.manual_seed(99)
        xg = x.clone().requires_grad_(True)
        y = route(xg)
        y.backward(dE)
        return [y.detach().clone(), xg.grad.clone()] + [q.grad.clone() for q in net.parameters()] + [q.clone() for q in net.buffers()]
    got, want = run(net), run(straight)
    assert len(got) == len(want) == 2 + (4 + 3 if batch_norm else 2)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_captured_module_step_draws_a_new_mask_on_every_replay():
    from laff_amd.model.model import TransformNet
    torch.manual_seed(16)
    N = 33
    net = TransformNet((68, 132), batch_norm=False, activation='tanh', dropout=0.2, device_norm=True).to(DEV).train()
    x, dE = torch.randn(N, 68, device=DEV).requires_grad_(True), torch.randn(N, 132, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                 # warm up outside the capture, as torch's whole-network capture does
            net.zero_grad(set_to_none=True)
            x.grad = None
            net(x).backward(dE)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    net.zero_grad(set_to_none=True)
    x.grad = None
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        y = net(x)
        y.backward(dE)
    masks, grads = [], []
    for _ in range(2):
        gr.replay()
        torch.cuda.synchronize()
        masks.append((y.detach() != 0).cpu().numpy())
        grads.append(x.grad.detach().cpu().clone())
    assert not np.array_equal(masks[0], masks[1]) and not torch.equal(grads[0], grads[1])
    for m in masks:
        assert abs(float(m.mean()) - 0.8) <= 5.0 * (0.8 * 0.2 / m.size) ** 0.5
