"""laff_grad_sqnorm / laff_grad_scale / laff_optim_step, laff_amd.optim and one whole training step on the MI355X.

Kernel level.  The reference is the float64 evaluation of the formulas of tests/optim_ref.py on the very fp32 p, g, m, v handed to the
device.  The bounds are derived there (one fp32 rounding per operation of the kernel's sequence, 2 u for the clip coefficient) and hold
element by element, u = 2^-24, G = |c g| + |wd p|:

    total_norm   |out - ref| <= 2^-23 ref
    m'           <= 10 u (|m| + (1 - beta1) G)
    v', s'       <= 14 u (beta v + (1 - beta) G^2)
    p'           <= u |ref| + 13 u |Delta|     against float64 evaluated FROM THE DEVICE'S OWN m', v' (s'), so each stage is held on its own
    c g          <= 3 u |c g|                   (clip_grad_norm_)

Every buffer sits in a NaN-filled frame that has to stay NaN, g has to keep its bits through the fused step, and the launches a call
issued are compared with the plan: the 16-byte variant for aligned lists, the single-float variant as soon as one base is 4 bytes past
a 16-byte boundary.

Module level: max |device - float64| / max |float64| within the larger of 4 x the same error of torch's own fp32 CPU run and 1.5e-6
(the rule of tests/test_gpu_fuse_backward.py).  Each case prints the largest fraction of its bounds that it used.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import optim_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
U = R.U
TOL_UNIT = TR.TOL_UNIT
MIXED = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
ROLES = ('p', 'g', 's1', 's2')


@functools.lru_cache(maxsize=None)
def _plan():
    from laff_amd import ops
    chunk, capacity, _, _, _, cap = ops.optim_plan([])
    return chunk, capacity, cap


def _sizes(name):
    chunk, capacity, cap = _plan()
    return {'n1': [1], 'n3': [3], 'n4': [4], 'n5': [5], 'mixed': MIXED, 'chunks': [chunk - 1, chunk, chunk + 1, 3 * chunk + 5],
            'many': [1 + i % 7 for i in range(capacity + 3)], 'stride': [cap * chunk + 3], 'empty': [5, 0, 64]}[name]


@functools.lru_cache(maxsize=None)
def _values(name, with_state):
    """fp32 p, g, m, v of a list on the CPU -- computed once, shared, never written.  g spreads over 1e-4 .. 1 with exact zeros; every
    7th element has g = m = v = 0 (p must keep its bits there without weight decay); with_state: moments as a previous step leaves them."""
    rng = np.random.default_rng(len(name) * 1009 + sum(_sizes(name)) % 1000003 + int(with_state))
    out = {k: [] for k in ROLES}
    for n in _sizes(name):
        p = rng.standard_normal(n).astype(np.float32)
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4.0, 0.0, n)).astype(np.float32)
        g[rng.random(n) < 0.1] = 0.0
        m = (0.1 * rng.standard_normal(n)).astype(np.float32) if with_state else np.zeros(n, np.float32)
        v = ((0.1 * rng.standard_normal(n)) ** 2).astype(np.float32) if with_state else np.zeros(n, np.float32)
        quiet = np.arange(n) % 7 == 3
        g[quiet] = 0.0
        m[quiet] = 0.0
        v[quiet] = 0.0
        for k, a in zip(ROLES, (p, g, m, v)):
            a.setflags(write=False)
            out[k].append(a)
    return out


def _place(arrays, offset):
    """Device copies, each in its own NaN frame, 16-byte aligned or (offset) 4 bytes past a 16-byte boundary: (buffers, views)."""
    bufs, views = [], []
    for a in arrays:
        buf = torch.full((a.size + 12,), NAN, device=DEV)
        lo = 5 if offset else 4
        view = buf[lo:lo + a.size]
        view.copy_(torch.tensor(a))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (4 if offset else 0)
        bufs.append(buf)
        views.append(view)
    return bufs, views


def _frames_intact(bufs, views):
    for buf, view in zip(bufs, views):
        chk = buf.clone()
        chk[view.storage_offset() - buf.storage_offset():][:view.numel()].fill_(NAN)
        if not bool(chk.isnan().all()):
            return False
    return True


def _launch(kind, name, with_state, hyper, clip, offset_role=None, values=None):
    """One fused step on the device.  clip: 'half' / 'twice' the norm, or None.  Returns the outputs as numpy arrays by role, the
    device's total norm (None without clipping), the max_norm used and the (16-byte, single-float) launches of the update."""
    from laff_amd import ops
    vals = values or _values(name, with_state)
    roles = ROLES if kind == 'adam' else ROLES[:3]
    # RMSprop's square_avg is the (non-negative) second moment of the values
    placed = {k: _place(vals['s2' if (kind, k) == ('rmsprop', 's1') else k], offset_role == k) for k in roles}
    views = {k: placed[k][1] for k in roles}
    norm = R.total_norm(vals['g'])
    max_norm = {None: 0.0, 'half': 0.5 * norm, 'twice': 2.0 * norm}[clip]
    ws, partials, total = None, 0, None
    g_before = [t.clone() for t in views['g']]
    if clip:
        ws_buf = torch.full((8 * ops.optim_plan(_sizes(name))[3] // 4 + 8,), NAN, device=DEV)        # fp32 words around the partials
        ws = ws_buf[4:-4].view(torch.uint8)
        ws, partials = ops.grad_sqnorm(views['g'], ws)
        assert ops.optim_last_launches() == ((0, ops.optim_plan(_sizes(name))[2]) if offset_role == 'g' else
                                             (ops.optim_plan(_sizes(name))[2], 0))
        total = torch.full((3,), NAN, device=DEV)
    ops.optim_step(kind, views['p'], views['g'], views['s1'], views['s2'] if kind == 'adam' else None, max_norm=max_norm, workspace=ws,
                   partials=partials, total_norm_out=total[1] if clip else None, **hyper)
    launches = ops.optim_last_launches()
    torch.cuda.synchronize()
    for k in roles:
        assert _frames_intact(*placed[k]), 'the frame around %s was written' % k
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g_before, views['g'])), 'g was written'
    if clip:
        assert bool(ws_buf[:4].isnan().all()) and bool(ws_buf[-4:].isnan().all()) and bool(total[0].isnan()) and bool(total[2].isnan())
    out = {k: [t.cpu().numpy() for t in views[k]] for k in roles}
    return out, (float(total[1]) if clip else None), max_norm, launches


def _fraction(key, got, ref, bound):
    """max |got - ref| / bound over a list; where the bound is zero the values must be equal."""
    worst = 0.0
    for a, r, b in zip(got, ref, bound):
        err = np.abs(a.astype(np.float64) - r)
        assert np.all(err[b == 0] == 0), key
        if np.any(b > 0):
            worst = max(worst, float(np.max(err[b > 0] / b[b > 0])))
    return worst


def _check(kind, name, with_state, hyper, out, total, max_norm, label):
    vals = _values(name, with_state)
    p, g, m, v = (vals[k] for k in ROLES)
    norm = R.total_norm(g)
    if max_norm > 0:
        assert abs(total - norm) <= 2.0 ** -23 * norm, (total, norm)
    c = R.clip_coef(norm, max_norm)
    wd, lr, eps = hyper.get('weight_decay', 0.0), hyper['lr'], hyper['eps']
    G = R.gmag(p, g, c, wd)
    used = {}
    if kind == 'adam':
        b1, b2, step = hyper['beta1'], hyper['beta2'], hyper['step']
        _, m_ref, v_ref = R.adam(p, g, m, v, lr, b1, b2, eps, wd, step, c)
        used['m'] = _fraction('m', out['s1'], m_ref, R.bound_m(m, G, b1))
        used['v'] = _fraction('v', out['s2'], v_ref, R.bound_v(v, G, b2))
        p_ref = R.adam_param(p, out['s1'], out['s2'], lr, b1, b2, eps, step)
        used['p'] = _fraction('p adam', out['p'], p_ref, R.bound_p_adam(p_ref, out['s1'], out['s2'], lr, b1, b2, eps, step))
    else:
        alpha = hyper['beta2']
        _, s_ref = R.rmsprop(p, g, v, lr, alpha, eps, wd, c)
        used['s'] = _fraction('s', out['s1'], s_ref, R.bound_v(v, G, alpha))
        gh = R.clipped(g, c, p, wd)
        p_ref = R.rmsprop_param(p, gh, out['s1'], lr, eps)
        used['p'] = _fraction('p rmsprop', out['p'], p_ref, R.bound_p_rmsprop(p_ref, G, out['s1'], lr, eps))
    print('%-60s %s' % (label, '  '.join('%s %.3f' % kv for kv in used.items())))
    assert all(f <= 1.0 for f in used.values()), (label, used)
    if wd == 0.0:                                        # g = m = v = 0: the parameter keeps its bits
        for a, b in zip(out['p'], p):
            quiet = np.arange(a.size) % 7 == 3
            assert np.array_equal(a[quiet].view(np.int32), b[quiet].view(np.int32))


def _hyper(kind, eps=None, wd=0.0, step=1):
    if kind == 'adam':
        return dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-4 if eps is None else eps, weight_decay=wd, step=step)
    return dict(lr=1e-2, beta2=0.99, eps=1e-8 if eps is None else eps, weight_decay=wd, step=step)


# (list, kind, eps, wd, step, state from a previous step, clip)
# every size list with both kinds, each fresh (step 1, zero moments, no decay) and continuing (step 7, moments, decay); the mixed list
# with the whole cross, moments of a previous step at step 1 (the smallest bias corrections, the largest step) and zero ones at 7 included
CASES = [(name, kind, None, wd, step, state, 'half')
         for name in ('n1', 'n3', 'n4', 'n5', 'chunks', 'many', 'stride', 'empty')
         for kind in ('adam', 'rmsprop') for wd, step, state in ((0.0, 1, False), (0.01, 7, True))]
CASES += [('mixed', kind, None, wd, step, state, clip)
          for kind in ('adam', 'rmsprop') for wd in (0.0, 0.01) for step, state in ((1, False), (7, True), (1, True), (7, False))
          for clip in ('half', 'twice', None)]
CASES += [('mixed', 'adam', 1e-8, 0.0, 7, True, 'half'), ('mixed', 'adam', 1e-8, 0.01, 1, False, None),
          ('chunks', 'adam', 1e-8, 0.01, 7, True, None), ('many', 'adam', None, 0.01, 7, True, 'twice')]


def _id(c):
    return '-'.join(str(x) for x in c)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_step_vs_float64(c):
    from laff_amd import ops
    name, kind, eps, wd, step, state, clip = c
    hyper = _hyper(kind, eps, wd, step)
    out, total, max_norm, launches = _launch(kind, name, state, hyper, clip)
    plan = ops.optim_plan(_sizes(name))
    assert launches == (plan[4], 0)                       # aligned bases: the 16-byte variant, as many launches as planned
    if name == 'many':
        assert plan[2] >= 2 and plan[4] >= 2
    if name == 'stride':
        assert plan[3] == _plan()[2] and sum(_sizes(name)) > _plan()[2] * _plan()[0]                 # more chunks than blocks
    _check(kind, name, state, hyper, out, total, max_norm, _id(c))


@pytest.mark.parametrize('kind, role', [(k, r) for k in ('adam', 'rmsprop') for r in ROLES if not (k == 'rmsprop' and r == 's2')])
def test_single_float_variant_when_a_base_is_4_bytes_off(kind, role):
    from laff_amd import ops
    hyper = _hyper(kind, None, 0.01, 7)
    out, total, max_norm, launches = _launch(kind, 'mixed', True, hyper, 'half', offset_role=role)
    assert launches == (0, ops.optim_plan(MIXED)[4])
    _check(kind, 'mixed', True, hyper, out, total, max_norm, '%s, %s 4 bytes off' % (kind, role))
    aligned = _launch(kind, 'mixed', True, hyper, 'half')[0]                                     # both variants: the same bits
    for k in out:
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(out[k], aligned[k])), k


@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
@pytest.mark.parametrize('name', ['mixed', 'chunks'])
def test_inactive_clip_is_bit_identical_to_none(kind, name):
    hyper = _hyper(kind, None, 0.01, 7)
    loose, total, max_norm, _ = _launch(kind, name, True, hyper, 'twice')
    none = _launch(kind, name, True, hyper, None)[0]
    again = _launch(kind, name, True, hyper, 'twice')[0]                                         # and two calls from equal state
    assert max_norm > R.total_norm(_values(name, True)['g'])
    for k in loose:
        for a, b, c in zip(loose[k], none[k], again[k]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(a.view(np.int32), c.view(np.int32)), k


@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_repeats_are_bit_identical(kind):
    hyper = _hyper(kind, None, 0.01, 7)
    first, t1, _, _ = _launch(kind, 'chunks', True, hyper, 'half')
    second, t2, _, _ = _launch(kind, 'chunks', True, hyper, 'half')
    assert t1 == t2
    for k in first:
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first[k], second[k])), k


def test_grad_is_none_and_empty_tensors_are_skipped():
    from laff_amd import optim
    ps = [torch.nn.Parameter(torch.randn(5, device=DEV)), torch.nn.Parameter(torch.randn(0, device=DEV)),
          torch.nn.Parameter(torch.randn(7, device=DEV)), torch.nn.Parameter(torch.randn(64, device=DEV))]
    before = [p.detach().clone() for p in ps]
    for i in (0, 1, 3):
        ps[i].grad = torch.randn_like(ps[i])
    opt = optim.Adam(ps, lr=1e-2, grad_clip=1.0)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(ps[2], before[2]) and ps[2] not in opt.state
    assert not torch.equal(ps[0], before[0]) and not torch.equal(ps[3], before[3])
    want = float(torch.cat([ps[0].grad, ps[3].grad]).double().norm())
    assert abs(float(opt.total_norm) - want) <= 2.0 ** -23 * want
    total = optim.clip_grad_norm_(ps, 0.5)
    assert abs(float(total) - want) <= 2.0 ** -23 * want and ps[2].grad is None


@pytest.mark.parametrize('name', ['Adam', 'RMSprop'])
def test_step_makes_a_strided_gradient_dense(name):
    """step() with a transposed .grad on one parameter: the same bits as with that gradient made contiguous beforehand, and the strided
    .grad itself is left as it was."""
    from laff_amd import optim
    g = torch.Generator().manual_seed(5)
    p0 = [torch.randn(6, 4, generator=g), torch.randn(33, generator=g)]
    g0 = [torch.randn(4, 6, generator=g), torch.randn(33, generator=g)]
    results = []
    for dense in (False, True):
        ps = [torch.nn.Parameter(t.to(DEV)) for t in p0]
        ps[0].grad = g0[0].to(DEV).t().contiguous() if dense else g0[0].to(DEV).t()
        ps[1].grad = g0[1].to(DEV)
        assert ps[0].grad.is_contiguous() == dense
        kept = ps[0].grad.clone()
        opt = getattr(optim, name)(ps, lr=1e-2, weight_decay=0.01, grad_clip=0.5)
        opt.step()
        opt.step()
        torch.cuda.synchronize()
        assert ps[0].grad.is_contiguous() == dense and torch.equal(ps[0].grad, kept)
        results.append([p.detach().clone() for p in ps] + [t for p in ps for k, t in sorted(opt.state[p].items()) if k != 'step'])
    assert not torch.equal(results[0][0], p0[0].to(DEV))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_nan_gradient_poisons_the_norm_and_every_parameter():
    vals = {k: list(v) for k, v in _values('mixed', True).items()}
    g = vals['g'][6].copy()
    g[17] = NAN
    vals['g'][6] = g
    for kind in ('adam', 'rmsprop'):
        from laff_amd import ops
        views = {k: _place(vals[k], False)[1] for k in ROLES}
        ws, partials = ops.grad_sqnorm(views['g'])
        total = torch.zeros((), device=DEV)
        ops.optim_step(kind, views['p'], views['g'], views['s1'], views['s2'] if kind == 'adam' else None, max_norm=1.0, workspace=ws,
                       partials=partials, total_norm_out=total, **_hyper(kind))
        assert bool(total.isnan())
        assert all(bool(t.isnan().all()) for t in views['p'])
        # the stand-alone clip: torch's behaviour with error_if_nonfinite=False
        out = ops.grad_scale(views['g'], 1.0, ws, partials)
        assert bool(out.isnan()) and all(bool(t.isnan().all()) for t in views['g'])


def test_graph_capture_replays_the_eager_bits():
    from laff_amd import ops
    vals = _values('chunks', True)
    hyper = _hyper('adam', None, 0.01, 7)
    max_norm = 0.5 * R.total_norm(vals['g'])
    eager = {k: _place(vals[k], False)[1] for k in ROLES}
    ws, partials = ops.grad_sqnorm(eager['g'])
    total_e = torch.zeros((), device=DEV)
    ops.optim_step('adam', eager['p'], eager['g'], eager['s1'], eager['s2'], max_norm=max_norm, workspace=ws, partials=partials,
                   total_norm_out=total_e, **hyper)
    cap = {k: _place(vals[k], False)[1] for k in ROLES}
    ws2 = torch.zeros_like(ws)
    total_c = torch.zeros((), device=DEV)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        ops.grad_sqnorm(cap['g'], ws2)
        ops.optim_step('adam', cap['p'], cap['g'], cap['s1'], cap['s2'], max_norm=max_norm, workspace=ws2, partials=partials,
                       total_norm_out=total_c, **hyper)
    torch.cuda.synchronize()
    assert all(torch.equal(t, torch.tensor(a).to(DEV)) for t, a in zip(cap['p'], vals['p']))       # captured, not run
    gr.replay()
    torch.cuda.synchronize()
    assert float(total_c) == float(total_e)
    for k in ROLES:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(cap[k], eager[k])), k
    # laff_amd.optim's step() refuses a capturing stream: step and lr are launch arguments
    from laff_amd import optim
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    p.grad = torch.ones(8, device=DEV)
    opt = optim.Adam([p])
    gr2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='cannot be captured'):
        with torch.cuda.graph(gr2, capture_error_mode='thread_local'):
            p.grad.mul_(1.0)                              # (a capture is not left empty)
            opt.step()


def test_argument_errors_come_before_any_gpu_work():
    from laff_amd import _lib, ops
    lib, h = ops._context(torch.device(DEV))
    n = 8
    bufs = [torch.full((n + 8,), NAN, device=DEV) for _ in range(4)]
    ptrs = [b.data_ptr() + 16 for b in bufs]
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)

    def step(t=None, count=1, max_norm=0.0, workspace=None, partials=0, **kw):
        hy = dict(kind=0, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
        hy.update(kw)
        hyper = _lib.OptimHyper(**hy)
        table = (_lib.OptimTensor * 1)(t if t is not None else _lib.OptimTensor(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n))
        rc = lib.laff_optim_step(h, table, count, ctypes.byref(hyper), max_norm, workspace, partials, None)
        return rc, lib.laff_last_error().decode()

    E_ARG, E_ALIGN = -1, -3
    for kw, code, word in ((dict(kind=2), E_ARG, 'unknown kind 2'), (dict(step=0), E_ARG, 'step=0'), (dict(beta1=1.0), E_ARG, 'outside'),
                           (dict(beta2=-0.1), E_ARG, 'outside'), (dict(eps=-1.0), E_ARG, 'eps'), (dict(weight_decay=-1.0), E_ARG, 'weight_decay'),
                           (dict(t=_lib.OptimTensor(ptrs[0], ptrs[1], ptrs[2], ptrs[3], -1)), E_ARG, 'n=-1'),
                           (dict(t=_lib.OptimTensor(ptrs[0], None, ptrs[2], ptrs[3], n)), E_ARG, 'null pointer'),
                           (dict(t=_lib.OptimTensor(ptrs[0], ptrs[1], ptrs[2], None, n)), E_ARG, 'null pointer'),
                           (dict(t=_lib.OptimTensor(ptrs[0], ptrs[1] + 2, ptrs[2], ptrs[3], n)), E_ALIGN, '4-byte'),
                           (dict(max_norm=1.0, workspace=None, partials=1), E_ARG, 'null workspace'),
                           (dict(max_norm=1.0, workspace=ws.data_ptr() + 4, partials=1), E_ALIGN, '8-byte'),
                           (dict(count=-1), E_ARG, 'count=-1')):
        rc, msg = step(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    # RMSprop reads no beta1
    assert step(t=_lib.OptimTensor(ptrs[0], ptrs[1], ptrs[2], None, n), kind=1, beta1=7.0, count=0)[0] == 0
    g = (ctypes.c_void_p * 1)(ptrs[1])
    ns = (ctypes.c_longlong * 1)(n)
    assert lib.laff_grad_sqnorm(h, 1, g, ns, ws.data_ptr(), 4) == E_ARG and 'workspace too small' in lib.laff_last_error().decode()
    assert lib.laff_grad_sqnorm(h, 1, g, (ctypes.c_longlong * 1)(-2), ws.data_ptr(), 64) == E_ARG
    assert lib.laff_grad_scale(h, 1, (ctypes.c_void_p * 1)(ptrs[1] + 1), ns, 1.0, ws.data_ptr(), 1, None) == E_ALIGN
    assert lib.laff_grad_scale(h, 1, g, ns, 1.0, None, 1, None) == E_ARG
    # accepted and without effect: count == 0, and entries of n == 0 whatever their pointers
    assert step(count=0)[0] == 0
    assert step(t=_lib.OptimTensor(None, None, None, None, 0))[0] == 0
    assert lib.laff_grad_sqnorm(h, 0, None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert all(bool(b.isnan().all()) for b in bufs)                                              # nothing was written by any of them


# ---- laff_amd.optim ------------------------------------------------------------------------------------------------------------------
def test_clip_grad_norm_against_torch():
    from laff_amd import optim
    vals = _values('mixed', False)
    for factor in (0.5, 2.0):
        mine = [torch.nn.Parameter(torch.zeros(a.size, device=DEV)) for a in vals['g']] + [torch.nn.Parameter(torch.zeros(3, device=DEV))]
        theirs = [torch.nn.Parameter(torch.zeros(a.size, device=DEV)) for a in vals['g']]
        for plist in (mine, theirs):
            for p, a in zip(plist, vals['g']):
                p.grad = torch.tensor(a).to(DEV)
        norm = R.total_norm(vals['g'])
        total = optim.clip_grad_norm_(iter(mine), factor * norm)                                 # any iterable, as torch takes
        want = torch.nn.utils.clip_grad_norm_(iter(theirs), factor * norm)
        assert total.dim() == 0 and total.is_cuda and mine[-1].grad is None
        assert abs(float(total) - norm) <= 2.0 ** -23 * norm and abs(float(total) - float(want)) <= 2.0 ** -22 * float(want)
        c = R.clip_coef(norm, factor * norm)
        worst = 0.0
        for p, q, a in zip(mine, theirs, vals['g']):
            got, ref = p.grad.cpu().numpy().astype(np.float64), c * a.astype(np.float64)
            assert np.all(np.abs(got - ref) <= R.CLIP_CONST * U * np.abs(ref))
            assert np.all(np.abs(got - q.grad.cpu().numpy().astype(np.float64)) <= 4 * U * np.abs(a.astype(np.float64)))
            if factor == 2.0:
                assert np.array_equal(p.grad.cpu().numpy().view(np.int32), a.view(np.int32))          # c = 1: the same bits
            nz = ref != 0
            worst = max(worst, float(np.max(np.abs(got - ref)[nz] / (R.CLIP_CONST * U * np.abs(ref[nz])))) if nz.any() else 0.0)
        print('clip_grad_norm_ x%.1f: c g uses %.3f of 3 u |c g|' % (factor, worst))
    # a non-contiguous gradient is scaled through a dense copy and written back
    p = torch.nn.Parameter(torch.zeros(6, 4, device=DEV))
    p.grad = torch.arange(24.0, device=DEV).reshape(4, 6).t()
    ref = p.grad.clone()
    total = optim.clip_grad_norm_(p, 1.0)
    assert not p.grad.is_contiguous() and torch.allclose(p.grad, ref / (float(total) + 1e-6), rtol=1e-6, atol=0)


SEQ_SHAPES = [(96, 40), (130,), (64, 33), (257,)]            # groups: the first two at lr, the last two at lr / 20


@functools.lru_cache(maxsize=None)
def _sequence():
    g = torch.Generator().manual_seed(21)
    params = [torch.randn(s, generator=g) for s in SEQ_SHAPES]
    grads = [[torch.randn(s, generator=g) * 10.0 ** float(-3.0 * torch.rand((), generator=g)) for s in SEQ_SHAPES] for _ in range(5)]
    return params, grads


def _run_sequence(make, clip, dtype, device, grad_clip):
    """5 steps over two groups; parameter 1 has no gradient at step 2 (its step count lags afterwards); StepLR steps once after step 3.
    clip: the function applied before opt.step(), or None when the optimizer clips by itself."""
    params, grads = _sequence()
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in params]
    opt = make([{'params': ps[:2]}, {'params': ps[2:], 'lr': 1e-3 / 20}])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    for i, gs in enumerate(grads):
        held = []
        for j, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if (i == 1 and j == 1) else g.to(device=device, dtype=dtype).clone()
            held.append(None if p.grad is None else p.grad.clone())
        if clip is not None:
            clip(ps, grad_clip)
        opt.step()
        if clip is None:                                 # the fused clip leaves .grad as it was
            assert all((p.grad is None and k is None) or torch.equal(p.grad, k) for p, k in zip(ps, held))
        if i == 2:
            sched.step()
    out = {}
    for j, p in enumerate(ps):
        out['p%d' % j] = p.detach().double().cpu()
        for k, t in opt.state[p].items():
            out['%s%d' % (k, j)] = t.detach().double().cpu()
    return out


@pytest.mark.parametrize('name', ['Adam', 'RMSprop'])
def test_five_steps_two_groups_against_torch_in_float64(name):
    from laff_amd import optim
    kw = dict(lr=1e-3, eps=1e-4, weight_decay=0.01) if name == 'Adam' else dict(lr=1e-3, weight_decay=0.01)
    _, grads = _sequence()
    grad_clip = 0.5 * min(R.total_norm([g.numpy() for j, g in enumerate(gs) if (i, j) != (1, 1)])
                          for i, gs in enumerate(grads))                                         # active at every step
    theirs = lambda groups: getattr(torch.optim, name)(groups, **kw)      # noqa: E731
    ref = _run_sequence(theirs, torch.nn.utils.clip_grad_norm_, torch.float64, 'cpu', grad_clip)
    f32 = _run_sequence(theirs, torch.nn.utils.clip_grad_norm_, torch.float32, 'cpu', grad_clip)
    got = _run_sequence(lambda groups: getattr(optim, name)(groups, grad_clip=grad_clip, **kw), None, torch.float32, DEV, grad_clip)
    assert sorted(got) == sorted(ref)
    assert got['step1'] == 4.0 and got['step0'] == 5.0
    for k in sorted(ref):
        if k.startswith('step'):
            assert float(got[k]) == float(ref[k])
            continue
        r = ref[k]
        top = float(r.abs().max())
        e32 = float((f32[k] - r).abs().max()) / top
        err = (got[k] - r).abs()
        print('%-14s device %.3e  fp32 CPU %.3e  bound %.3e' % (k, float(err.max()) / top, e32, max(4.0 * e32, TOL_UNIT)))
        assert float(err.max()) <= max(4.0 * e32, TOL_UNIT) * top, k
        # where only the floor admits an element it is a state element that is tiny next to its tensor
        floor_only = err > 4.0 * e32 * top
        assert not k.startswith('p') or not bool(floor_only.any()), k
        assert bool((r.abs()[floor_only] < 1e-6 * top).all()), k


def test_state_dict_moves_to_torch_on_the_device():
    from laff_amd import optim
    params, grads = _sequence()
    kw = dict(lr=1e-3, eps=1e-4, weight_decay=0.01)
    ps = [torch.nn.Parameter(p.to(DEV).clone()) for p in params]
    mine = optim.Adam(ps, **kw)
    for gs in grads[:2]:
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        mine.step()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    theirs = torch.optim.Adam(qs, **kw)
    theirs.load_state_dict(copy.deepcopy(mine.state_dict()))      # as torch.save / torch.load would: load_state_dict shares 'step'
    before = [(p.detach().cpu().numpy(), mine.state[p]['exp_avg'].cpu().numpy(), mine.state[p]['exp_avg_sq'].cpu().numpy()) for p in ps]
    for p, q, g in zip(ps, qs, grads[2]):
        p.grad = g.to(DEV)
        q.grad = g.to(DEV)
    mine.step()
    theirs.step()
    torch.cuda.synchronize()
    worst = 0.0
    for p, q, g, (p0, m0, v0) in zip(ps, qs, grads[2], before):
        assert float(theirs.state[q]['step']) == 3.0 and float(mine.state[p]['step']) == 3.0
        gn = [g.numpy().ravel()]
        p0, m0, v0 = [p0.ravel()], [m0.ravel()], [v0.ravel()]
        G = R.gmag(p0, gn, 1.0, 0.01)
        pr, mr, vr = R.adam(p0, gn, m0, v0, 1e-3, 0.9, 0.999, 1e-4, 0.01, 3)
        # the whole step's bound: p' from exact moments, plus what the moments' own bounds move it by
        ss, bc2 = 1e-3 / (1.0 - 0.9 ** 3), 1.0 - 0.999 ** 3
        den = np.sqrt(vr[0]) / np.sqrt(bc2) + 1e-4
        bm, bv = R.bound_m(m0, G, 0.9)[0], R.bound_v(v0, G, 0.999)[0]
        dden = np.where(vr[0] > 0, bv / (2.0 * np.sqrt(np.maximum(vr[0], 1e-300)) * np.sqrt(bc2)), 0.0)
        bound = R.bound_p_adam(pr, mr, vr, 1e-3, 0.9, 0.999, 1e-4, 3)[0] + ss * bm / den + ss * np.abs(mr[0]) / den ** 2 * dden
        a, b = p.detach().cpu().numpy().ravel().astype(np.float64), q.detach().cpu().numpy().ravel().astype(np.float64)
        assert np.all(np.abs(a - pr[0]) <= bound)
        assert np.all(np.abs(a - b) <= 4.0 * bound)
        worst = max(worst, float(np.max(np.abs(a - b) / bound)))
    print('optim.Adam and torch.optim.Adam after the hand-over: %.3f bounds apart at most (4 allowed)' % worst)


# ---- end to end: one training step with every stage on this library's kernels -------------------------------------------------------
def _towers():
    """The graph of tests/test_gpu_fc_backward.py's end-to-end test: L = 3, H = 2, d = 64, B = 16, both sides, with its seed search
    (pairs 1e-4 clear of every hinge decision, in float64)."""
    B, H, d, margin = 16, 2, 64, 0.2
    dims = (24, 16, 8)
    def build():
        txt, vis = TR.Side(dims, H * d, H), TR.Side(dims, H * d, H)
        with torch.no_grad():
            for p in list(txt.proj) + list(vis.proj):
                p.fc1.bias.uniform_(-0.2, 0.2)
        z = torch.randn(B, 8)
        ft = [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims]
        fv = [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims]
        with torch.no_grad():
            return (txt, vis, ft, fv), TR.side_f64(txt, ft, clone=True)[0], TR.side_f64(vis, fv, clone=True)[0]
    txt, vis, ft, fv = TR.hinge_clear_seed(build, margin, 100)
    return txt, vis, ft, fv, margin


def test_one_training_step_end_to_end():
    """TransformNet.train().plane() -> fuse_planes on each side -> loss.MarginRankingLoss -> backward -> one
    optim.Adam(lr=1e-3, eps=1e-4, grad_clip=2.0) step over both towers' parameters, against the float64 graph stepped by
    torch.nn.utils.clip_grad_norm_ and torch.optim.Adam.  Every parameter T:  max |device - float64| <= max(4 e32, 1.5e-6) max |T|,
    e32 from the fp32 CPU graph stepped by torch."""
    from laff_amd import loss as laff_loss
    from laff_amd import optim
    txt, vis, ft, fv, margin = _towers()
    stepped, norms = {}, {}
    for dtype in (torch.float64, torch.float32):
        (Et, lt), (Ev, lv) = TR.side_f64(txt, ft, dtype, clone=True), TR.side_f64(vis, fv, dtype, clone=True)
        TR.margin_loss_f64(Et, Ev, margin).backward()
        leaves = {'txt.' + k: v for k, v in lt.items() if not k.startswith('feat')}
        leaves.update({'vis.' + k: v for k, v in lv.items() if not k.startswith('feat')})
        ps = list(leaves.values())
        norms[dtype] = float(torch.nn.utils.clip_grad_norm_(ps, 2.0))
        torch.optim.Adam(ps, lr=1e-3, eps=1e-4).step()
        stepped[dtype] = {k: v.detach().double() for k, v in leaves.items()}
    txt, vis = txt.to(DEV).train(), vis.to(DEV).train()
    named = {'txt.' + n: p for n, p in txt.named_parameters()}
    named.update({'vis.' + n: p for n, p in vis.named_parameters()})
    before = {n: p.detach().clone() for n, p in named.items()}
    opt = optim.Adam(list(named.values()), lr=1e-3, eps=1e-4, grad_clip=2.0)
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    crit(txt([f.to(DEV) for f in ft]), vis([f.to(DEV) for f in fv])).backward()
    opt.step()
    torch.cuda.synchronize()
    print('global gradient norm: device %.6f  float64 %.6f  (grad_clip 2.0)' % (float(opt.total_norm), norms[torch.float64]))
    assert abs(float(opt.total_norm) - norms[torch.float64]) <= 2e-5 * norms[torch.float64]
    without = sorted(n for n, p in named.items() if p.grad is None)
    assert sorted(set(named) - set(without)) == sorted(stepped[torch.float64])
    for n in without:                                     # gw and the unused layer norm: no gradient, no state, not a bit moved
        assert torch.equal(named[n], before[n]) and named[n] not in opt.state
    for n, r in stepped[torch.float64].items():
        top = float(r.abs().max())
        e32 = float((stepped[torch.float32][n] - r).abs().max()) / top
        err = float((named[n].detach().double().cpu() - r).abs().max()) / top
        print('%-52s device %.3e  fp32 CPU %.3e  bound %.3e' % (n, err, e32, max(4.0 * e32, TOL_UNIT)))
        assert err <= max(4.0 * e32, TOL_UNIT), (n, err, e32)
        assert not torch.equal(named[n], before[n]) or n.endswith('embedding_common.0.bias')


def test_twenty_steps_lower_the_dual_softmax_loss():
    from laff_amd import loss as laff_loss
    from laff_amd import optim
    txt, vis, ft, fv, _ = _towers()
    txt, vis = txt.to(DEV).train(), vis.to(DEV).train()
    dt, dv = [f.to(DEV) for f in ft], [f.to(DEV) for f in fv]
    opt = optim.Adam(list(txt.parameters()) + list(vis.parameters()), lr=1e-3, eps=1e-4, grad_clip=2.0)
    crit = laff_loss.DualSoftmaxLoss()
    losses = []
    for _ in range(21):
        opt.zero_grad()
        loss = crit(txt(dt), vis(dv))
        losses.append(loss.detach())
        loss.backward()
        opt.step()
    losses = [float(x) for x in losses]
    print('dual softmax loss: %.6f at the start, %.6f after 20 steps' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
