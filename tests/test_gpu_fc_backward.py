"""laff_fc_backward, ops.fc_backward and the training-mode TransformNet on the MI355X.

Kernel level.  The saved forward output A is an input of the call, so the reference is the float64 evaluation of the formulas of
tests/fc_bwd_ref.py on the very fp32 X, W, A, dA handed to the device; no forward error enters.  The bound is derived, not measured, and
holds element by element (u = 2^-24, magnitudes in float64):

    |dW - ref| <= (N + 4) u |dA|^T |X|      |dX - ref| <= (D + 4) u |dA| |W|      |db - ref| <= (N + 4) u sum_n |dA|

Any summation order of a K-term fp32 dot product, fma or not, stays within gamma_K sum |a b|; forming dz from a costs at most three
roundings against a factor |act'| <= 1 -- hence |dA| and the + 4.  An element over the bound is a bug.

Module level and end to end: the rule of tests/test_gpu_fuse_backward.py, max |device - float64| / max |float64| within the larger of
4 x the same error of the float32 CPU graph and 1.5e-6 (end to end: that test's bound formula, copied).

The table at the end of the file records the largest fraction of its bound that each tensor used.
"""
import functools

import numpy as np
import pytest
import torch

import fc_bwd_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')

# layouts of every operand and output: 'dense' rows on a 16-byte aligned base; 'pitch4' a wider pitch that keeps the rows 16-byte aligned
# (the 16-byte loads, strided); 'pitch3' a wider pitch that does not (the generic loads); 'offset' a base pointer 4 bytes past a 16-byte
# boundary.  (N, Dk, D, activation, layout)
CASES = [
    (1, 1, 1, None, 'dense'),
    (1, 4, 4, 'tanh', 'dense'),
    (3, 5, 7, 'sigmoid', 'dense'),            # odd widths: the generic loads
    (33, 68, 132, 'relu', 'pitch4'),
    (129, 100, 64, 'tanh', 'offset'),         # the smallest N at which the sum over N is cut
    (257, 36, 260, 'sigmoid', 'pitch3'),
    (64, 512, 512, None, 'dense'),            # exact tiles: the instantiations without bounds checks, 64 x 64
    (130, 516, 36, 'relu', 'dense'),
    # beyond the issue's list: the 128 x 128 tiles, which a product takes once they make 256 blocks -- dW uncut and dX cut in 16 in
    # the first, dW cut in 4 and dX uncut in the second
    (5, 2050, 2040, 'tanh', 'pitch3'),
    (520, 8100, 6, 'relu', 'pitch4'),
    (128, 2048, 2048, 'sigmoid', 'dense'),    # exact tiles of 128 x 128 in both products, dX cut in 16
]


def _id(c):
    return 'N%d-Dk%d-D%d-%s-%s' % c


@functools.lru_cache(maxsize=None)
def _case(c):
    """The fp32 operands of a case on the CPU, the float64 reference and the bounds -- computed once, shared, never written."""
    N, Dk, D, act, layout = c
    g = torch.Generator().manual_seed(N * 1000003 + Dk * 1009 + D)
    x = torch.randn(N, Dk, generator=g)
    w = torch.randn(D, Dk, generator=g) / Dk ** 0.5
    b = 0.1 * torch.randn(D, generator=g)
    scale = 3.0 if act in ('tanh', 'sigmoid') else 1.0                  # logits x 3: part of A sits in saturation
    a = R.forward_torch(scale * x, w, scale * b, act)
    da = torch.randn(N, D, generator=g)
    if act == 'relu' and N * D >= 16:
        assert (a == 0).any() and (a > 0).any()
    if act == 'tanh' and N * D >= 1000:
        assert (a.abs() > 0.999).any()
    return dict(c=c, x=x, w=w, a=a, da=da, ref=R.backward(x, w, a, da, act), bounds=R.bounds(x, w, da))


@functools.lru_cache(maxsize=None)
def _device_inputs(c):
    cs = _case(c)
    return tuple(TR.place(cs[k], c[4]) for k in ('x', 'w', 'a', 'da'))


def _launch(c, want=(True, True, True)):
    """ops.fc_backward into NaN-framed buffers of the case's layout: the three outputs (None where not wanted) after the canary check."""
    from laff_amd import ops
    N, Dk, D, act, layout = c
    (_, x), (_, w), (_, a), (_, da) = _device_inputs(c)
    bufs = [TR.pitched(N, Dk, layout) if want[0] else None, TR.pitched(D, Dk, layout) if want[1] else None,
            TR.out_vec(D, layout != 'offset') if want[2] else None]
    res = ops.fc_backward(x, w, a, da, act, *want, out=tuple(None if b is None else b[1] for b in bufs))
    torch.cuda.synchronize()
    for name, b, r in zip(('dx', 'dw', 'db'), bufs, res):
        if b is None:
            assert r is None
            continue
        assert r.data_ptr() == b[1].data_ptr()
        assert TR.untouched_around(*b), '%s: a write outside the output' % name
        assert not r.isnan().any(), '%s: an element was not written (or read a canary)' % name
    for ibuf, iview in _device_inputs(c):
        assert TR.untouched_around(ibuf, iview)
    return res


def _check(c, res, label=''):
    cs = _case(c)
    for name, got, ref, bound in zip(('dx', 'dw', 'db'), res, cs['ref'], cs['bounds']):
        if got is None:
            continue
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        assert err.shape == bound.shape
        # a zero bound (a zero row of |dA|) admits only the exact zero
        frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))
        print('%s %s%s: max err %.3e, largest err / bound %.4f' % (_id(c), name, label, float(err.max(initial=0.0)), frac))
        assert frac <= 1.0, (name, frac)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_backward_vs_float64(c):
    _check(c, _launch(c))


def test_plan_cuts_the_sum_over_n_by_the_shape_alone():
    from laff_amd import ops
    chunks = {c[:3]: ops.fc_backward_plan(*c[:3])[0] for c in CASES}
    assert sum(1 for v in chunks.values() if v > 1) >= 2 and sum(1 for v in chunks.values() if v == 1) >= 2
    assert chunks[(129, 100, 64)] == 2 and ops.fc_backward_plan(128, 100, 64)[:2] == (1, 0)       # the smallest N that is cut
    assert chunks[(257, 36, 260)] == 3 and chunks[(64, 512, 512)] == 1 and chunks[(520, 8100, 6)] == 4
    # dX's sum over D is cut likewise, and both tile variants of both products are among the cases, each cut and uncut
    plans = {c[:3]: ops.fc_backward_plan(*c[:3]) for c in CASES}
    assert plans[(33, 68, 132)][2:] == (2, 0) and plans[(64, 512, 512)][2:] == (4, 0) and plans[(130, 516, 36)][2:] == (1, 0)
    assert plans[(5, 2050, 2040)] == (1, 16 * 5 * 2050 * 4, 16, 3) and plans[(520, 8100, 6)][2:] == (1, 3)
    assert plans[(128, 2048, 2048)] == (1, 16 * 128 * 2048 * 4, 16, 3)
    # the training call: dW + db from a batch of 128 rows, no cut and no workspace
    assert ops.fc_backward_plan(128, 512, 4096, want_dx=False)[:2] == (1, 0) and ops.fc_backward_plan(128, 4096, 4096, want_dx=False) == (1, 0, 8, 3)


@pytest.mark.parametrize('c', [CASES[2], CASES[3], CASES[4], CASES[5]], ids=_id)
def test_each_output_absent_in_turn(c):
    full = _launch(c)
    for skip in range(3):
        want = tuple(i != skip for i in range(3))
        res = _launch(c, want)
        for i in range(3):
            assert (res[i] is None) == (i == skip)
            if res[i] is not None:
                assert torch.equal(res[i], full[i]), 'output %d changes when output %d is absent' % (i, skip)
    only_db = _launch(c, (False, False, True))
    assert torch.equal(only_db[2], full[2])
    assert _launch(c, (False, False, False)) == (None, None, None)


@pytest.mark.parametrize('c', [CASES[3], CASES[5], CASES[6], CASES[8]], ids=_id)
def test_repeats_are_bit_identical(c):
    first = [t.clone() for t in _launch(c)]
    again = _launch(c)
    assert all(torch.equal(p, q) for p, q in zip(first, again))


def test_empty_batch_writes_zeros_and_nothing_else():
    from laff_amd import ops
    Dk, D = 5, 7
    w = torch.randn(D, Dk, device=DEV)
    for layout in ('dense', 'pitch3'):
        bdw, bdb = TR.pitched(D, Dk, layout), TR.out_vec(D, layout != 'offset')
        dx, dw, db = ops.fc_backward(torch.empty(0, Dk, device=DEV), w, torch.empty(0, D, device=DEV), torch.empty(0, D, device=DEV), 'tanh',
                                     out=(None, bdw[1], bdb[1]))
        torch.cuda.synchronize()
        assert tuple(dx.shape) == (0, Dk) and not dw.any() and not db.any() and tuple(dw.shape) == (D, Dk) and tuple(db.shape) == (D,)
        assert TR.untouched_around(*bdw) and TR.untouched_around(*bdb)


def test_argument_errors():
    from laff_amd import ops
    x, w = torch.randn(4, 8, device=DEV), torch.randn(16, 8, device=DEV)
    a = torch.randn(4, 16, device=DEV)
    with pytest.raises(ValueError, match='do not fit'):
        ops.fc_backward(x, w, a[:, :15], a, 'tanh')
    with pytest.raises(ValueError, match='activation'):
        ops.fc_backward(x, w, a, a, 'gelu')
    with pytest.raises(TypeError):
        ops.fc_backward(x.double(), w, a, a, 'tanh')
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fc_backward(x.cpu(), w, a, a, 'tanh')
    # a non-unit inner stride is made dense, not refused
    wide = torch.randn(4, 32, device=DEV)
    got = ops.fc_backward(x, w, a, wide[:, ::2], None)
    want = ops.fc_backward(x, w, a, wide[:, ::2].contiguous(), None)
    assert all(torch.equal(p, q) for p, q in zip(got, want))


def test_graph_capture_replays_the_eager_bits():
    from laff_amd import ops
    c = CASES[4]                                           # cut in two: the product, then the two adds of the partial tiles
    N, Dk, D, act, layout = c
    (_, x), (_, w), (_, a), (_, da) = _device_inputs(c)
    eager = [t.clone() for t in ops.fc_backward(x, w, a, da, act)]
    outs = (torch.full((N, Dk), NAN, device=DEV), torch.full((D, Dk), NAN, device=DEV), torch.full((D,), NAN, device=DEV))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        ops.fc_backward(x, w, a, da, act, out=outs)
    gr.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(outs, eager))
    _check(c, outs, ' (graph)')


# ---- TransformNet in training mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_norm, activation, dropout', [(True, 'tanh', 0.0), (True, 'relu', 0.0), (False, 'sigmoid', 0.0),
                                                             (False, None, 0.0), (False, 'tanh', 0.2)],
                         ids=lambda v: str(v))
def test_transform_net_train(batch_norm, activation, dropout):
    from laff_amd.model.model import TransformNet
    torch.manual_seed(11)
    N = 33
    net = TransformNet((68, 132), batch_norm=batch_norm, activation=activation, dropout=dropout)
    with torch.no_grad():
        net.fc1.bias.normal_(0.0, 0.1)
    W, b = net.fc1.weight.detach().clone(), net.fc1.bias.detach().clone()
    x, dE = torch.randn(N, 68), torch.randn(N, 132)
    net = net.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    assert y.requires_grad and tuple(y.shape) == (N, 132)
    y.backward(dE.to(DEV))
    mask = None
    if dropout:
        # the mask from the output: a tanh output is never exactly zero for these inputs
        a64 = R.forward_torch(x.double(), W.double(), b.double(), activation)
        assert (a64 != 0).all() and (R.forward_torch(x, W, b, activation) != 0).all()
        mask = (y.detach() != 0).cpu()
        kept = float(mask.double().mean())
        assert abs(kept - (1.0 - dropout)) <= 5.0 * ((1.0 - dropout) * dropout / mask.numel()) ** 0.5, kept
    ref = TR.layer_graph(torch.float64, W, b, x, dE, activation, batch_norm, mask, dropout)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, activation, batch_norm, mask, dropout)
    got = {'y': y, 'x.grad': xd.grad, 'fc1.weight.grad': net.fc1.weight.grad, 'fc1.bias.grad': net.fc1.bias.grad}
    if batch_norm:
        got.update({'bn1.weight.grad': net.bn1.weight.grad, 'bn1.bias.grad': net.bn1.bias.grad, 'running_mean': net.bn1.running_mean,
                    'running_var': net.bn1.running_var})
    TR.compare(got, ref, f32)
    # plane(): the same bits, plain and dense, accepted by the training-mode fusion blocks as it is; `pending` is not used
    pending = []
    src, tile, scale, shift = net.plane(xd.detach(), heads=2, pending=pending)
    assert pending == [] and tile is False and scale is None and shift is None and src.requires_grad
    assert dropout or torch.equal(src, y)
    # eval afterwards: today's code path
    net.eval()
    with torch.no_grad():
        ye = net(x.to(DEV))
    assert not ye.requires_grad and tuple(ye.shape) == (N, 132)


def test_no_dx_launch_for_inputs_without_grad(monkeypatch):
    from laff_amd import ops
    from laff_amd.model.model import TransformNet
    torch.manual_seed(12)
    net = TransformNet((68, 132), batch_norm=False, activation='tanh', dropout=0.0).to(DEV).train()
    x, dE = torch.randn(33, 68, device=DEV), torch.randn(33, 132, device=DEV)
    calls = []
    real = ops.fc_backward

    def spy(*args, **kw):
        calls.append(dict(kw))
        return real(*args, **kw)
    monkeypatch.setattr(ops, 'fc_backward', spy)
    xg = x.clone().requires_grad_(True)
    net(xg).backward(dE)
    gw, gb = net.fc1.weight.grad.clone(), net.fc1.bias.grad.clone()
    net.zero_grad()
    net(x).backward(dE)
    assert [k['want_dx'] for k in calls] == [True, False] and all(k['want_dw'] and k['want_db'] for k in calls)
    assert xg.grad is not None and torch.equal(net.fc1.weight.grad, gw) and torch.equal(net.fc1.bias.grad, gb)


# ---- end to end: a LAFF tower's training step with every stage on this library's kernels -------------------------------------------
def test_end_to_end_two_towers_margin_loss():
    """L = 3, H = 2, d = 64, B = 16: TransformNet.train().plane() projections -> Multi_head_MyApply_Attention.train().fuse_planes on each
    side -> loss.MarginRankingLoss -> backward.  Every parameter gradient and both sides' input gradients against the same graph in
    float64.

    Bound of a gradient tensor T, element by element:  max(4 e32, 1.5e-6) max |T|  +  GRAD_ABS sum_j |dT / dE_j|
    (tests/test_gpu_fuse_backward.py::test_end_to_end_two_towers_margin_loss, whose graph this is with its Linear + tanh replaced)."""
    from laff_amd import loss as laff_loss
    B, L, H, d, margin = 16, 3, 2, 64, 0.2
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
            return (txt, vis, ft, fv), TR.side_f64(txt, ft)[0], TR.side_f64(vis, fv)[0]
    txt, vis, ft, fv = TR.hinge_clear_seed(build, margin, 100)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        (Et, lt), (Ev, lv) = TR.side_f64(txt, ft, dtype), TR.side_f64(vis, fv, dtype)
        TR.margin_loss_f64(Et, Ev, margin).backward()
        grads[dtype] = ({k: v.grad.double() for k, v in lt.items()}, {k: v.grad.double() for k, v in lv.items()}, Et, Ev)
    # sum_j |dT / dE_j| per side, from the float64 graph: one batched backward over the unit vectors of E
    absjac = [TR.abs_jacobian(*TR.side_f64((txt, vis)[side], (ft, fv)[side])) for side in (0, 1)]
    # the device
    txt, vis = txt.to(DEV).train(), vis.to(DEV).train()
    dt = [f.to(DEV).requires_grad_(True) for f in ft]
    dv = [f.to(DEV).requires_grad_(True) for f in fv]
    Et, Ev = txt(dt), vis(dv)
    assert Et.shape == (B, H, d)
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    loss = crit(Et, Ev)
    loss.backward()
    torch.cuda.synchronize()
    l64 = float(TR.margin_loss_f64(grads[torch.float64][2].detach(), grads[torch.float64][3].detach(), margin))
    assert abs(loss.item() - l64) <= 2e-5 * max(1.0, abs(l64))
    worst = 0.0
    for side, (mod, feats) in enumerate(((txt, dt), (vis, dv))):
        got = {n: p.grad for n, p in mod.named_parameters()}
        got.update({'feat%d' % i: f.grad for i, f in enumerate(feats)})
        for h in range(H):
            assert got.pop('att.attention_layer.%d.global_emb_weight_net.weight' % h) is None       # gw: no gradient
        for n in ('att.layer_norm.weight', 'att.layer_norm.bias'):                                  # declared and unused
            assert got.pop(n) is None
        ref64, ref32 = grads[torch.float64][side], grads[torch.float32][side]
        assert sorted(got) == sorted(ref64)
        for n, g in got.items():
            r = ref64[n]
            if n.endswith('embedding_common.0.bias'):
                assert not g.any(), n                                                               # db of the fusion: exactly zero
                continue
            bound, e32, top = TR.end_to_end_bound(r, ref32[n], absjac[side][n])
            err = (g.cpu().double() - r).abs()
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            print('side %d %-52s max |g| %.3e  err %.3e  fp32 CPU %.2e  bound %.3e .. %.3e  worst err / bound %.3f'
                  % (side, n, top, float(err.max()), e32, float(bound.min()), float(bound.max()), ratio))
            assert ratio <= 1.0, (n, ratio)
    print('end to end: worst err / bound %.3f' % worst)


# MEASURED on the MI355X by test_backward_vs_float64: per case and tensor the largest fraction of its element-by-element bound that the
# device used, with the largest absolute error beside it.  Largest over all cases: dx 0.31 at (520, 8100, 6), dw 0.38 and db 0.14 at
# (5, 2050, 2040) -- sums of 6 and 5 terms, where the bound is 10 u and 9 u of the products' magnitudes; 0.0001 .. 0.07 elsewhere, in
# line with the 0.01 typical and 0.10 at most of a numpy emulation of sequential fp32 chains.  Module level: largest error 4.2e-7 of a
# tensor's largest entry (bounds 1.5e-6 .. 2.5e-6).  End to end: the worst element used 0.155 of its bound.
#   case                                 dx                       dw                       db
#   N1-Dk1-D1-None-dense                 0.1288 (1.002e-07)       0.0117 (2.207e-09)       0.0000 (0.000e+00)
#   N1-Dk4-D4-tanh-dense                 0.0035 (1.182e-09)       0.0513 (2.881e-09)       0.0356 (2.020e-09)
#   N3-Dk5-D7-sigmoid-dense              0.0251 (7.591e-08)       0.0588 (4.269e-08)       0.0282 (2.198e-08)
#   N33-Dk68-D132-relu-pitch4            0.0075 (6.172e-07)       0.0489 (2.586e-06)       0.0184 (1.125e-06)
#   N129-Dk100-D64-tanh-offset           0.0196 (3.940e-07)       0.0075 (4.920e-06)       0.0040 (3.413e-06)
#   N257-Dk36-D260-sigmoid-pitch3        0.0010 (4.342e-07)       0.0009 (2.272e-06)       0.0008 (2.444e-06)
#   N64-Dk512-D512-None-dense            0.0028 (1.211e-06)       0.0718 (1.192e-05)       0.0356 (8.028e-06)
#   N130-Dk516-D36-relu-dense            0.0552 (1.478e-07)       0.0113 (7.841e-06)       0.0054 (4.577e-06)
#   N5-Dk2050-D2040-tanh-pitch3          0.0001 (4.234e-07)       0.3836 (1.353e-06)       0.1395 (3.943e-07)
#   N520-Dk8100-D6-relu-pitch4           0.3113 (1.736e-08)       0.0020 (1.987e-05)       0.0004 (5.579e-06)
#   N128-Dk2048-D2048-sigmoid-dense      0.0000 (1.773e-07)       0.0070 (4.171e-06)       0.0026 (2.241e-06)
