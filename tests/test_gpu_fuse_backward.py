"""laff_fuse_backward, ops.fuse_backward and the training-mode attention modules on a real MI355X, element by element against float64
autograd of tests/fuse_ref.attention on the very fp32 inputs (tests/fuse_bwd_ref.py).

Error of a tensor = max |device - float64| / max |float64| (fuse_bwd_ref.rel_err; a float64 tensor that is zero throughout, dw at
L = 1, admits only zeros).  Bound of a case = the larger of
  (i)  4 x the same error of float32 CPU autograd of the restatement on that case -- the kernel's butterfly and two-stage sums associate
       differently from aten's, and
  (ii) 1.5e-6, the forward's own contract (TOL_UNIT of tests/test_gpu_fuse_routes.py): a gradient cannot be asked to beat the forward
       it recomputes.
db is exactly zero.  Before each launch the float64 reference asserts min |g| >= 0.05 and, under the per-head l2norm, min |raw_l| >= 0.05:
it stays clear of the 1 / r singularity by itself.  Inputs come from the first seed of a case's fixed seed range that clears both, found
on the CPU: no case is skipped.

MEASURED: test_backward_vs_float64 prints, per case, the float32 CPU error (i) and the device error of dx and dw; the table at the end of
this file lists them as measured on the MI355X.  Largest device error: dx 1.4e-6, dw 1.6e-6 (the near one-hot case, bounds 3.0e-5 and
3.8e-5); outside the peaked cases dx 2.2e-7, dw 3.1e-7; closest to a bound: dw at 0.17 x.
"""
import functools
import itertools

import pytest
import torch

import fuse_bwd_ref as R
import fuse_ref
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL_UNIT = TR.TOL_UNIT
MULTI = dict(with_ave=True, mul=True)              # what Multi_head_MyApply_Attention defaults to


def _flag_name(kw):
    names = [k for k, v in sorted(kw.items()) if v is True and k != 'split_head'] + ([] if kw.get('split_head', True) else ['nosplit'])
    return '+'.join(names) or 'plain'


# (N, L, H, d, flags, logit scale): the smallest shapes at which each piece can go wrong
CASES = []
CASES += [(N, 2, 3, 260, MULTI, None) for N in (1, 3, 5, 257)]                # a partial block of four waves; several dw partial rows
CASES += [(5, L, 3, 260, MULTI, None) for L in (1, 5, 8)]                      # (L = 2 above)
CASES += [(5, 2, H, 256, MULTI, None) for H in (1, 8)]                         # (H = 3 above)
CASES += [(5, 3, 2, d, MULTI, None) for d in (4, 252, 256, 512)]               # register variants: partial / whole heads, NCH 1 and 2
CASES += [(5, 3, 2, d, MULTI, None) for d in (516, 1024)]                      # streaming
CASES += [(6, 3, 2, 516, dict(with_ave=True, mul=True, l2norm_each_head=True), None)]      # streaming with its second dx pass
CASES += [(5, 3, 3, d, dict(with_ave=True, mul=True, split_head=False, l2norm_each_head=n), None)
          for d in (260, 516) for n in (False, True)]                           # no split heads: dx summed over the heads
CASES += [(5, 5, 3, 260, dict(with_ave=a, mul=m, l2norm_each_head=n, split_head=s), None)
          for a, m, n, s in itertools.product((False, True), repeat=4)]        # every flag combination
CASES += [(5, 5, 3, 260, dict(just_average=True), None), (5, 5, 3, 516, dict(just_average=True, split_head=False), None)]
CASES += [(9, 4, 2, 128, MULTI, 3.0),                                          # peaked softmax: logits of standard deviation 3 in a row
          (9, 4, 2, 128, MULTI, 12.0)]                                         # near one-hot
# Several rows per wavefront.  fuse_bwd_plan gives a block more than four rows only once N / 4 exceeds 4096 / H row chunks (4096 without
# split heads): below that every wavefront has one row at most, and the register kernel's dw share carried across rows, the streaming
# kernel's read-modify-write of its workspace row and the no-split accumulation over a wavefront's later rows would run unchecked.
CASES += [(4100, 2, 8, 4, MULTI, None),                                        # register variant, 12 rows a block: 3 per wavefront
          (2100, 2, 8, 260, dict(MULTI, l2norm_each_head=True), None),         # NCH = 2, 8 rows a block
          (2100, 2, 8, 516, MULTI, None),                                      # streaming, 8 rows a block
          (16500, 2, 3, 4, dict(MULTI, split_head=False), None)]               # no split heads, 8 rows a block
_FLAG_DEFAULTS = dict(with_ave=False, mul=False, l2norm_each_head=False, split_head=True, just_average=False)
CASES = list(dict.fromkeys((N, L, H, d, tuple(sorted(dict(_FLAG_DEFAULTS, **kw).items())), sc) for N, L, H, d, kw, sc in CASES))


def _key(kw):
    return tuple(sorted(dict(_FLAG_DEFAULTS, **kw).items()))


def _case_id(c):
    N, L, H, d, kw, sc = c
    return 'N%d-L%d-H%d-d%d-%s%s' % (N, L, H, d, _flag_name(dict(kw)), '' if sc is None else '-std%g' % sc)


def _inputs(N, L, H, d, kw, scale, seed):
    g = torch.Generator().manual_seed(seed)
    Dp = H * d if kw.get('split_head', True) else d
    planes = (0.5 * torch.randn(N, L, Dp, generator=g, dtype=torch.float64)).float()
    w = (torch.randn(H, d, generator=g, dtype=torch.float64) / d ** 0.5).float()
    b = (0.1 * torch.randn(H, generator=g, dtype=torch.float64)).float()
    gw = (0.5 + torch.rand(H, generator=g, dtype=torch.float64)).float()
    dE = torch.randn(N, H, d, generator=g, dtype=torch.float64).float()          # random: not orthogonal to E
    if scale is not None and not kw.get('just_average'):
        lg = fuse_ref.logits(R.heads_of(planes.double(), H, d, kw.get('split_head', True)), w, torch.zeros(H), kw.get('mul', False),
                             kw.get('l2norm_each_head', False))
        w = (w.double() * (scale / _row_std(lg))).float()
    return planes, w, b, gw, dE


def _row_std(lg):
    """The standard deviation of the logits about their softmax row's mean: what decides how peaked the softmax is."""
    return float((lg - lg.mean(2, keepdim=True)).pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs (fp32, CPU), the float64 autograd reference and the bound of one case: computed once, shared, never written to."""
    N, L, H, d, kw, scale = c
    kw = dict(kw)
    base = 7919 * (N + 31 * L + 57 * H) + d + 13 * sum(1 << i for i, (k, v) in enumerate(sorted(kw.items())) if v)
    for seed in range(base, base + 20):
        planes, w, b, gw, dE = _inputs(N, L, H, d, kw, scale, seed)
        cf = R.closed_form(planes, H, d, w, b, gw, dE, **kw)
        if float(cf['g_norm'].min()) >= 0.05 and float(cf['raw_norm'].min()) >= 0.05:
            break
    # the reference alone stays clear of the 1 / r singularity
    assert float(cf['g_norm'].min()) >= 0.05 and float(cf['raw_norm'].min()) >= 0.05, c
    ref = R.autograd_grads(planes, H, d, w, b, gw, dE, **kw)
    f32 = R.autograd_grads(planes, H, d, w, b, gw, dE, dtype=torch.float32, **kw)
    e32 = (R.rel_err(f32[0], ref[0]), R.rel_err(f32[1], ref[1]))
    assert R.rel_err(cf['dx'], ref[0]) <= 1e-12 and R.rel_err(cf['dw'], ref[1]) <= 1e-12
    top = float(torch.softmax(fuse_ref.logits(R.heads_of(planes.double(), H, d, kw.get('split_head', True)), w, b, kw.get('mul', False),
                                              kw.get('l2norm_each_head', False)), 2).max(2).values.min()) if not kw.get('just_average') else 0.0
    return dict(N=N, L=L, H=H, d=d, kw=kw, planes=planes, w=w, b=b, gw=gw, dE=dE, ref=ref, e32=e32, min_top=top,
                bound=(max(4.0 * e32[0], TOL_UNIT), max(4.0 * e32[1], TOL_UNIT)))


def _flags(kw):
    from laff_amd import ops
    return ops.attention_flags(kw.get('with_ave', False), kw.get('mul', False), kw.get('l2norm_each_head', False),
                               kw.get('split_head', True), kw.get('just_average', False))


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def _launch(cs, planes_dev=None, grad=None, out=None):
    """ops.fuse_backward on the case's inputs; every dx buffer holds NaN before the launch."""
    from laff_amd import ops
    kw, H, d = cs['kw'], cs['H'], cs['d']
    javg = kw.get('just_average', False)
    if planes_dev is None:
        x = cs['planes'].to(DEV)
        planes_dev = [x[:, l, :].contiguous() for l in range(cs['L'])]
    if out is None:
        out = [_nan(*p.shape) for p in planes_dev]
    grad = cs['dE'].to(DEV) if grad is None else grad
    w, b, gw = (None, None, None) if javg else (cs['w'].to(DEV), cs['b'].to(DEV), cs['gw'].to(DEV))
    dxs, dw, db = ops.fuse_backward(planes_dev, H, d, w, b, gw, _flags(kw), grad, out=out)
    torch.cuda.synchronize()
    return dxs, dw, db


def _check(cs, dxs, dw, db, label):
    dx = torch.stack([t.cpu() for t in dxs], 1)
    assert torch.isfinite(dx).all(), label
    e_dx = R.rel_err(dx, cs['ref'][0])
    if cs['kw'].get('just_average'):
        assert dw is None and db is None
        e_dw = 0.0
    else:
        assert tuple(dw.shape) == (cs['H'], cs['d']) and tuple(db.shape) == (cs['H'],)
        assert not db.any(), label                                   # exactly zero
        e_dw = R.rel_err(dw.cpu(), cs['ref'][1])
    print('%-44s fp32 CPU dx %.2e dw %.2e | device dx %.2e (bound %.2e) dw %.2e (bound %.2e) | min top weight %.4f'
          % (label, cs['e32'][0], cs['e32'][1], e_dx, cs['bound'][0], e_dw, cs['bound'][1], cs['min_top']))
    assert e_dx <= cs['bound'][0] and e_dw <= cs['bound'][1], (label, e_dx, cs['bound'][0], e_dw, cs['bound'][1])
    return e_dx, e_dw


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_backward_vs_float64(c):
    cs = _case(c)
    dxs, dw, db = _launch(cs)
    _check(cs, dxs, dw, db, _case_id(c))
    # two launches on the same inputs: the same bits
    dxs2, dw2, _ = _launch(cs)
    assert all(torch.equal(a, b) for a, b in zip(dxs, dxs2))
    assert dw is None or torch.equal(dw, dw2)


def test_multi_row_cases_give_a_wavefront_several_rows():
    """The workspace holds one partial row of dw per (head, row chunk) -- four per chunk in the streaming variant --, so its size tells
    how many rows a block walks: more than four in the cases meant to carry state from row to row."""
    import ctypes as C
    from laff_amd import _lib
    lib, n = _lib.load(), C.c_size_t()
    many = [c for c in CASES if c[0] > 1000]
    assert len(many) == 4
    for N, L, H, d, kw, _ in CASES:
        assert lib.laff_fuse_backward_workspace_bytes(L, N, H, d, _flags(dict(kw)), C.byref(n)) == 0
        if dict(kw)['just_average']:
            continue
        chunks = n.value // (H * d * 4) // (4 if d > 512 else 1)
        rows = -(-N // chunks)
        assert (rows > 4) == (N > 1000), (N, L, H, d, rows)


def test_peaked_cases_are_peaked():
    std3, onehot = (_case(next(c for c in CASES if c[5] == sc)) for sc in (3.0, 12.0))
    for cs, want in ((std3, 3.0), (onehot, 12.0)):
        lg = fuse_ref.logits(R.heads_of(cs['planes'].double(), cs['H'], cs['d']), cs['w'], torch.zeros(cs['H']), True)
        assert abs(_row_std(lg) - want) < 0.05 * want
    a = torch.softmax(fuse_ref.logits(R.heads_of(onehot['planes'].double(), onehot['H'], onehot['d']), onehot['w'], onehot['b'], True), 2)
    assert float(a.max(2).values.median()) > 0.99                   # near one-hot: the typical row gives one plane all but 1 %


@pytest.mark.parametrize('c', [(5, 3, 2, 260, _key(MULTI), None),
                               (5, 3, 3, 516, _key(dict(MULTI, split_head=False)), None)], ids=_case_id)
def test_stacked_planes_and_gradient_in_place(c):
    """The L slices of a stacked (N, L, D) tensor are read with their pitch, and the gradient is written into a stacked tensor."""
    cs = _case(c)
    x = cs['planes'].to(DEV)                                         # (N, L, D) contiguous: slice l has the row pitch L D
    G = _nan(*x.shape)
    planes = [x[:, l, :] for l in range(cs['L'])]
    assert cs['L'] > 1 and planes[1].stride(0) == cs['L'] * x.shape[2] and not planes[1].is_contiguous()
    dxs, dw, db = _launch(cs, planes_dev=planes, out=[G[:, l, :] for l in range(cs['L'])])
    assert torch.isfinite(G).all()                                   # every element of the stacked gradient was written
    _check(cs, [G[:, l, :] for l in range(cs['L'])], dw, db, 'stacked ' + _case_id(c))
    ref_dx, ref_dw, _ = _launch(cs)                                  # the same bits as from dense planes
    assert all(torch.equal(G[:, l, :], ref_dx[l]) for l in range(cs['L'])) and torch.equal(dw, ref_dw)


def test_non_contiguous_grad():
    c = (5, 3, 2, 260, _key(MULTI), None)
    cs = _case(c)
    N, H, d = cs['N'], cs['H'], cs['d']
    ref_dx, ref_dw, _ = _launch(cs)
    wide = _nan(N, H, 2 * d)
    wide[:, :, ::2] = cs['dE'].to(DEV)                                # inner stride 2: made dense by the op
    pitched = _nan(N, H * d + 8)
    pitched[:, :H * d] = cs['dE'].to(DEV).reshape(N, H * d)          # a row pitch: read in place
    for name, g in (('inner stride 2', wide[:, :, ::2]), ('row pitch', pitched[:, :H * d])):
        assert not g.is_contiguous()
        dxs, dw, db = _launch(cs, grad=g)
        _check(cs, dxs, dw, db, name)
        assert all(torch.equal(a, b) for a, b in zip(dxs, ref_dx)) and torch.equal(dw, ref_dw)


def test_no_parameter_gradients_when_not_wanted_and_empty_batch():
    from laff_amd import ops
    cs = _case((5, 3, 2, 260, _key(MULTI), None))
    x = cs['planes'].to(DEV)
    planes = [x[:, l, :].contiguous() for l in range(cs['L'])]
    w, b, gw = cs['w'].to(DEV), cs['b'].to(DEV), cs['gw'].to(DEV)
    full = ops.fuse_backward(planes, 2, 260, w, b, gw, _flags(cs['kw']), cs['dE'].to(DEV))
    dxs, dw, db = ops.fuse_backward(planes, 2, 260, w, b, gw, _flags(cs['kw']), cs['dE'].to(DEV), want_param_grads=False)
    assert dw is None and db is None and all(torch.equal(a, b) for a, b in zip(dxs, full[0]))
    # N = 0: empty gradients, zero parameter gradients, nothing launched
    empty = [torch.empty(0, 520, device=DEV) for _ in range(3)]
    dxs, dw, db = ops.fuse_backward(empty, 2, 260, w, b, gw, _flags(cs['kw']), torch.empty(0, 2, 260, device=DEV))
    assert [tuple(t.shape) for t in dxs] == [(0, 520)] * 3 and not dw.any() and not db.any() and tuple(dw.shape) == (2, 260)


# ---- the modules in training mode ---------------------------------------------------------------------------------------------------
def _f64_module_graph(planes64, heads, with_ave, mul, l2n=False, split=True):
    """E of a (multi-head) block in float64 torch from per-head (weight, bias, gw) float64 leaves."""
    w = torch.stack([h[0].reshape(-1) for h in heads])
    b = torch.cat([h[1].reshape(1) for h in heads])
    gw = torch.cat([h[2].reshape(1) for h in heads])
    N, L, D = planes64.shape
    H = len(heads)
    d = D // H if split else D
    return fuse_ref.attention(R.heads_of(planes64, H, d, split), w, b, gw, with_ave=with_ave, mul=mul, l2norm_each_head=l2n)[0]


def test_attention_1_and_just_average_train():
    from laff_amd.model.Attention import Attention_1, JustAverage
    torch.manual_seed(5)
    N, L, D = 6, 3, 64
    x = (0.5 * torch.randn(N, L, D)).to(DEV).requires_grad_(True)
    dE = torch.randn(N, D)
    m = Attention_1(D, with_ave=True, mul=False).to(DEV).train()
    m.change_raw_global_emb_weight(0.7)
    E = m(x)
    assert E.shape == (N, D) and E.requires_grad and not m.weights.requires_grad and tuple(m.weights.shape) == (N, L)
    E.backward(dE.to(DEV))
    lin = m.embedding_common[0]
    args = (x.detach().cpu(), 1, D, lin.weight.detach().cpu(), lin.bias.detach().cpu(), torch.tensor([0.7]), dE)
    ref = R.autograd_grads(*args, with_ave=True)
    f32 = R.autograd_grads(*args, with_ave=True, dtype=torch.float32)
    E64 = fuse_ref.attention(R.heads_of(args[0].double(), 1, D), args[3], args[4], args[5], with_ave=True)[0]
    assert R.rel_err(E.detach().cpu(), E64.reshape(N, D)) <= TOL_UNIT
    for got, r, r32 in ((x.grad, ref[0], f32[0]), (lin.weight.grad, ref[1], f32[1])):
        assert R.rel_err(got.cpu(), r) <= max(4.0 * R.rel_err(r32, r), TOL_UNIT)
    assert not lin.bias.grad.any() and m.global_emb_weight_net.weight.grad is None
    # fuse_planes over separate planes: the same bits as over the stacked tensor
    ps = [x.detach()[:, l, :].contiguous().requires_grad_(True) for l in range(L)]
    m.zero_grad()
    m.fuse_planes([(p, False, None, None) for p in ps]).backward(dE.to(DEV))
    assert all(torch.equal(p.grad, x.grad[:, l, :]) for l, p in enumerate(ps))
    # a view the kernels cannot read in place (base 4 bytes off a 16-byte boundary, pitch no multiple of 4) is copied, not refused
    wide = torch.zeros(N, L, D + 1, device=DEV)
    wide[:, :, 1:] = x.detach()
    view = wide[:, :, 1:].requires_grad_(True)
    assert view.data_ptr() % 16 and view.stride(1) % 4
    m.zero_grad()
    E2 = m(view)
    E2.backward(dE.to(DEV))
    assert torch.equal(E2, E) and torch.equal(view.grad, x.grad)
    # JustAverage: dx_l = dE / L
    ja = JustAverage().train()
    y = x.detach().clone().requires_grad_(True)
    out = ja(y)
    out.backward(dE.to(DEV))
    assert torch.equal(out, JustAverage().eval()(y.detach()))
    # dE * fl(1 / L): two roundings
    assert R.rel_err(y.grad.cpu(), (dE.double() / L)[:, None, :].expand(N, L, D)) <= 2.0 ** -22


class _Side(torch.nn.Module):
    """One tower of the end-to-end test: L nn.Linear + tanh projections in torch, torch.stack, the fusion block."""

    def __init__(self, dims, D, H):
        super().__init__()
        from laff_amd.model.Attention import Multi_head_MyApply_Attention
        self.proj = torch.nn.ModuleList([torch.nn.Linear(k, D) for k in dims])
        self.att = Multi_head_MyApply_Attention(D, H, D // H, with_ave=True, mul=True)

    def forward(self, feats):
        return self.att(torch.stack([torch.tanh(p(f)) for p, f in zip(self.proj, feats)], 1))


def _side_f64(side, feats, dtype=torch.float64):
    """The same tower as a CPU torch graph in `dtype` with fuse_ref.attention: (E, its leaves by name)."""
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().cpu().to(dtype).requires_grad_(True)
        return leaves[name]
    fs = [leaf('feat%d' % i, f) for i, f in enumerate(feats)]
    planes = torch.stack([torch.tanh(f @ leaf('proj.%d.weight' % i, p.weight).T + leaf('proj.%d.bias' % i, p.bias))
                          for i, (p, f) in enumerate(zip(side.proj, fs))], 1)
    heads = [(leaf('att.attention_layer.%d.embedding_common.0.weight' % h, a.embedding_common[0].weight),
              leaf('att.attention_layer.%d.embedding_common.0.bias' % h, a.embedding_common[0].bias),
              a.global_emb_weight_net.weight.detach().cpu().to(dtype).reshape(1)) for h, a in enumerate(side.att.attention_layer)]
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        E = _f64_module_graph(planes, heads, True, True)
    finally:
        fuse_ref.F64 = keep
    return E, leaves


def test_end_to_end_two_towers_margin_loss():
    """L = 3, H = 2, d = 64, B = 16: Linear + tanh projections -> torch.stack -> Multi_head_MyApply_Attention.train() on each side ->
    loss.MarginRankingLoss -> backward.  Every parameter gradient and both sides' input gradients against the same graph in float64.

    Bound of a gradient tensor T, element by element:  max(4 e32, 1.5e-6) max |T|  +  GRAD_ABS sum_j |dT / dE_j|.
    The first term is the bound of the cases above, e32 being the error of the whole graph in float32 CPU autograd; the second is the
    margin loss's own contract (its d_s / d_im are within GRAD_ABS = 2e-6 of float64, element by element) carried to T through the
    absolute values of the tower's Jacobian, to first order -- T is linear in the loss's gradient."""
    from laff_amd import loss as laff_loss
    B, L, H, d, margin = 16, 3, 2, 64, 0.2
    dims = (24, 16, 8)
    def build():
        txt, vis = _Side(dims, H * d, H), _Side(dims, H * d, H)
        z = torch.randn(B, 8)
        ft = [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims]
        fv = [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims]
        with torch.no_grad():
            return (txt, vis, ft, fv), _side_f64(txt, ft)[0], _side_f64(vis, fv)[0]
    txt, vis, ft, fv = TR.hinge_clear_seed(build, margin, 100)
    # float64 and float32 CPU graphs
    grads = {}
    for dtype in (torch.float64, torch.float32):
        (Et, lt), (Ev, lv) = _side_f64(txt, ft, dtype), _side_f64(vis, fv, dtype)
        TR.margin_loss_f64(Et, Ev, margin).backward()
        grads[dtype] = ({k: v.grad.double() for k, v in lt.items()}, {k: v.grad.double() for k, v in lv.items()}, Et, Ev, lt, lv)
    # sum_j |dT / dE_j| per side, from the float64 graph: one batched backward over the unit vectors of E
    absjac = [TR.abs_jacobian(*_side_f64((txt, vis)[side], (ft, fv)[side])) for side in (0, 1)]
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
                assert not g.any(), n                                                               # db: exactly zero
                continue
            bound, e32, top = TR.end_to_end_bound(r, ref32[n], absjac[side][n])
            err = (g.cpu().double() - r).abs()
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            print('side %d %-52s max |g| %.3e  err %.3e  fp32 CPU %.2e  bound %.3e .. %.3e  worst err / bound %.3f'
                  % (side, n, top, float(err.max()), e32, float(bound.min()), float(bound.max()), ratio))
            assert ratio <= 1.0, (n, ratio)
    # eval afterwards: the code path of today, bit for bit
    from laff_amd import ops
    txt.eval()
    with torch.no_grad():
        stacked = torch.stack([torch.tanh(p(f)) for p, f in zip(txt.proj, dt)], 1)
        got = txt.att(stacked)
        att = txt.att
        w = torch.stack([att.attention_layer[h].embedding_common[0].weight.reshape(-1) for h in range(H)]).contiguous()
        b = torch.cat([att.attention_layer[h].embedding_common[0].bias.reshape(1) for h in range(H)]).contiguous()
        gw = torch.cat([att.attention_layer[h].global_emb_weight_net.weight.reshape(1) for h in range(H)]).contiguous()
        want = ops.fuse([(stacked[:, l, :], False, None, None) for l in range(L)], H, d, w, b, gw, ops.attention_flags(True, True))
    assert not got.requires_grad and torch.equal(got, want) and torch.equal(got, Et.detach())


# MEASURED on the MI355X by test_backward_vs_float64 (and the stacked / non-contiguous tests, last four lines), per case: the error of
# float32 CPU autograd against float64 (i), and the device's error beside the bound it was held to, for dx and for dw.  The float32 CPU
# figures, and with them the bounds above 1.5e-6, depend a little on the CPU that runs them (summation order follows the vector width
# and the thread count); these are from the GPU host.  Largest device error: dx 1.4e-6 and dw 1.6e-6, both in the near one-hot case
# (float32 CPU 7.6e-6 and 9.4e-6, bounds 3.0e-5 and 3.8e-5); outside the peaked cases dx 2.2e-7, dw 3.1e-7.  Closest to its bound: dw at
# (1, 2, 3, 260), 2.6e-7 of 1.5e-6 (0.17 x).  The four cases with several rows per wavefront: dx 1.2e-7 .. 2.2e-7, dw 1.7e-7 .. 2.6e-7.
# End to end: the worst element used 0.10 of its bound.
#   case                                                 fp32 CPU dx, dw      device dx (bound)              device dw (bound)
#   N1-L2-H3-d260-mul+with_ave                           7.97e-08 2.36e-07   1.26e-07 (1.50e-06)            2.59e-07 (1.50e-06)
#   N3-L2-H3-d260-mul+with_ave                           8.90e-08 1.17e-07   1.29e-07 (1.50e-06)            1.38e-07 (1.50e-06)
#   N5-L2-H3-d260-mul+with_ave                           1.64e-07 1.61e-07   1.13e-07 (1.50e-06)            1.40e-07 (1.50e-06)
#   N257-L2-H3-d260-mul+with_ave                         1.44e-07 6.18e-07   1.40e-07 (1.50e-06)            3.07e-07 (2.47e-06)
#   N5-L1-H3-d260-mul+with_ave                           1.06e-07 0.00e+00   1.28e-07 (1.50e-06)            0.00e+00 (1.50e-06)
#   N5-L5-H3-d260-mul+with_ave                           1.57e-07 3.71e-07   1.28e-07 (1.50e-06)            2.19e-07 (1.50e-06)
#   N5-L8-H3-d260-mul+with_ave                           1.37e-07 2.50e-07   1.57e-07 (1.50e-06)            1.78e-07 (1.50e-06)
#   N5-L2-H1-d256-mul+with_ave                           1.33e-07 1.73e-07   6.95e-08 (1.50e-06)            2.07e-07 (1.50e-06)
#   N5-L2-H8-d256-mul+with_ave                           1.75e-07 1.95e-07   1.24e-07 (1.50e-06)            1.90e-07 (1.50e-06)
#   N5-L3-H2-d4-mul+with_ave                             9.41e-08 3.24e-07   7.97e-08 (1.50e-06)            1.28e-07 (1.50e-06)
#   N5-L3-H2-d252-mul+with_ave                           1.10e-07 3.69e-07   1.12e-07 (1.50e-06)            2.16e-07 (1.50e-06)
#   N5-L3-H2-d256-mul+with_ave                           1.10e-07 1.26e-07   1.17e-07 (1.50e-06)            9.42e-08 (1.50e-06)
#   N5-L3-H2-d512-mul+with_ave                           1.68e-07 2.35e-07   1.39e-07 (1.50e-06)            1.47e-07 (1.50e-06)
#   N5-L3-H2-d516-mul+with_ave                           1.32e-07 2.32e-07   1.17e-07 (1.50e-06)            1.62e-07 (1.50e-06)
#   N5-L3-H2-d1024-mul+with_ave                          1.83e-07 3.31e-07   1.32e-07 (1.50e-06)            2.28e-07 (1.50e-06)
#   N6-L3-H2-d516-l2norm_each_head+mul+with_ave          2.09e-07 3.72e-07   2.11e-07 (1.50e-06)            2.01e-07 (1.50e-06)
#   N5-L3-H3-d260-mul+with_ave+nosplit                   9.16e-08 1.98e-07   1.03e-07 (1.50e-06)            1.52e-07 (1.50e-06)
#   N5-L3-H3-d260-l2norm_each_head+mul+with_ave+nosplit  2.08e-07 2.53e-07   2.08e-07 (1.50e-06)            2.20e-07 (1.50e-06)
#   N5-L3-H3-d516-mul+with_ave+nosplit                   1.14e-07 2.41e-07   1.09e-07 (1.50e-06)            1.72e-07 (1.50e-06)
#   N5-L3-H3-d516-l2norm_each_head+mul+with_ave+nosplit  1.22e-07 2.56e-07   1.63e-07 (1.50e-06)            2.46e-07 (1.50e-06)
#   N5-L5-H3-d260-nosplit                                2.08e-07 2.49e-07   1.15e-07 (1.50e-06)            1.95e-07 (1.50e-06)
#   N5-L5-H3-d260-plain                                  2.23e-07 2.85e-07   9.01e-08 (1.50e-06)            1.20e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+nosplit               1.66e-07 2.28e-07   1.64e-07 (1.50e-06)            1.47e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head                       1.88e-07 2.12e-07   1.91e-07 (1.50e-06)            1.71e-07 (1.50e-06)
#   N5-L5-H3-d260-mul+nosplit                            1.39e-07 2.54e-07   1.15e-07 (1.50e-06)            1.61e-07 (1.50e-06)
#   N5-L5-H3-d260-mul                                    1.56e-07 2.02e-07   1.21e-07 (1.50e-06)            1.87e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+mul+nosplit           1.63e-07 2.45e-07   1.22e-07 (1.50e-06)            2.31e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+mul                   1.92e-07 2.13e-07   1.56e-07 (1.50e-06)            1.71e-07 (1.50e-06)
#   N5-L5-H3-d260-with_ave+nosplit                       8.95e-08 1.42e-07   1.12e-07 (1.50e-06)            1.50e-07 (1.50e-06)
#   N5-L5-H3-d260-with_ave                               1.35e-07 2.65e-07   1.24e-07 (1.50e-06)            2.09e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+with_ave+nosplit      1.86e-07 3.02e-07   1.71e-07 (1.50e-06)            2.26e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+with_ave              1.37e-07 1.88e-07   1.73e-07 (1.50e-06)            1.26e-07 (1.50e-06)
#   N5-L5-H3-d260-mul+with_ave+nosplit                   1.03e-07 1.55e-07   1.23e-07 (1.50e-06)            1.82e-07 (1.50e-06)
#   N5-L5-H3-d260-l2norm_each_head+mul+with_ave+nosplit  1.38e-07 4.51e-07   1.92e-07 (1.50e-06)            2.33e-07 (1.81e-06)
#   N5-L5-H3-d260-l2norm_each_head+mul+with_ave          1.37e-07 2.80e-07   1.78e-07 (1.50e-06)            1.84e-07 (1.50e-06)
#   N5-L5-H3-d260-just_average                           3.13e-08 0.00e+00   4.69e-08 (1.50e-06)            0.00e+00 (1.50e-06)
#   N5-L5-H3-d516-just_average+nosplit                   5.48e-08 0.00e+00   9.58e-08 (1.50e-06)            0.00e+00 (1.50e-06)
#   N9-L4-H2-d128-mul+with_ave-std3                      2.47e-06 1.65e-06   2.26e-07 (9.88e-06)            1.98e-07 (6.61e-06)
#   N9-L4-H2-d128-mul+with_ave-std12                     7.61e-06 9.41e-06   1.36e-06 (3.04e-05)            1.58e-06 (3.76e-05)
#   N4100-L2-H8-d4-mul+with_ave                          2.42e-07 1.91e-06   1.23e-07 (1.50e-06)            2.31e-07 (7.63e-06)
#   N2100-L2-H8-d260-l2norm_each_head+mul+with_ave       1.94e-07 1.97e-06   2.16e-07 (1.50e-06)            2.61e-07 (7.90e-06)
#   N2100-L2-H8-d516-mul+with_ave                        2.06e-07 1.39e-06   1.79e-07 (1.50e-06)            1.67e-07 (5.55e-06)
#   N16500-L2-H3-d4-mul+with_ave+nosplit                 1.40e-07 4.07e-06   1.41e-07 (1.50e-06)            2.64e-07 (1.63e-05)
#   stacked N5-L3-H2-d260-mul+with_ave                   1.23e-07 1.96e-07   1.19e-07 (1.50e-06)            1.81e-07 (1.50e-06)
#   stacked N5-L3-H3-d516-mul+with_ave+nosplit           1.14e-07 2.41e-07   1.09e-07 (1.50e-06)            1.72e-07 (1.50e-06)
#   inner stride 2                                       1.23e-07 1.96e-07   1.19e-07 (1.50e-06)            1.81e-07 (1.50e-06)
#   row pitch                                            1.23e-07 1.96e-07   1.19e-07 (1.50e-06)            1.81e-07 (1.50e-06)
