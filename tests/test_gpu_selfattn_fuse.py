"""laff_selfattn_fuse / laff_selfattn_fuse_backward (laff_amd/csrc/selfattn_fuse.hip) and the module built on them against the float64
restatement tests/selfattn_ref.py: forward and every gradient, every output type, with and without l2norm_each_head.

Error rule (that of tests/test_gpu_fuse_backward.py): selfattn_ref.rel_err against float64, limit max(4 e32, 1.5e-6), e32 being the error
of the restatement's float32 CPU run on the same case.  For 'max' and 'max_embedding' the GRADIENT comparison leaves out the groups
(n, h) that hold an element whose two largest candidates lie within 1e-5 max |o| of each other in float64 (a float32 run may route that
element's gradient to the other one); at most 5 % of a case's groups may be left out, which is asserted on the CPU when the case is
built (inputs come from the first seed of the case's fixed range that stays under the cap, found on the CPU: no case is skipped).
A group is left out by giving it a zero incoming gradient, on the device and in the reference alike: it then adds nothing to dx, dgamma
or dbeta, and all of them are compared in every case.  The forward is compared everywhere.
A token of zeros under l2norm_each_head has no gradient in the reference either (0 / 0): there the forward alone is compared.

MEASURED: test_kernel_vs_float64 prints, per case, the float32 CPU error and the device error of every output; the table at the end of
this file is from an MI355X.
"""
import functools

import pytest
import torch

import selfattn_ref as R

pytestmark = pytest.mark.gpu

TYPES = tuple(t for t in R.OUTPUT_TYPES if t != 'random')
# N in {1, 5, 67}: one block, a ragged last block, 17 blocks = partial rows of dgamma | dbeta; L in {1, 2, 4, 8} (T = 9 under the prepending
# types) and 3; H in {1, 2, 8}; d in {4, 36, 64, 260, 512}: 36 and 260 are a lane tail and one chunk plus a tail; d = H = 8: s = 1.
SHAPES = [(1, 1, 1, 4), (5, 2, 2, 36), (67, 4, 1, 64), (5, 8, 2, 260), (5, 4, 8, 512), (5, 3, 8, 8)]
CASES = [(s, t, l2n, 'normal') for s in SHAPES for t in TYPES for l2n in (False, True)]
# several groups per wavefront: a block takes more than four groups only once N H / 4 exceeds 4096 blocks
CASES += [((2100, 2, 8, 8), t, l2n, 'normal') for t, l2n in (('mean', False), ('max_embedding', True), ('Attention_1', False))]
# token rows nearly parallel at large norm: logits of standard deviation 3 in a row, a peaked softmax
CASES += [((9, 4, 2, 128), t, l2n, 'peaked') for t in ('mean', 'last', 'mean_embedding', 'Attention_1') for l2n in (False, True)]
# ('max' is not among them: the outputs of nearly parallel tokens are nearly equal, so most groups hold a near tie)
# a token of zeros: l2norm's eps, and at L = 1 a constant residual row, LayerNorm's var = 0
CASES += [((5, L, 2, 36), t, l2n, 'zero') for L in (1, 3) for t in ('mean', 'max', 'first') for l2n in (False, True)]
TOL_FLOOR = 1.5e-6


def _case_id(c):
    (N, L, H, d), t, l2n, kind = c
    return 'N%d-L%d-H%d-d%d-%s%s%s' % (N, L, H, d, t, '-l2n' if l2n else '', '' if kind == 'normal' else '-' + kind)


def _row_std(planes, H, d, t, l2n):
    """The standard deviation of the logits about their softmax row's mean (float64)."""
    N, L = planes.shape[:2]
    x = planes.double().reshape(N, L, H, d).permute(0, 2, 1, 3)
    if l2n:
        x = x / (x.pow(2).sum(3, keepdim=True).sqrt() + R.NORM_EPS)
    z = (d // H) ** -0.5 * torch.einsum('nhid,nhjd->nhij', x, x)
    return float((z - z.mean(3, keepdim=True)).pow(2).mean().sqrt())


def _stacked_run(x, H, d, gamma, beta, l2n, dO, dtype):
    """'Attention_1' at the kernel's level: the stacked tokens (N, L, H d) and the gradients of sum(O * dO)."""
    P, g, b = R._t(x, dtype).requires_grad_(True), R._t(gamma, dtype).requires_grad_(True), R._t(beta, dtype).requires_grad_(True)
    with torch.enable_grad():
        o, _ = R.tokens_out(P, H, d, g, b, 'Attention_1', l2n)
        O = o.permute(0, 2, 1, 3).reshape(P.shape)
        (O * R._t(dO, dtype)).sum().backward()
    return {'E': O.detach().double(), 'dx': P.grad.double(), 'dgamma': g.grad.double(), 'dbeta': b.grad.double()}


def _inputs(N, L, H, d, t, l2n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, L, H * d, generator=g)
    if kind == 'peaked':
        u = torch.randn(N, 1, H * d, generator=g)
        if l2n:                                      # unit tokens: the logits lie in [-s, s]; as peaked as they get is what is asked
            x = u * torch.randn(N, L, 1, generator=g).sign() + 0.3 * x
        else:
            x = u * (1.0 + 0.5 * torch.randn(N, L, 1, generator=g)) + 0.05 * x
            x = x * (3.0 / _row_std(x, H, d, t, l2n)) ** 0.5
    if kind == 'zero':
        x[0] = 0.0 if L == 1 else x[0]
        x[1, 0] = 0.0
        x[2, L - 1, :d] = 0.0
    return x, 0.5 + torch.rand(d, generator=g), 0.3 * torch.randn(d, generator=g), g


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs (fp32, CPU), the float64 reference, the float32 CPU errors and the groups left out: computed once, shared, never written."""
    (N, L, H, d), t, l2n, kind = c
    base = 7919 * (N + 31 * L + 57 * H) + d + 13 * TYPES.index(t) + l2n
    for seed in range(base, base + 20):              # the first seed of the case's range that keeps the groups near a tie under 5 %
        x, gamma, beta, g = _inputs(N, L, H, d, t, l2n, kind, seed)
        out = R.max_gap_groups(x, H, d, gamma, beta, t, l2n)
        if int(out.sum()) <= 0.05 * N * H:
            break
    assert int(out.sum()) <= 0.05 * N * H, 'more than 5 %% of the groups are near a tie: %d of %d' % (int(out.sum()), N * H)
    stacked = t == 'Attention_1'
    dE = torch.randn((N, L, H * d) if stacked else (N, H, d), generator=g)
    if bool(out.any()):                              # the groups left out get no incoming gradient: they add nothing to dx, dgamma, dbeta
        dE[out] = 0.0
    if kind == 'peaked' and not l2n:                 # the inputs are what the case says: logits of standard deviation 3, a peaked softmax
        assert abs(_row_std(x, H, d, t, l2n) - 3.0) < 0.15
        assert float(R.tokens_out(x.double(), H, d, gamma.double(), beta.double(), t, l2n)[1].max(3).values.median()) > 0.6
    if stacked:
        ref, f32 = (_stacked_run(x, H, d, gamma, beta, l2n, dE, dt) for dt in (torch.float64, torch.float32))
    else:
        ref, f32 = (R.run(x, H, d, gamma, beta, t, l2n, None, dE, dt) for dt in (torch.float64, torch.float32))
    grads = not (kind == 'zero' and l2n)
    if grads:
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ref if ref[k] is not None)
    names = ('E', 'dx', 'dgamma', 'dbeta') if grads else ('E',)
    e32 = {k: R.rel_err(f32[k], ref[k]) for k in names}
    return dict(x=x, gamma=gamma, beta=beta, dE=dE, ref=ref, e32=e32, names=names, H=H, d=d, t=t, l2n=l2n)


def _device(cs, x=None, want=True):
    from laff_amd import ops
    x = cs['x'].cuda() if x is None else x
    planes = [x[:, l, :] for l in range(x.shape[1])]
    gamma, beta = cs['gamma'].cuda(), cs['beta'].cuda()
    E = ops.selfattn_fuse(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'])
    dxs, dg, db = ops.selfattn_fuse_backward(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'], cs['dE'].cuda(),
                                             want_param_grads=want)
    return {'E': E, 'dx': torch.stack(dxs, 1), 'dgamma': dg, 'dbeta': db}


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_kernel_vs_float64(c):
    cs = _case(c)
    got = _device(cs)
    figures = {}
    for k in cs['names']:
        g, r = got[k].cpu().double().reshape(cs['ref'][k].shape), cs['ref'][k]
        figures[k] = (cs['e32'][k], R.rel_err(g, r), max(4 * cs['e32'][k], TOL_FLOOR))
    print('%-44s %s' % (_case_id(c), '  '.join('%s %.2e %.2e (%.2e)' % ((k,) + v) for k, v in figures.items())))
    for k, (e32, err, lim) in figures.items():
        assert err <= lim, (k, err, lim)


def test_random_in_eval_is_the_mean():
    cs = _case(((5, 2, 2, 36), 'mean', False, 'normal'))
    assert torch.equal(_device(dict(cs, t='random'))['E'], _device(cs)['E'])


# ---- layout and plumbing ----------------------------------------------------------------------------------------------------------
PLUMB = ((5, 4, 8, 512), 'max_embedding', True, 'normal')


def test_pitched_stacked_input_is_read_in_place_and_its_gradient_written_in_place():
    from laff_amd import ops
    cs = _case(PLUMB)
    N, L, D = cs['x'].shape
    big = torch.full((N, L + 1, D + 8), 7.0, device='cuda')
    big[:, :L, :D] = cs['x'].cuda()
    x = big[:, :L, :D]
    planes = [x[:, l, :] for l in range(L)]
    seen = []
    real = ops._plane_arrays

    def spy(ts, name, n, dd):
        res = real(ts, name, n, dd)
        seen.append((name, [a.data_ptr() for a in res[0]]))
        return res
    ops._plane_arrays = spy
    try:
        gbig = torch.full((N, L + 1, D + 8), 7.0, device='cuda')
        out = [gbig[:, l, :D] for l in range(L)]
        gamma, beta = cs['gamma'].cuda(), cs['beta'].cuda()
        E = ops.selfattn_fuse(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'])
        dxs, dg, db = ops.selfattn_fuse_backward(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'], cs['dE'].cuda(), out=out)
    finally:
        ops._plane_arrays = real
    assert all(ptrs == [p.data_ptr() for p in planes] for nm, ptrs in seen if nm == 'planes') and len(seen) == 3   # no copies
    dense = _device(cs)
    assert torch.equal(E, dense['E']) and torch.equal(gbig[:, :L, :D], dense['dx']) and torch.equal(dg, dense['dgamma'])
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(dxs, out))
    assert bool((gbig[:, L] == 7.0).all()) and bool((gbig[:, :, D:] == 7.0).all())                  # nothing beyond the views


def test_misaligned_view_is_copied_not_refused():
    cs = _case(PLUMB)
    N, L, D = cs['x'].shape
    big = torch.zeros((N, L, D + 4), device='cuda')
    big[:, :, 1:D + 1] = cs['x'].cuda()
    got, dense = _device(cs, big[:, :, 1:D + 1]), _device(cs)
    assert all(torch.equal(got[k], dense[k]) for k in dense)


def test_non_contiguous_dE_and_two_runs_give_equal_bits():
    from laff_amd import ops
    cs = _case(PLUMB)
    x = cs['x'].cuda()
    planes = [x[:, l, :] for l in range(x.shape[1])]
    gamma, beta = cs['gamma'].cuda(), cs['beta'].cuda()
    dE = cs['dE'].cuda()
    dEt = dE.reshape(dE.shape[0], -1).t().contiguous().t()                                        # column-major: copied by the wrapper
    assert not dEt.is_contiguous()
    a = ops.selfattn_fuse_backward(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'], dE)
    b = ops.selfattn_fuse_backward(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'], dEt)
    for p, q in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert torch.equal(p, q)
    big = _case(((67, 4, 1, 64), 'max', False, 'normal'))                                          # 17 partial rows
    r1, r2 = _device(big), _device(big)
    assert all(torch.equal(r1[k], r2[k]) for k in r1)


def test_no_workspace_when_parameter_gradients_are_not_wanted():
    from laff_amd import ops
    cs = _case(PLUMB)
    asked = []
    real = ops._workspace

    def spy(nbytes, device, floor=0):
        asked.append(nbytes)
        return real(nbytes, device, floor)
    ops._workspace = spy
    try:
        got = _device(cs, want=False)
        assert asked == [0] and got['dgamma'] is None and got['dbeta'] is None
        want = _device(cs)
        assert asked[1] == ops.selfattn_fuse_backward_plan(5, 8, 512)[0] > 0
    finally:
        ops._workspace = real
    assert torch.equal(got['dx'], want['dx'])


@pytest.mark.parametrize('t', ['mean', 'Attention_1'])
def test_empty_input(t):
    from laff_amd import ops
    H, d, L = 2, 36, 3
    planes = [torch.zeros((0, H * d), device='cuda') for _ in range(L)]
    gamma, beta = torch.ones(d, device='cuda'), torch.zeros(d, device='cuda')
    E = ops.selfattn_fuse(planes, H, d, gamma, beta, t)
    assert tuple(E.shape) == ((0, L, H * d) if t == 'Attention_1' else (0, H, d))
    dxs, dg, db = ops.selfattn_fuse_backward(planes, H, d, gamma, beta, t, False, torch.zeros_like(E))
    assert [tuple(x.shape) for x in dxs] == [(0, H * d)] * L
    assert tuple(dg.shape) == (d,) and not bool(dg.any()) and not bool(db.any())


def test_graph_replay_equals_eager():
    from laff_amd import ops
    cs = _case(((67, 4, 1, 64), 'mean_embedding', True, 'normal'))
    eager = _device(cs)                                                                            # also the warm-up
    x = cs['x'].cuda()
    planes = [x[:, l, :] for l in range(x.shape[1])]
    gamma, beta, dE = cs['gamma'].cuda(), cs['beta'].cuda(), cs['dE'].cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E = ops.selfattn_fuse(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'])
        dxs, dg, db = ops.selfattn_fuse_backward(planes, cs['H'], cs['d'], gamma, beta, cs['t'], cs['l2n'], dE)
    for t in [E, dg, db] + dxs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(E, eager['E']) and torch.equal(torch.stack(dxs, 1), eager['dx'])
    assert torch.equal(dg, eager['dgamma']) and torch.equal(db, eager['dbeta'])


# ---- the module ---------------------------------------------------------------------------------------------------------------------
def _module(case, training):
    from laff_amd.config import config
    from laff_amd.model.Attention import Multi_head_MyApply_selfAttention
    N, L, H, d = case['shape']
    opt = config()
    a1 = case['att1']
    opt.attention_param_each_head = {'with_ave': bool(a1 and a1['with_ave']), 'mul': bool(a1 and a1['mul']), 'split_head': True}
    m = Multi_head_MyApply_selfAttention(H * d, H, d, 0.0, output_type=case['type'], encoder_num=L, l2norm_each_head=case['l2n'], opt=opt)
    with torch.no_grad():
        m.layer_norm.weight.copy_(torch.from_numpy(case['gamma']))
        m.layer_norm.bias.copy_(torch.from_numpy(case['beta']))
        if a1:
            for h, a in enumerate(m.Attention_list):
                a.embedding_common[0].weight.copy_(torch.from_numpy(a1['w'][h:h + 1]))
                a.embedding_common[0].bias.copy_(torch.from_numpy(a1['b'][h:h + 1]))
                a.change_raw_global_emb_weight(float(a1['gw'][h]))
    return m.cuda().train(training)


# ('random' has no training mode)
FIXTURE = [(i, c) for i, c in R.fixture_cases() if c['type'] != 'random']


@pytest.mark.parametrize('case', [c for _, c in FIXTURE], ids=[i for i, _ in FIXTURE])
def test_module_train_gradients_against_the_fixture(case):
    """The reference's own class (float64, CPU) is the yardstick here; e32 is the reference's own float32 run, stored with the fixture."""
    m = _module(case, True)
    x = torch.from_numpy(case['x']).cuda().requires_grad_(True)
    E = m(x)
    (E * torch.from_numpy(case['dE']).cuda()).sum().backward()
    got = {'E': E, 'dx': x.grad, 'dgamma': m.layer_norm.weight.grad, 'dbeta': m.layer_norm.bias.grad}
    if case['att1']:
        got['dw'] = torch.cat([a.embedding_common[0].weight.grad for a in m.Attention_list])
        got['weights'] = m.get_attention_weight()
    for k, v in got.items():
        err, lim = R.rel_err(v, case[k]), max(4 * case['e32'][k], TOL_FLOOR)
        print('%-12s e32 %.2e device %.2e (%.2e)' % (k, case['e32'][k], err, lim))
        assert err <= lim, (k, err, lim)
    if case['att1']:
        db = torch.cat([a.embedding_common[0].bias.grad for a in m.Attention_list])
        assert not bool(db.any())                                  # exactly zero: a softmax does not see a shift of its logits
    # ... and after .eval() the forward gives the training forward's bits
    assert torch.equal(m.eval()(x.detach()), E.detach())


def test_attention_1_weights_equal_the_restatement():
    case = next(c for i, c in FIXTURE if c['type'] == 'Attention_1' and c['l2n'] and c['shape'][1] == 8)
    N, L, H, d = case['shape']
    m = _module(case, False)
    m(torch.from_numpy(case['x']).cuda())
    ref = R.run(case['x'], H, d, case['gamma'], case['beta'], 'Attention_1', True, case['att1'])
    assert R.rel_err(m.get_attention_weight(), ref['weights']) <= TOL_FLOOR
    with pytest.raises(Exception, match='not applied'):
        _module(dict(case, type='mean', att1=None), False).get_attention_weight()


def test_eval_forward_equals_fuse_planes_on_written_out_planes():
    """A tiled plane, a folded affine and a deferred activation, written out by hand; the expert row rides in `shift`, l2norm_planes
    divides every row by its norm over all H d columns -- and the training route through _ExpertStageFn gives the same."""
    from laff_amd.model.autograd import _ExpertStageFn
    case = next(c for i, c in FIXTURE if c['type'] == 'mean' and not c['l2n'] and c['shape'] == (5, 3, 2, 8))
    N, L, H, d = case['shape']
    D = H * d
    g = torch.Generator().manual_seed(5)
    src = [torch.randn(N, d, generator=g).cuda(), torch.randn(N, D, generator=g).cuda(), torch.randn(N, D, generator=g).cuda()]
    scale, shift = (0.5 + torch.rand(D, generator=g)).cuda(), torch.randn(D, generator=g).cuda()
    planes = [(src[0], True, None, None), (src[1], False, scale, shift), (src[2], False, None, None, 'tanh')]
    hand = torch.stack([src[0].repeat(1, H), src[1] * scale + shift, torch.tanh(src[2])], 1)
    m = _module(case, False)
    got, want = m.fuse_planes(planes, H), m(hand)
    assert tuple(got.shape) == (N, H, d) and R.rel_err(got, want) <= TOL_FLOOR
    normed = hand / (hand.pow(2).sum(2, keepdim=True).sqrt() + 1e-13 + 1e-14)
    assert R.rel_err(m.fuse_planes(planes, H, l2norm_planes=True), m(normed)) <= TOL_FLOOR
    # expert rows + l2norm: eval (the row rides in the descriptor) against the training route (the expert stage, one launch)
    expert = torch.randn(L, D, generator=g).cuda()
    dense = [hand[:, l, :].contiguous() for l in range(L)]
    ones = torch.ones(D, device='cuda')                                     # (a descriptor's scale and shift come together)
    ev = m.fuse_planes([(dense[l], False, ones, expert[l]) for l in range(L)], H, l2norm_planes=True)
    tr = m.train()(_ExpertStageFn.apply(True, expert, *dense))
    assert R.rel_err(tr, ev) <= TOL_FLOOR


# ---- MEASURED on an MI355X (132 kernel cases; per output the largest device error, where it occurred, the float32 CPU error of that
# case and its bound).  Outside the peaked cases every output stayed under 2.3e-7 against the floor bound of 1.5e-6.  The module tests
# against the fixture (L > 1): largest 6.3e-7 (dw, bound 1.7e-6).
#   E        4.75e-07 at N5-L4-H8-d512-mean_embedding                 float32 CPU 8.43e-07  bound 3.37e-06
#   dx       5.55e-07 at N5-L4-H8-d512-mean_embedding                 float32 CPU 8.53e-07  bound 3.41e-06
#   dgamma   3.49e-07 at N1-L1-H1-d4-mean-l2n                         float32 CPU 4.63e-07  bound 1.85e-06
#   dbeta    2.62e-07 at N2100-L2-H8-d8-Attention_1                   float32 CPU 1.92e-07  bound 1.50e-06
