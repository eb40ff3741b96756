"""laff_expert_stage_train, its backward, the ops and _ExpertStageFn on the MI355X, element by element against the
float64 restatement tests/expert_stage_ref.py.  With u = 2^-24, all from float64 values:

    |Y - Y64|        <= (D / 2 + 5) u |Y64|        one rounding for v, at most (D + 2) u on the sum of squares, halved by the root, three
                                                   more operations (the sum with eps, the reciprocal, the product)
    |r - r64|        <= (D / 2 + 3) u r64          the same without v's own rounding and the product
    |dx - dx64|      <= (3 D + 16) u (r |g_i| + |v_i| (r^2 / s) sum_j |v_j g_j|)
    |d_expert - ref| <= (3 D + 16 + N) u sum_n (the same expression)
    without l2norm:  Y is one rounding from the float64 sum (u |Y64|), dx is dY bit for bit, d_expert within N u sum_n |g|

The kernel forms its row sums in its own order (the device function of laff_plane_row_norms is not shared: that kernel walks the heads
of a plane one by one, d columns at a time), so r is compared with laff_plane_row_norms under the (D / 2 + 3) u bound, not bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import expert_stage_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
U = R.U
# (N, L, D); (130, 8, 128) is cut into nine blocks of rows by the plan, (65, 2, 2052) has a one-row last block
CASES = [(1, 1, 4), (2, 3, 36), (63, 3, 512), (64, 8, 512), (65, 2, 2052), (130, 8, 128), (0, 3, 36)]
SWITCHES = [(True, False), (False, True), (True, True)]             # (expert, l2norm)
GUARD = 64


def _id(c):
    return 'N%d-L%d-D%d' % c


def _sw(s):
    return ('expert' if s[0] else '') + ('+' if all(s) else '') + ('l2norm' if s[1] else '')


@functools.lru_cache(maxsize=None)
def _case(c):
    """The fp32 operands of a case on the CPU -- computed once, shared, never written."""
    N, L, D = c
    g = torch.Generator().manual_seed(N * 1000003 + L * 1009 + D)
    xs = [torch.randn(N, D, generator=g) * (0.5 + l) for l in range(L)]
    expert = torch.randn(L, D, generator=g)
    dY = torch.randn(N, L, D, generator=g)
    return dict(xs=xs, expert=expert, dY=dY)


@functools.lru_cache(maxsize=None)
def _ref(c, sw):
    cs = _case(c)
    xs, e = [x.numpy() for x in cs['xs']], cs['expert'].numpy() if sw[0] else None
    Y, r = R.forward(xs, e, sw[1])
    dx, de, mag = R.backward(xs, e, sw[1], cs['dY'].numpy())
    return dict(Y=Y, r=r, dx=dx, de=de, mag=mag)


def _stacked(N, L, D, pitched, fill=None):
    """A NaN-filled device buffer and the (N, L, D) view inside it, GUARD floats in front and behind: dense, or with a plane pitch of
    D + 4 and a row pitch of L (D + 4) + 8.  (buffer, view)."""
    ldl = D + 4 if pitched else D
    ldn = L * ldl + (8 if pitched else 0)
    buf = torch.full((2 * GUARD + max(N, 1) * ldn,), NAN, device=DEV)
    view = torch.as_strided(buf, (N, L, D), (ldn, ldl, 1), GUARD)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _run(c, sw, pitched=True, want_de=True, xs=None):
    """Forward and backward through the ops, every operand and output inside NaN frames; the outputs by name on the CPU after the
    frames were checked."""
    from laff_amd import ops
    cs = _case(c)
    N, L, D = c
    expert, l2norm = sw
    want_de = want_de and expert
    layout = 'pitch4' if pitched else 'dense'
    held = [TR.place(x, layout) for x in (xs or cs['xs'])]
    planes = [v for _, v in held]
    e = None
    if expert:
        held.append(TR.place(cs['expert'], layout))
        e = held[-1][1]
    held.append(_stacked(N, L, D, pitched))
    Y = held[-1][1]
    held.append(_stacked(N, L, D, pitched, cs['dY']))
    dY = held[-1][1]
    dxs = []
    for _ in range(L):
        held.append(TR.pitched(N, D, layout))
        dxs.append(held[-1][1])
    fr = TR.Frames(GUARD)
    rn = fr.floats(L, N) if l2norm and N else (torch.empty((L, N), device=DEV) if l2norm else None)
    de = fr.floats(L, D) if want_de else None
    y2, r2 = ops.expert_stage_train(planes, e, l2norm, out=(Y, rn))
    assert y2.data_ptr() == Y.data_ptr() and (r2 is None) == (not l2norm)
    dx2, de2 = ops.expert_stage_train_backward(dY, planes, e, l2norm, rn, want_d_expert=want_de, out=(dxs, de))
    assert [t.data_ptr() for t in dx2] == [t.data_ptr() for t in dxs] and (de2 is None) == (not want_de)
    torch.cuda.synchronize()
    assert all(TR.untouched_around(buf, view) for buf, view in held) and fr.intact(), 'a write outside a buffer or into the slack of a pitch'
    return dict(Y=Y.cpu(), r=None if rn is None else rn.cpu(), dx=torch.stack([t.cpu() for t in dxs], 1) if L else None,
                de=None if de is None else de.cpu())


def _within(name, got, ref, bound):
    err = np.abs(got.double().numpy() - ref)
    assert np.all(err[bound == 0] == 0), name
    worst = float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
    assert worst <= 1.0, (name, worst)
    return worst


@pytest.mark.parametrize('sw', SWITCHES, ids=_sw)
@pytest.mark.parametrize('c', CASES, ids=_id)
def test_stage_against_float64(c, sw):
    from laff_amd import ops
    N, L, D = c
    chunks, nbytes = ops.expert_stage_train_plan(N, L, D)
    assert chunks == (N + 15) // 16 and nbytes == chunks * L * D * 4
    if c == (130, 8, 128):
        assert chunks > 1
    ref = _ref(c, sw)
    bY, bdx, bde = R.bounds(N, D, sw[1], ref['Y'], ref['mag'])
    for pitched in (True, False):
        out = _run(c, sw, pitched)
        used = {'Y': _within('Y', out['Y'], ref['Y'], bY), 'dx': _within('dx', out['dx'], ref['dx'], bdx)}
        if sw[1]:
            used['r'] = _within('r', out['r'], ref['r'], (D / 2 + 3) * U * ref['r'])
        else:
            assert torch.equal(out['dx'].view(torch.int32), _case(c)['dY'].view(torch.int32)), 'dx must be dY bit for bit'
        if sw[0]:
            used['d_expert'] = _within('d_expert', out['de'], ref['de'], bde)
            if N == 0:
                assert not out['de'].any()                 # N == 0 touches nothing, except d_expert = 0
        print('%s %-14s %s  %s' % (_id(c), _sw(sw), 'pitched' if pitched else 'dense  ',
                                   '  '.join('%s %.3f' % kv for kv in used.items())))


@pytest.mark.parametrize('c', [(2, 3, 36), (65, 2, 2052)], ids=_id)
def test_d_expert_absent_leaves_the_rest_unchanged(c):
    full, without = _run(c, (True, True)), _run(c, (True, True), want_de=False)
    assert without['de'] is None
    assert all(torch.equal(full[k], without[k]) for k in ('Y', 'r', 'dx'))


@pytest.mark.parametrize('c', [(2, 3, 36), (63, 3, 512)], ids=_id)
def test_a_row_of_zeros(c):
    """l2norm on a zero row: finite outputs, Y = 0 there, and every other row carries the bits of the run without that row's zeros."""
    N, L, D = c
    xs = [x.clone() for x in _case(c)['xs']]
    xs[1][N - 1] = 0.0
    zero, plain = _run(c, (False, True), xs=xs), _run(c, (False, True))
    assert all(bool(torch.isfinite(zero[k]).all()) for k in ('Y', 'r', 'dx'))
    assert not zero['Y'][N - 1, 1].any()
    g = _case(c)['dY'][N - 1, 1].double().numpy()
    assert np.all(np.abs(zero['dx'][N - 1, 1].double().numpy() - g / R.EPS) <= 4 * U * np.abs(g) / R.EPS)          # dv = r g: the second term is 0
    keep = torch.ones(N, L, dtype=torch.bool)
    keep[N - 1, 1] = False
    assert torch.equal(zero['Y'][keep], plain['Y'][keep]) and torch.equal(zero['dx'][keep], plain['dx'][keep])
    assert torch.equal(zero['r'].T[keep], plain['r'].T[keep])


def test_a_row_with_a_tiny_norm_stays_finite():
    """A non-zero row of norm 1e-16: r^2 / s is beyond fp32's range, r (r ((v . g) / s)) is not; dx stays within its bound."""
    c = (2, 3, 36)
    N, L, D = c
    xs = [x.clone() for x in _case(c)['xs']]
    xs[1][1] *= 1e-17
    out = _run(c, (False, True), xs=xs)
    dx, _, mag = R.backward([x.numpy() for x in xs], None, True, _case(c)['dY'].numpy())
    assert bool(torch.isfinite(out['dx']).all())
    _within('dx', out['dx'], dx, (3 * D + 16) * U * mag)


@pytest.mark.parametrize('c', [(64, 8, 512), (130, 8, 128)], ids=_id)
def test_two_calls_give_identical_bits(c):
    a, b = _run(c, (True, True)), _run(c, (True, True))
    assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize('c', [(2, 3, 36), (130, 8, 128)], ids=_id)
def test_graph_capture_replays_the_eager_bits(c):
    """A forward plus backward captured on one stream (linear: each launch follows the one before) replays to the eager bits."""
    from laff_amd import ops
    cs = _case(c)
    N, L, D = c
    planes = [x.to(DEV) for x in cs['xs']]
    e, dY = cs['expert'].to(DEV), cs['dY'].to(DEV)

    def buffers():
        return ([torch.full((N, L, D), NAN, device=DEV), torch.full((L, N), NAN, device=DEV)],
                [[torch.full((N, D), NAN, device=DEV) for _ in range(L)], torch.full((L, D), NAN, device=DEV)])

    def step(fw, bw):
        ops.expert_stage_train(planes, e, True, out=tuple(fw))
        ops.expert_stage_train_backward(dY, planes, e, True, fw[1], out=tuple(bw))
    ws_warm = buffers()
    step(*ws_warm)                                         # the workspace allocation happens outside the capture
    eager = buffers()
    step(*eager)
    torch.cuda.synchronize()
    held = buffers()
    nbytes = ops.expert_stage_train_plan(N, L, D)[1]
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    keep = ops._workspace
    gr = torch.cuda.CUDAGraph()
    try:
        ops._workspace = lambda n, dev, floor=0: ws[:n] if n else None       # a workspace that outlives the capture
        with torch.cuda.graph(gr, capture_error_mode='thread_local'):
            step(*held)
    finally:
        ops._workspace = keep
    assert held[0][0].isnan().all()                        # capturing runs nothing
    gr.replay()
    torch.cuda.synchronize()
    flat = lambda b: [b[0][0], b[0][1]] + b[1][0] + [b[1][1]]       # noqa: E731
    assert all(torch.equal(p, q) for p, q in zip(flat(held), flat(eager)))


@pytest.mark.parametrize('sw', SWITCHES, ids=_sw)
def test_function_matches_the_ops_and_feeds_the_expert_table(sw):
    """_ExpertStageFn: the stacked output and every gradient are the ops' bits; the expert nn.Embedding.weight receives d_expert."""
    from laff_amd import ops
    from laff_amd.model.autograd import _ExpertStageFn
    c = (63, 3, 512)
    cs = _case(c)
    N, L, D = c
    planes = [x.to(DEV).requires_grad_(True) for x in cs['xs']]
    emb = torch.nn.Embedding(L + 2, D).to(DEV)             # a table with more rows than planes: the tower hands its first L rows over
    with torch.no_grad():
        emb.weight[:L].copy_(cs['expert'])
    dY = cs['dY'].to(DEV)
    Y = _ExpertStageFn.apply(sw[1], emb.weight[:L] if sw[0] else None, *planes)
    assert Y.shape == (N, L, D) and Y.requires_grad
    Y.backward(dY)
    want_Y, rn = ops.expert_stage_train([p.detach() for p in planes], emb.weight.detach()[:L] if sw[0] else None, sw[1])
    dxs, de = ops.expert_stage_train_backward(dY, [p.detach() for p in planes], emb.weight.detach()[:L] if sw[0] else None, sw[1], rn,
                                              want_d_expert=sw[0])
    torch.cuda.synchronize()
    assert torch.equal(Y.detach(), want_Y) and all(torch.equal(p.grad, d) for p, d in zip(planes, dxs))
    if sw[0]:
        assert torch.equal(emb.weight.grad[:L], de) and not emb.weight.grad[L:].any()
    else:
        assert emb.weight.grad is None
    # no gradient asked of the table: no d_expert is formed
    if sw[0]:
        calls = []
        keep = ops.expert_stage_train_backward
        try:
            ops.expert_stage_train_backward = lambda *a, **k: (calls.append(k), keep(*a, **k))[1]
            _ExpertStageFn.apply(sw[1], emb.weight.detach()[:L], *planes).backward(dY)
        finally:
            ops.expert_stage_train_backward = keep
        assert calls and calls[0]['want_d_expert'] is False


def test_row_norms_agree_with_laff_plane_row_norms():
    """The stage's r against laff_plane_row_norms' value for the same rows (the expert row as the plane's shift under a unit scale), both
    under the (D / 2 + 3) u bound: the device function is not shared -- that kernel walks a plane head by head, d columns at a time, so
    its partial sums are laid out by (H, d), which the stage does not know -- and the bits may differ in the last place."""
    import ctypes as C

    from laff_amd import _lib, ops
    c = (63, 3, 512)
    cs = _case(c)
    N, L, D = c
    H = 4
    planes = [x.to(DEV) for x in cs['xs']]
    e = cs['expert'].to(DEV)
    _, r = ops.expert_stage_train(planes, e, True)
    ones = torch.ones(D, device=DEV)
    arr = (_lib.Plane * L)()
    for l in range(L):
        arr[l] = _lib.Plane(planes[l].data_ptr(), D, 0, ones.data_ptr(), e[l].data_ptr(), _lib.ACT[None], None, None, None, None, 0, 0, None)
    norms = torch.empty((L, N), device=DEV)
    lib, h = ops._context(planes[0].device)
    _lib.check(lib.laff_plane_row_norms(h, arr, L, N, H, D // H, ops.attention_flags(just_average=True), C.c_void_p(norms.data_ptr())))
    torch.cuda.synchronize()
    r64 = _ref(c, (True, True))['r']
    bound = (D / 2 + 3) * U * r64
    assert np.all(np.abs(r.cpu().double().numpy() - r64) <= bound) and np.all(np.abs(norms.cpu().double().numpy() - r64) <= bound)
    same = float((r == norms).float().mean())
    print('r against laff_plane_row_norms: %.1f %% of the rows carry equal bits' % (100 * same))
