"""Dual-softmax and margin criteria, the part that needs no GPU: the C ABI's declarations, exports, bindings and argument checks, the
float64 restatement (tests/loss_ref.py) against the golden vectors, central differences and float64 autograd, the inputs and the
derived gradient bound of the embedding margin test (tests/test_gpu_losses.py), and the routing of loss.criterion_for."""
import ctypes as C
import types

import numpy as np
import pytest

import loss_ref

NEW_SYMBOLS = ('laff_dsl_loss_workspace_bytes', 'laff_dsl_loss', 'laff_margin_loss_scores')
F64_NOISE = 1e-12          # float64 rounding of the restatement itself (a BLAS that sums in another order), far below any e_ref > 0


# ------------------------------------------------------------------------------------------------ C ABI
# (the three entry points in the header, the library and the binding: test_cabi.py, ENTRY_POINTS)
def test_argument_errors_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)                          # never dereferenced: every call below ends in its checks
    n = C.c_size_t()

    assert lib.laff_dsl_loss_workspace_bytes(17, 2, 36, C.byref(n)) == 0 and n.value > 4 * (3 * 2 * 17 * 20 + 4 * 2 * 17 * 36)
    need = n.value
    assert lib.laff_dsl_loss_workspace_bytes(0, 2, 36, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_dsl_loss_workspace_bytes(-1, 2, 36, C.byref(n)) == -1
    assert lib.laff_dsl_loss_workspace_bytes(17, 0, 36, C.byref(n)) == -1
    assert lib.laff_dsl_loss_workspace_bytes(17, 2, 36, None) == -1

    def dsl(ctx=fake, s=fake, im=fake, B=17, H=2, d=36, temp=1000.0, loss=fake, ws=fake, nbytes=need):
        return lib.laff_dsl_loss(ctx, s, im, B, H, d, temp, loss, None, None, ws, nbytes)

    assert dsl(ctx=None) == -1 and b'null ctx' in lib.laff_last_error()
    assert dsl(B=-1) == -2 and b'bad shape' in lib.laff_last_error()
    assert dsl(H=0) == -2 and dsl(d=0) == -2 and dsl(B=16385) == -2
    assert dsl(B=8189, nbytes=1 << 40) == -5 and b'LDS budget' in lib.laff_last_error()      # the margin loss's own limit
    assert dsl(temp=0.0) == -1 and dsl(temp=-1.0) == -1 and dsl(temp=float('nan')) == -1
    assert dsl(s=None) == -1 and dsl(im=None) == -1 and dsl(loss=None) == -1
    assert dsl(nbytes=need - 1) == -1 and b'workspace too small' in lib.laff_last_error()
    assert dsl(ws=None) == -1 and b'workspace too small' in lib.laff_last_error()
    assert dsl(ws=C.c_void_p(4100)) == -3
    assert dsl(B=0, s=None, im=None, loss=None, ws=None, nbytes=0) == 0                      # the empty batch touches nothing

    def msc(ctx=fake, score=fake, ld=9, B=9, flags=4, loss=fake):
        return lib.laff_margin_loss_scores(ctx, score, ld, B, 0.2, flags, loss, None)

    assert msc(ctx=None) == -1 and b'null ctx' in lib.laff_last_error()
    assert msc(B=-1) == -2 and b'bad shape' in lib.laff_last_error()
    assert msc(ld=8) == -2 and msc(B=16385, ld=16385) == -2 and msc(B=8189, ld=8189) == -5
    assert msc(flags=16) == -1 and b'unknown flags' in lib.laff_last_error()
    assert msc(score=None) == -1 and msc(loss=None) == -1
    assert msc(B=0, ld=0, score=None, loss=None) == 0


# ------------------------------------------------------------------------------------------------ float64 restatement
def test_restatement_reproduces_the_dsl_golden_cases(golden):
    g = golden('dsl_loss')
    cases = g.json('cases')
    assert [tuple(c['shape']) for c in cases] == [(1, 8)] * 2 + [(2, 5)] * 2 + [(3, 7)] * 2 + [(17, 36)] * 2 + [(5, 3, 12)]
    assert [c['temp'] for c in cases] == [1000, 0.05] * 4 + [1000]
    for c in cases:
        k = c['key']
        loss, d_s, d_im = loss_ref.dsl(g[k + '/s'], g[k + '/im'], c['temp'])
        e_loss, e_grad = g[k + '/e_ref']
        ref = float(g[k + '/loss'])
        assert abs(ref - loss) / max(1.0, abs(loss)) <= e_loss + F64_NOISE, c
        assert max(np.abs(g[k + '/d_s'] - d_s).max(), np.abs(g[k + '/d_im'] - d_im).max()) <= e_grad + F64_NOISE, c
        assert e_loss <= 2e-5 and e_grad <= 2e-6, c          # the reference's own fp32 noise sits inside the project's loss bounds
    # a single pair: the loss is exactly 0 and so are the gradients
    loss, d_s, d_im = loss_ref.dsl(g['c0/s'], g['c0/im'], 1000)
    assert loss == 0.0 and not d_s.any() and not d_im.any()


def test_restatement_reproduces_the_margin_score_golden_cases(golden):
    g = golden('margin_scores')
    cases = g.json('cases')
    assert sorted({c['B'] for c in cases}) == [1, 2, 9]
    assert {(c['max_violation'], c['cost_style']) for c in cases} == {(a, b) for a in (False, True) for b in ('sum', 'mean')}
    assert {c['direction'] for c in cases} == {'i2t', 't2i', 'bidir'}
    for c in cases:
        k = c['key']
        sc = g[k + '/score']
        assert loss_ref.margin_scores_slack(sc, c['margin'], c['max_violation'], c['direction']) >= 1e-4, c
        loss, d = loss_ref.margin_scores(sc, c['margin'], c['max_violation'], c['cost_style'], c['direction'])
        e_loss, e_grad = g[k + '/e_ref']
        assert abs(float(g[k + '/loss']) - loss) / max(1.0, abs(loss)) <= e_loss + F64_NOISE, c
        assert np.abs(g[k + '/d_score'] - d).max() <= e_grad + F64_NOISE, c


@pytest.mark.parametrize('shape,temp', [((2, 5), 1000), ((3, 7), 0.05), ((6, 4), 1.0), ((5, 3, 6), 1000), ((4, 2, 5), 0.05)])
def test_dsl_analytic_gradient_matches_central_differences(shape, temp):
    """Step and bound of test_properties.py's margin-loss check: eps 1e-6, 2e-3 relative to max(1, |numeric|)."""
    g = np.random.default_rng(sum(shape) + int(temp))
    s, im = g.normal(0, 1, shape), g.normal(0, 1, shape)
    _, d_s, d_im = loss_ref.dsl(s, im, temp)
    eps = 1e-6
    for _ in range(8):
        idx = tuple(int(g.integers(0, n)) for n in shape)
        for which, grad in ((0, d_s), (1, d_im)):
            a, b = (s, im)[which].copy(), (s, im)[which].copy()
            a[idx] += eps
            b[idx] -= eps
            hi = loss_ref.dsl(a, im, temp)[0] if which == 0 else loss_ref.dsl(s, a, temp)[0]
            lo = loss_ref.dsl(b, im, temp)[0] if which == 0 else loss_ref.dsl(s, b, temp)[0]
            num = (hi - lo) / (2 * eps)
            assert abs(num - grad[idx]) <= 2e-3 * max(1.0, abs(num)), (idx, which, num, grad[idx])


@pytest.mark.parametrize('B', [2, 5, 9])
@pytest.mark.parametrize('maxv', [False, True])
@pytest.mark.parametrize('style,direction', [('sum', 'bidir'), ('mean', 'i2t'), ('sum', 't2i')])
def test_margin_scores_analytic_gradient_matches_central_differences(B, maxv, style, direction):
    g = np.random.default_rng(B * 8 + maxv)
    for _ in range(100):
        sc = 0.6 * np.eye(B) + g.uniform(-0.5, 0.5, (B, B))
        if loss_ref.margin_scores_slack(sc, 0.2, maxv, direction) >= 1e-4:        # no kink inside +-eps
            break
    else:
        pytest.fail('no draw with every decision 1e-4 clear')
    _, d = loss_ref.margin_scores(sc, 0.2, maxv, style, direction)
    eps = 1e-6
    for i in range(B):
        for j in range(B):
            a, b = sc.copy(), sc.copy()
            a[i, j] += eps
            b[i, j] -= eps
            num = (loss_ref.margin_scores(a, 0.2, maxv, style, direction)[0] - loss_ref.margin_scores(b, 0.2, maxv, style, direction)[0]) / (2 * eps)
            assert abs(num - d[i, j]) <= 2e-3 * max(1.0, abs(num)), (i, j, num, d[i, j])


# ------------------------------------------------------------------------------------------------ margin loss from embeddings
from test_gpu_losses import FLAGS, MARGIN, MARGIN_SHAPES, MIN_ACTIVE, _margin_inputs, margin_active_share, margin_scores64  # noqa: E402


def _autograd64(s, im, margin, maxv, style, direction):
    """The reference's formula per head on torch float64 autograd: l2norm, mm, hinge, optional max, sum or mean."""
    import torch
    s = torch.tensor(np.asarray(s, np.float64).reshape(len(s), -1, s.shape[-1]), requires_grad=True)
    im = torch.tensor(np.asarray(im, np.float64).reshape(len(im), -1, im.shape[-1]), requires_grad=True)

    def l2norm(x):
        return x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-13 + 1e-14)

    total = 0
    for h in range(s.shape[1]):
        scores = l2norm(im[:, h]).mm(l2norm(s[:, h]).t())
        dg = scores.diag().view(-1, 1)
        eye = torch.eye(len(scores), dtype=torch.bool)
        for name, ref, dim in (('i2t', dg.expand_as(scores), 1), ('t2i', dg.t().expand_as(scores), 0)):
            if direction in (name, 'bidir'):
                cost = (margin + scores - ref).clamp(min=0).masked_fill(eye, 0)
                if maxv:
                    cost = cost.max(dim)[0]
                total = total + (cost.sum() if style == 'sum' else cost.mean())
    total.backward()
    return float(total.item()), s.grad.numpy(), im.grad.numpy()


@pytest.mark.parametrize('maxv,style,direction', FLAGS)
@pytest.mark.parametrize('shape', [(2, 5), (7, 3, 6), (19, 2, 12)])
def test_margin_restatement_matches_float64_autograd(shape, maxv, style, direction):
    g = np.random.default_rng(sum(shape))
    s, im = g.normal(0, 1, shape), g.normal(0, 1, shape)
    loss, d_s, d_im, b_s, b_im = loss_ref.margin(s, im, 0.2, maxv, style, direction)
    rl, rs, ri = _autograd64(s, im, 0.2, maxv, style, direction)
    assert d_s.shape == shape and d_im.shape == shape and b_s.shape == shape and b_im.shape == shape
    assert abs(loss - rl) <= 1e-12 * max(1.0, abs(rl))
    assert np.abs(d_s - rs.reshape(shape)).max() <= 1e-12 and np.abs(d_im - ri.reshape(shape)).max() <= 1e-12
    assert (b_s >= 0).all() and (b_im >= 0).all() and ((b_s > 0) | (d_s == 0)).all() and ((b_im > 0) | (d_im == 0)).all()


@pytest.mark.parametrize('B,H,d', MARGIN_SHAPES)
def test_margin_inputs_converge_with_every_decision_clear_and_many_hinges_active(B, H, d):
    s, im = _margin_inputs(B, H, d)
    assert s.shape == im.shape == (B, H, d) and s.dtype == im.dtype == np.float32
    assert not s.flags.writeable and not im.flags.writeable and _margin_inputs(B, H, d)[0] is s
    for h in range(H):
        S = margin_scores64(s, im, h)
        for maxv in (False, True):
            for direction in ('i2t', 't2i', 'bidir'):
                assert loss_ref.margin_scores_slack(S, MARGIN, maxv, direction) >= 1e-4, (h, maxv, direction)
        if B >= 17:
            assert margin_active_share(S) >= MIN_ACTIVE, (h, margin_active_share(S))


def _fp32_chain(s, im, margin, maxv, style, direction, fault=None):
    """(d_s, d_im) of laff_margin_loss's chain in fp32 numpy with every sum strictly sequential (one rounded product and one rounded
    addition per term, in index order): the worst order a kernel could take.  The decisions come from the float64 restatement, as the
    inputs guarantee.  fault = 'pair' drops one active off-diagonal pair from dS of the last head, 'row' zeroes its last row."""
    f = np.float32
    B, H, d = s.shape
    d_s, d_im = np.zeros((B, H, d), f), np.zeros((B, H, d), f)

    def seq_sum(terms):                       # over axis -1, in order
        acc = np.zeros(terms.shape[:-1], f)
        for k in range(terms.shape[-1]):
            acc = acc + terms[..., k]
        return acc

    def matmul(a, b):                         # a (n, K) . b (K, m), K in order
        acc = np.zeros((a.shape[0], b.shape[1]), f)
        for k in range(a.shape[1]):
            acc = acc + a[:, k, None] * b[None, k, :]
        return acc

    def normalize(x):
        r = np.sqrt(seq_sum(x * x))
        n = r + f(1e-13) + f(1e-14)
        return x / n[:, None], r, n

    def bwd(xh, r, n, G):
        return G / n[:, None] - xh * (seq_sum(xh * G) / r)[:, None]

    w = f(1.0)
    if style == 'mean':
        w = f(1.0) / f(B) if maxv else f(1.0) / (f(B) * f(B))
    for h in range(H):
        sh, rs, ns = normalize(s[:, h])
        ih, ri, ni = normalize(im[:, h])
        _, d64 = loss_ref.margin_scores(margin_scores64(s, im, h), margin, maxv, 'sum', direction)     # integer pair counts
        count = np.rint(d64).astype(int)
        dS = np.zeros((B, B), f)
        for t in range(1, int(np.abs(count).max()) + 1):          # one rounded addition of +-w per counted term
            dS = np.where(np.abs(count) >= t, dS + np.sign(count).astype(f) * w, dS)
        if h == H - 1 and fault == 'pair':
            i, j = np.argwhere((count > 0) & ~np.eye(B, dtype=bool))[-1]
            dS[i, j] = 0
        if h == H - 1 and fault == 'row':
            dS[-1] = 0
        d_im[:, h] = bwd(ih, ri, ni, matmul(dS, sh))
        d_s[:, h] = bwd(sh, rs, ns, matmul(dS.T.copy(), ih))
    return d_s, d_im


@pytest.mark.parametrize('maxv,style,direction', FLAGS)
@pytest.mark.parametrize('B,H,d', [(65, 1, 30), (130, 2, 30)])
def test_margin_gradient_bound_holds_for_sequential_fp32_and_catches_planted_faults(B, H, d, maxv, style, direction):
    s, im = _margin_inputs(B, H, d)
    _, ds64, di64, b_s, b_im = loss_ref.margin(s, im, MARGIN, maxv, style, direction)
    d_s, d_im = _fp32_chain(s, im, MARGIN, maxv, style, direction)
    assert d_s.dtype == np.float32
    e_s, e_i = np.abs(d_s - ds64), np.abs(d_im - di64)
    assert (e_s <= b_s).all() and (e_i <= b_im).all()
    pos_s, pos_i = b_s > 0, b_im > 0
    worst = max((e_s[pos_s] / b_s[pos_s]).max(), (e_i[pos_i] / b_im[pos_i]).max())
    assert worst <= 0.5, worst                # the worst order stays well inside: the kernel's tree sums have room
    # the bound is small against the gradient ...
    assert max(b_s.max(), b_im.max()) <= 1e-3 * max(np.abs(ds64).max(), np.abs(di64).max())
    # ... so a single dropped pair, or a dropped row, of one head's dS is far outside it
    for fault in ('pair', 'row'):
        f_s, f_i = _fp32_chain(s, im, MARGIN, maxv, style, direction, fault)
        over = max((np.abs(f_s - ds64)[pos_s] / b_s[pos_s]).max(), (np.abs(f_i - di64)[pos_i] / b_im[pos_i]).max())
        assert over >= 100.0, (fault, over)


# ------------------------------------------------------------------------------------------------ Python surface
def _opt(**kw):
    base = dict(loss='mrl', margin=0.2, measure='cosine', max_violation=True, cost_style='sum', direction='t2i')
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_criterion_for_routes_like_the_reference():
    from laff_amd import loss as L
    crit = L.criterion_for(_opt(loss='mrl', margin=0.3, direction='bidir', cost_style='mean', max_violation=False))
    assert isinstance(crit, L.MarginRankingLoss)
    assert (crit.margin, crit.max_violation, crit.cost_style, crit.direction) == (0.3, False, 'mean', 'bidir')
    assert isinstance(L.criterion_for(_opt(loss='dsl')), L.DualSoftmaxLoss)
    with pytest.raises(NotImplementedError, match='TypeError'):
        L.criterion_for(_opt(loss='CELoss'))
    with pytest.raises(Exception, match='Not such loss.') as e:
        L.criterion_for(_opt(loss='kl'))
    assert type(e.value) is Exception
    ws = L.MarginRankingLossWithScore(margin=0.1, max_violation=True, cost_style='mean', direction='i2t')
    assert (ws.margin, ws.max_violation, ws.cost_style, ws.direction) == (0.1, True, 'mean', 'i2t')
    assert callable(L.compute_loss_with_score)


def test_hist_margin_loss_is_still_refused():
    from laff_amd import loss as L
    with pytest.raises(NotImplementedError):
        L.MarginRankingLoss(measure='hist')
    with pytest.raises(NotImplementedError):
        L.criterion_for(_opt(loss='mrl', measure='hist'))


def test_ops_validate_before_touching_the_device():
    import torch
    from laff_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        ops.dsl_loss(x, torch.zeros(4, 7))
    with pytest.raises(ValueError):
        ops.dsl_loss(x, x, temp=0)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.dsl_loss(x, x)
    with pytest.raises(ValueError):
        ops.margin_loss_scores(torch.zeros(4, 5), 0.2)
    with pytest.raises(ValueError):
        ops.margin_loss_scores(torch.zeros(4, 4), 0.2, direction='both')
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.margin_loss_scores(torch.zeros(4, 4), 0.2)
