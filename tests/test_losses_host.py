"""Dual-softmax and score-matrix margin criteria, the part that needs no GPU: the C ABI's declarations, exports, bindings and argument
checks, the float64 restatement (tests/loss_ref.py) against the golden vectors and against central differences, and the routing of
loss.criterion_for."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('laff_dsl_loss_workspace_bytes', 'laff_dsl_loss', 'laff_margin_loss_scores')
F64_NOISE = 1e-12          # float64 rounding of the restatement itself (a BLAS that sums in another order), far below any e_ref > 0


# ------------------------------------------------------------------------------------------------ C ABI
@pytest.mark.parametrize('name', NEW_SYMBOLS)
def test_header_declares_the_symbol(name):
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert re.search(r'^int %s\(' % name, text, flags=re.M), name


@pytest.mark.parametrize('name', NEW_SYMBOLS)
def test_library_exports_and_lib_binds_the_symbol(name):
    from laff_amd import _lib
    assert name in _lib.SIGNATURES
    raw = C.CDLL(_lib.LIB_PATH)
    assert getattr(raw, name) is not None            # AttributeError if the built library does not export it
    fn = getattr(_lib.load(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]


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
