"""Host tests of tests/fc_ref.py: the reference of the FC routes and its tolerances can tell right from wrong (no GPU needed).

  * split_ref keeps the invariants of the documented hi/lo split, on rows of every magnitude class;
  * fc_exact64 (the operands the kernel forms) and fc_contract64 (the fp32 x and W) agree within the 2^-22-class error the header
    promises for the split;
  * SENSITIVITY: every tolerance constant the GPU suite uses is at least 10 x below what each of eight deliberately wrong kernels
    produces, on the GPU suite's own input generator and at the K values of its CASES table.  This is a condition on the
    tolerances: one that fails it is too loose to be kept.
"""
import numpy as np
import pytest
import torch

import fc_ref as R
from test_gpu_fc_routes import CASES

KS = (32, 96, 512, 2080, 4096)


def _rows_of_every_class(K, seed=0):
    g = np.random.default_rng(seed)
    base = np.clip(g.standard_normal((7, K)), -3, 3).astype(np.float32)
    x = base.copy()
    x[1] *= np.float32(3e4)
    x[2] *= np.float32(1e-6)
    x[3] *= np.float32(1e-30)
    x[4] *= np.float32(1e38)
    x[5] = 0
    x[6, K // 2] = np.inf
    return x


@pytest.mark.parametrize('K', (4, 77, 96, 512, 1030))
def test_split_ref_invariants(K):
    x = _rows_of_every_class(K)
    hi, lo, rs, e = R.split_ref(x)
    Kp = -(-K // 64) * 64
    assert hi.shape == lo.shape == (7, Kp) and hi.dtype == lo.dtype == np.float16 and rs.dtype == np.float32
    assert not hi[:, K:].view(np.int16).any() and not lo[:, K:].view(np.int16).any()                 # padding: +0 bits
    mant = rs.view(np.uint32) & 0x7fffff
    assert not mant.any() and np.all(rs > 0) and np.all(np.isfinite(rs))                              # powers of two, normal
    assert np.array_equal(rs.astype(np.float64), np.ldexp(1.0, e - 9))
    for r in range(5):                                                                                # the finite, non-zero rows
        m = np.abs(x[r]).max().astype(np.float64)
        top = np.abs(hi[r].astype(np.float64)).max()
        assert 512 <= top <= 1024, (r, top)       # [512, 1024) before rounding; hi may round up to 1024 itself
        back = (hi[r, :K].astype(np.float64) + lo[r, :K].astype(np.float64)) * rs[r].astype(np.float64)
        assert np.abs(back - x[r].astype(np.float64)).max() <= 2.0 ** -21 * m, r
    assert e[5] == 0 and not hi[5].view(np.int16).any() and not lo[5].view(np.int16).any()          # the all-zero row
    assert e[6] == 0 and np.isinf(hi[6, K // 2]) and np.isnan(lo[6, K // 2])                          # the row holding an inf
    fin = np.ones(K, bool)
    fin[K // 2] = False
    t = x[6, :K][fin].astype(np.float64) * 512                      # its other entries: split at s = 2^9, still exact to 2^-21
    back = hi[6, :K][fin].astype(np.float64) + lo[6, :K][fin].astype(np.float64)
    assert np.abs(back - t).max() <= 2.0 ** -21 * np.abs(t).max()


def test_split_ref_exponent_rule():
    x = np.zeros((6, 8), np.float32)
    x[0, 3] = 2.0 ** -105                    # below the clamp: e = -100
    x[1, 0] = np.float32(1e-45)              # a denormal maximum: clamped too
    x[2, 1] = -1023.9                        # e = 9: s = 1
    x[3, :] = np.nan                         # NaNs never win the maximum: an all-NaN row has maximum 0
    x[4, 2], x[4, 5] = np.nan, 3.0           # ... and a NaN beside finite entries leaves their exponent
    x[5, 7] = -np.inf
    hi, lo, rs, e = R.split_ref(x)
    assert e.tolist() == [-100, -100, 9, 0, 1, 0]
    assert rs[0] == np.float32(2.0 ** -109) and rs[2] == 1.0 and rs[4] == np.float32(2.0 ** -8)
    assert hi[0, 3] == np.float16(16.0) and hi[2, 1] == np.float16(-1024.0) and hi[4, 5] == np.float16(768.0)
    assert np.isnan(hi[3, :8]).all() and not hi[3, 8:].view(np.int16).any() and np.isnan(hi[4, 2]) and np.isnan(lo[4, 2])
    assert hi[5, 7] == -np.inf and np.isnan(lo[5, 7])


@pytest.mark.parametrize('K', (4, 77, 260, 1030))
def test_split_ref_torch_twin_is_bit_identical(K):
    x = np.concatenate([_rows_of_every_class(K, 3), np.full((1, K), np.nan, np.float32)])
    x[0, K // 3] = np.nan
    hi, lo, rs, _ = R.split_ref(x)
    th, tl, tr = R.split_ref_t(torch.from_numpy(x))
    for a, b in ((hi, th), (lo, tl)):
        a16, b16 = a.view(np.int16), b.numpy().view(np.int16)
        nan = np.isnan(a)
        assert np.array_equal(nan, np.isnan(b.numpy())) and np.array_equal(a16[~nan], b16[~nan])
    assert np.array_equal(rs.view(np.int32), tr.numpy().view(np.int32))


def _planes(t):
    return R.split_ref_t(t)


@pytest.mark.parametrize('K', KS)
def test_exact_and_contract_references_agree(K):
    """x~ = hi + lo = x (1 + d), |d| <= 2^-22 (lo's own rounding); the kernel's three products leave lo lo' <= 2^-22 |x w| out: the two
    references differ by at most (2 + 1) 2^-22 sum |x w| = 12 units of 2^-24 absdot, and a little for second-order terms."""
    x, w, b, sc, sh = R.make_problem(96, K, 80, 100 + K)
    ex = R.fc_exact64(_planes(x), _planes(w), b, None, sc, sh)
    co = R.fc_contract64(x, w, b, None, sc, sh)
    e = R.norm_err(ex, co, R.absdot(x, w, b, sc, sh))
    print('K = %d: exact vs contract %.2f units' % (K, e))
    assert 0 < e <= 13.0
    assert torch.equal(R.fc_exact64(x, w, b, 'tanh', sc, sh), R.fc_contract64(x, w, b, 'tanh', sc, sh))       # fp32 routes: one thing


@pytest.mark.parametrize('K', KS)
def test_inputs_keep_tanh_unsaturated(K):
    x, w, b, sc, sh = R.make_problem(512, K, 256, 7 + K)
    pre = x.double() @ w.double().T + b.double()
    assert float((pre.abs() > 3).double().mean()) < 0.01
    xp = R.make_problem(1000, K, 64, 7 + K, plant=True)[0]
    pre = xp.double() @ w.double()[:64].T
    frac = float((~(pre.abs() <= 3)).double().mean())
    print('K = %d: %.2f %% of the planted problem beyond |pre| = 3' % (K, 100 * frac))
    assert frac < 0.01


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------
def _wrong_results(x, w, b, sc, sh, act, split):
    """(name, float64 result) of deliberately wrong kernels on the split operands (split) or on the fp32 ones."""
    N, K = x.shape
    D = w.shape[0]
    xr, wr = x.double(), w.double()
    if split:
        xh, xl, xs = [t.double() for t in _planes(x)]
        wh, wl, ws = [t.double() for t in _planes(w)]
        Kp = xh.shape[1]
        scale = xs[:, None] * ws[None, :]
        full = xl @ wh.T + xh @ wl.T + xh @ wh.T
        ep = lambda p, bias=b, s_=sc, h_=sh, sc_=scale: R.epilogue64(p * sc_, bias, act, s_, h_)
        yield 'lo*hi dropped', ep(xh @ wl.T + xh @ wh.T)
        yield 'hi*lo dropped', ep(xl @ wh.T + xh @ wh.T)
        cut = lambda n: (xl[:, :K - n] @ wh[:, :K - n].T + xh[:, :K - n] @ wl[:, :K - n].T + xh[:, :K - n] @ wh[:, :K - n].T)
        if Kp > K:          # the pad columns K..Kp of both operands hold the next row's first values instead of zeros
            n = Kp - K
            xt, wt = (xh + xl).roll(-1, 0)[:, :n], (wh + wl).roll(-1, 0)[:, :n]
            yield 'pad read as the next row', ep(full + xt @ wt.T)
        s2 = scale.clone()
        s2[N // 2] *= 2
        yield 'rscale one binade off', ep(full, sc_=s2)
    else:
        full = xr @ wr.T
        ep = lambda p, bias=b, s_=sc, h_=sh: R.epilogue64(p, bias, act, s_, h_)
        cut = lambda n: xr[:, :K - n] @ wr[:, :K - n].T
    yield 'last 16 columns dropped', ep(cut(min(16, K // 2)))
    yield 'last 64-column chunk dropped', ep(cut(K - (K - 1) // 64 * 64 if K > 64 else K // 2))
    if b is not None:
        yield 'bias of column j + 1', ep(full, bias=b.roll(-1))
    if sc is not None:
        yield 'BatchNorm scale and shift swapped', ep(full, s_=sh, h_=sc)


def _ks(pred):
    return sorted({p.Dk for c in CASES if pred(c) for p in c.problems(256)})


def _check(name, got_err, tol, what):
    print('  %-34s %10.3g   (%s %.3g)' % (name, got_err, what, tol))
    assert got_err >= 10 * tol, '%s: a kernel with "%s" errs %.3g, within 10 x the tolerance %.3g: the tolerance is too loose' % (
        what, name, got_err, tol)


@pytest.mark.parametrize('act', (None, 'relu'))
@pytest.mark.parametrize('route', sorted(R.EXACT_TOL))
def test_exact_tolerance_catches_wrong_kernels(route, act):
    split = not route.startswith('F32')
    for K in _ks(lambda c: route in c.route):
        x, w, b, sc, sh = R.make_problem(96, K, 80, 1000 + K)
        ref = R.fc_exact64(_planes(x), _planes(w), b, act, sc, sh) if split else R.fc_exact64(x, w, b, act, sc, sh)
        ad = R.absdot(x, w, b, sc, sh)
        print('%s %s, K = %d' % (route, act, K))
        for name, y in _wrong_results(x, w, b, sc, sh, act, split):
            _check(name, R.norm_err(y, ref, ad), R.EXACT_TOL[route], 'EXACT_TOL[%s]' % route)


@pytest.mark.parametrize('act', (None, 'tanh', 'sigmoid'))
@pytest.mark.parametrize('family', sorted(R.CONTRACT_TOL))
def test_contract_tolerance_catches_wrong_kernels(family, act):
    """The GPU suite holds every problem, whatever its activation, against fc_contract64 in units of 2^-24 absdot_act."""
    for K in _ks(lambda c: c.family == family):
        x, w, b, sc, sh = R.make_problem(96, K, 80, 2000 + K)
        ref = R.fc_contract64(x, w, b, act, sc, sh)
        ad = R.absdot_act(x, w, b, act, sc, sh)
        print('%s %s, K = %d' % (family, act, K))
        for name, y in _wrong_results(x, w, b, sc, sh, act, family != 'fp32'):
            _check(name, R.norm_err(y, ref, ad), R.CONTRACT_TOL[family], 'CONTRACT_TOL[%s]' % family)


@pytest.mark.parametrize('act', ('tanh', 'sigmoid'))
@pytest.mark.parametrize('split', (False, True), ids=('fp32', 'split'))
def test_activation_tolerance_catches_wrong_kernels(split, act):
    for K in _ks(lambda c: (c.family != 'fp32') == split):
        x, w, b, sc, sh = R.make_problem(96, K, 80, 3000 + K)
        ref = R.fc_exact64(_planes(x), _planes(w), b, act, sc, sh) if split else R.fc_exact64(x, w, b, act, sc, sh)
        assert float(R.absdot(x, w, b).max()) <= R.ACT_ABSDOT_MAX          # the GPU suite applies ACT_TOL to such entries
        print('%s %s, K = %d' % ('split' if split else 'fp32', act, K))
        for name, y in _wrong_results(x, w, b, sc, sh, act, split):
            _check(name, float((y - ref).abs().max()), R.ACT_TOL[act], 'ACT_TOL[%s]' % act)
