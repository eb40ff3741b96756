"""laff_dsl_loss, laff_margin_loss_scores and laff_margin_loss on a real MI355X against the float64 restatement of tests/loss_ref.py and the golden vectors.

Bounds of the dual-softmax checks are derived per case, not fixed: the reference arithmetic is run in fp32 on the CPU (plain torch ops,
_torch_fp32 below) on the case's inputs, its deviation from the float64 restatement is measured, and the kernel gets 4x that -- it sums
in another order and uses the hardware exp / log.  Floors: one fp32 ulp of the loss; 2^-23 times the largest gradient magnitude.  Every
derived bound is asserted to stay inside what the project accepts for the margin loss (2e-5 relative on the loss, 2e-6 absolute on the
gradients), or to stay within the figures listed in NEEDS_MORE; the MEASURED table below holds the largest kernel deviations seen on the
MI355X beside the bounds they were held to.
"""
import functools

import numpy as np
import pytest
import torch

import loss_ref
from util import maxdiff

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LOSS_REL, GRAD_ABS = 2e-5, 2e-6          # the project's margin-loss bounds (test_margin_loss_golden_forward_and_backward)

# what each shape exercises
SHAPES = [(1, 1, 8),        # a single pair: loss exactly 0, zero gradients
          (2, 3, 5),        # the smallest real case, heads != 1, d no multiple of 4
          (63, 1, 36), (64, 2, 64), (65, 1, 30),      # either side of one wavefront
          (130, 2, 30),     # padded Bp and dp
          (257, 1, 64),     # one row past a 256 boundary
          (1024, 1, 64)]    # the largest batch the margin loss is tested at per workgroup (laff_margin_loss accepts up to 8188)
TEMPS = [1000, 1, 0.01]     # 0.01: logits of +-100, only the max subtraction keeps exp finite

# MEASURED on the MI355X by test_dsl_loss_vs_float64 (it prints every figure): the kernel's largest deviation from float64 over the seven
# shapes with B > 1 (B = 1 is exactly 0), beside the tightest .. loosest derived bound of those shapes and the largest error / bound
# ratio of any single case.  The loss errors are absolute; relative to max(1, |loss|) none exceeds 1e-6.
#   temp   loss: max error  (case)              bounds             worst ratio | gradient: max error   bounds             worst ratio
#   1000   6.76e-5  (130, 2, 30), loss 1073     2.88e-7 .. 4.88e-4   0.25      | 2.87e-8               2.53e-8 .. 9.45e-8   0.56
#   1      3.43e-5  (1024, 1, 64), loss 5510    1.65e-6 .. 1.82e-3   0.25      | 9.31e-8               7.83e-8 .. 2.36e-7   0.55
#   0.01   6.34e-4  (1024, 1, 64), loss 651     6.49e-7 .. 4.73e-3   0.60      | 8.49e-4 (max |g| 111) 1.40e-6 .. 2.04e-3   0.62

# At temp = 0.01 the reference arithmetic in fp32 is itself further from float64 than the margin-loss bounds: it rounds M / temp, logits
# of +-100, to 100 * 2^-24 = 6e-6 before the exp, and the gradients carry the factor n / temp.  These cases are held to their derived
# bound (4x that deviation), which is wider than 2e-5 relative / 2e-6 absolute.  Per case: the derived loss and gradient bounds, the
# largest |gradient|, and the kernel's deviation from float64 MEASURED on the MI355X (loss, gradient).  The derived bounds depend a
# little on the CPU that runs the fp32 reference (its summation order follows the vector width and the thread count: 1.7e-3 and 2.0e-3
# were seen for the last case on two hosts), so a bound may exceed its listed figure by half, not more.
# Only the loss bound of (64, 2, 64) exceeds 2e-5 * max(1, |loss|) (4.0e-5 against 2.7e-5); the other five loss bounds are inside it
# (1024: 4.7e-3 against 1.3e-2) and these cases are listed for their gradient bound.
NEEDS_MORE = {
    # (B, H, d, temp): (b_loss, b_grad, max |grad|, measured e_loss, measured e_grad)
    (2, 3, 5, 0.01): (6.5e-7, 2.5e-6, 0.22, 7.6e-8, 1.1e-6),
    (63, 1, 36, 0.01): (3.6e-6, 1.5e-5, 0.59, 1.9e-6, 7.0e-6),
    (64, 2, 64, 0.01): (4.0e-5, 4.8e-5, 0.95, 4.5e-6, 5.4e-6),
    (65, 1, 30, 0.01): (2.1e-5, 8.4e-5, 1.2, 5.2e-6, 2.2e-5),
    (130, 2, 30, 0.01): (6.1e-6, 1.2e-4, 3.2, 3.4e-6, 3.3e-5),
    (1024, 1, 64, 0.01): (4.7e-3, 2.1e-3, 111.0, 6.3e-4, 8.5e-4),
}


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)          # a copy: the shared references are read-only


def _inputs(B, H, d, seed=0):
    """The correlated construction of test_margin_loss_vs_oracle: matched pairs share a latent, the diagonal dominates."""
    g = np.random.default_rng(B + H + d + seed)
    z = g.normal(0, 1, (B, 16)).astype(np.float32)
    P = g.normal(0, 1, (16, H * d)).astype(np.float32)
    s = (z @ P + 2.0 * g.normal(0, 1, (B, H * d))).astype(np.float32).reshape(B, H, d)
    im = (z @ P + 2.0 * g.normal(0, 1, (B, H * d))).astype(np.float32).reshape(B, H, d)
    return s, im


def _torch_fp32(s, im, temp):
    """The reference arithmetic in fp32 on the CPU, with autograd: (loss, d_s, d_im) as numpy."""
    s = torch.tensor(s, requires_grad=True)
    im = torch.tensor(im, requires_grad=True)

    def l2norm(x):
        return x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-13 + 1e-14)

    def cal(m):
        m = m * torch.softmax(m / temp, dim=0) * len(m)
        return -torch.diag(torch.log_softmax(m, dim=-1)).sum()

    with torch.enable_grad():
        total = 0
        for h in range(s.shape[1]):
            m = l2norm(s[:, h]).mm(l2norm(im[:, h]).t())
            total = total + (cal(m) + cal(m.T)) / 2
        total.backward()
    return float(total.item()), s.grad.numpy(), im.grad.numpy()


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _bounds(l64, g64s, l32, g32s):
    """(absolute loss bound, absolute gradient bound) from the fp32 reference's own deviation; the gradient pairs are (d_s, d_im)."""
    b_loss = max(4.0 * abs(l32 - l64), _ulp32(l64))
    dev_g = max(np.abs(a - b).max() for a, b in zip(g32s, g64s))
    gmax = max(np.abs(a).max() for a in g64s)
    b_grad = max(4.0 * dev_g, 2.0 ** -23 * gmax)
    return b_loss, b_grad


@functools.lru_cache(maxsize=None)
def _case(B, H, d, temp):
    """Inputs, the float64 reference and the derived bounds of one case: computed once, shared, never written to."""
    s, im = _inputs(B, H, d)
    l64, ds64, di64 = loss_ref.dsl(s, im, temp)
    l32, ds32, di32 = _torch_fp32(s, im, temp)
    b_loss, b_grad = _bounds(l64, (ds64, di64), l32, (ds32, di32))
    for a in (s, im, ds64, di64):
        a.setflags(write=False)
    return s, im, l64, ds64, di64, b_loss, b_grad


def _nan_like(shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def _dsl_raw(s, im, temp, want_grad=True):
    """laff_dsl_loss through the binding with every output buffer (and the workspace) NaN before the launch."""
    import ctypes as C
    from laff_amd import ops
    B, H, d = s.shape
    lib, h = ops._context(s.device)
    nbytes = ops._size_query('laff_dsl_loss_workspace_bytes', B, H, d)
    ws = _nan_like((nbytes // 4,))
    loss = _nan_like(())
    d_s = _nan_like(tuple(s.shape)) if want_grad else None
    d_im = _nan_like(tuple(s.shape)) if want_grad else None
    ops.check(lib.laff_dsl_loss(h, ops._ptr(s), ops._ptr(im), B, H, d, float(temp), ops._ptr(loss), ops._ptr(d_s), ops._ptr(d_im),
                                ops._ptr(ws), C.c_size_t(nbytes)))
    return loss, d_s, d_im


# ---------------------------------------------------------------------------------------------- dual softmax
@pytest.mark.parametrize('temp', TEMPS)
@pytest.mark.parametrize('B,H,d', SHAPES)
def test_dsl_loss_vs_float64(B, H, d, temp):
    s, im, l64, ds64, di64, b_loss, b_grad = _case(B, H, d, temp)
    loss, d_s, d_im = _dsl_raw(dev(s), dev(im), temp)
    e_loss = abs(loss.item() - l64)
    e_grad = max(maxdiff(d_s, ds64), maxdiff(d_im, di64))
    print('dsl B=%d H=%d d=%d temp=%g: loss %.9g err %.3g (bound %.3g)  grad max %.3g err %.3g (bound %.3g)'
          % (B, H, d, temp, l64, e_loss, b_loss, max(np.abs(ds64).max(), np.abs(di64).max()), e_grad, b_grad))
    # the derived bounds are no looser than the project's margin-loss ones; a case listed in NEEDS_MORE may reach 1.5x its listed figures
    lim_loss, lim_grad = LOSS_REL * max(1.0, abs(l64)), GRAD_ABS
    if (B, H, d, temp) in NEEDS_MORE:
        listed = NEEDS_MORE[(B, H, d, temp)]
        lim_loss, lim_grad = max(lim_loss, 1.5 * listed[0]), max(lim_grad, 1.5 * listed[1])
    assert b_loss <= lim_loss and b_grad <= lim_grad, (b_loss, lim_loss, b_grad, lim_grad)
    assert np.isfinite(loss.item()) and torch.isfinite(d_s).all() and torch.isfinite(d_im).all()
    assert e_loss <= b_loss and e_grad <= b_grad, (e_loss, b_loss, e_grad, b_grad)
    if B == 1:
        assert loss.item() == 0.0 and not d_s.any() and not d_im.any()


def test_dsl_loss_golden(golden):
    """Against the reference's own fp32 results: 4x its deviation from float64 (e_ref) for the kernel, plus e_ref itself for the golden
    side of the comparison, with the same floors."""
    from laff_amd import ops
    g = golden('dsl_loss')
    for c in g.json('cases'):
        k = c['key']
        s, im = g[k + '/s'], g[k + '/im']
        loss, d_s, d_im = ops.dsl_loss(dev(s), dev(im), c['temp'])
        l64, ds64, di64 = loss_ref.dsl(s, im, c['temp'])
        e_loss, e_grad = g[k + '/e_ref']
        b_loss = max(4.0 * e_loss * max(1.0, abs(l64)), _ulp32(l64))
        b_grad = max(4.0 * e_grad, 2.0 ** -23 * max(np.abs(ds64).max(), np.abs(di64).max()))
        assert b_loss <= LOSS_REL * max(1.0, abs(l64)) and b_grad <= GRAD_ABS, c
        assert tuple(d_s.shape) == tuple(s.shape) and abs(loss.item() - l64) <= b_loss, (c, loss.item(), l64, b_loss)
        assert max(maxdiff(d_s, ds64), maxdiff(d_im, di64)) <= b_grad, c
        ref = float(g[k + '/loss'])
        assert abs(loss.item() - ref) <= b_loss + e_loss * max(1.0, abs(l64)), c
        assert max(maxdiff(d_s, g[k + '/d_s']), maxdiff(d_im, g[k + '/d_im'])) <= b_grad + e_grad, c


@pytest.mark.parametrize('B,H,d,temp', [(2, 3, 5, 1000), (65, 1, 30, 0.01), (130, 2, 30, 1)])
def test_dsl_forward_only_writes_no_gradients_and_the_same_loss(B, H, d, temp):
    from laff_amd import ops
    s, im = _case(B, H, d, temp)[:2]
    full = _dsl_raw(dev(s), dev(im), temp)[0]
    loss, d_s, d_im = _dsl_raw(dev(s), dev(im), temp, want_grad=False)
    assert d_s is None and d_im is None
    assert loss.item() == full.item()                      # bit for bit
    # no gradient buffer is allocated: the peak of the forward-only call stays below the gradient call's by at least d_s + d_im
    ds, di = dev(s), dev(im)
    peaks = []
    for want in (True, False):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = ops.dsl_loss(ds, di, temp, want_grad=want)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert out[0].item() == full.item() and (out[1] is None) == (not want) and (out[2] is None) == (not want)
        del out
    assert peaks[1] <= peaks[0] - 2 * B * H * d * 4, peaks
    # under no_grad the module takes the same forward-only path
    from laff_amd import loss as L
    sg, ig = ds.clone().requires_grad_(True), di.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        l3 = L.DualSoftmaxLoss()(sg, ig, temp)
    torch.cuda.synchronize()
    assert l3.item() == full.item() and torch.cuda.max_memory_allocated() - base <= peaks[1]


def test_dsl_module_on_autograd_2d_and_3d():
    from laff_amd import loss as L
    crit = L.DualSoftmaxLoss()
    for shape, temp in (((40, 64), 1000), ((33, 2, 20), 1)):
        g = np.random.default_rng(len(shape))
        s_np, im_np = g.normal(0, 1, shape).astype(np.float32), g.normal(0, 1, shape).astype(np.float32)
        s = torch.tensor(s_np, device=DEV, requires_grad=True)
        im = torch.tensor(im_np, device=DEV, requires_grad=True)
        (3 * crit(s, im, temp)).backward()
        l64, ds64, di64 = loss_ref.dsl(s_np, im_np, temp)
        l32, ds32, di32 = _torch_fp32(s_np.reshape(shape[0], -1, shape[-1]), im_np.reshape(shape[0], -1, shape[-1]), temp)
        b_loss, b_grad = _bounds(l64, (ds64, di64), l32, (ds32.reshape(shape), di32.reshape(shape)))
        assert b_grad <= GRAD_ABS
        assert s.grad.shape == s.shape and maxdiff(s.grad, 3 * ds64) <= 3 * b_grad and maxdiff(im.grad, 3 * di64) <= 3 * b_grad
        with torch.no_grad():
            assert abs(crit(s, im, temp).item() - l64) <= b_loss
    # compute_loss takes the criterion unchanged (vis first, as the reference's signature)
    s = torch.tensor(s_np, device=DEV, requires_grad=True)
    im = torch.tensor(im_np, device=DEV, requires_grad=True)
    loss, items = L.compute_loss(crit, im, s)
    assert items == {'triplet_loss': loss} and items['triplet_loss'] is loss
    l64 = loss_ref.dsl(s_np, im_np, 1000)[0]
    assert abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64))
    loss.backward()
    assert s.grad is not None and im.grad is not None


# ---------------------------------------------------------------------------------------------- margin ranking loss on a score matrix
FLAGS = [(maxv, style, direction) for maxv in (False, True) for style in ('sum', 'mean') for direction in ('i2t', 't2i', 'bidir')]


def test_margin_loss_scores_golden(golden):
    from laff_amd import ops
    g = golden('margin_scores')
    for c in g.json('cases'):
        k = c['key']
        sc = g[k + '/score']
        loss, d = ops.margin_loss_scores(dev(sc), c['margin'], c['max_violation'], c['cost_style'], c['direction'])
        l64, d64 = loss_ref.margin_scores(sc, c['margin'], c['max_violation'], c['cost_style'], c['direction'])
        ref = float(g[k + '/loss'])
        assert abs(loss.item() - ref) <= LOSS_REL * max(1.0, abs(ref)) and abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64)), c
        assert tuple(d.shape) == sc.shape and maxdiff(d, g[k + '/d_score']) <= GRAD_ABS and maxdiff(d, d64) <= GRAD_ABS, c


def _too_close(sc, margin, maxv, direction):
    """The off-diagonal entries of sc that sit within 1e-4 of a decision (float64): a hinge argument near 0, or, under max_violation,
    a row's / column's hardest negative that leads its runner-up by less."""
    S = sc.astype(np.float64)
    B = S.shape[0]
    off = ~np.eye(B, dtype=bool)
    bad = np.zeros((B, B), bool)
    for name, ref, axis in (('i2t', np.diag(S)[:, None], 1), ('t2i', np.diag(S)[None, :], 0)):
        if direction not in (name, 'bidir'):
            continue
        arg = margin + S - ref
        bad |= (np.abs(arg) < 1e-4) & off
        if maxv and B > 2:
            cost = np.where(off, np.maximum(arg, 0.0), -np.inf)
            top = np.sort(cost, axis=axis)
            first, second = (top[:, -1], top[:, -2]) if axis == 1 else (top[-1, :], top[-2, :])
            q = np.nonzero((first > 0.0) & (first - second < 1e-4))[0]
            a = cost.argmax(axis=axis)[q]
            bad[(q, a) if axis == 1 else (a, q)] = True
    return bad


@functools.lru_cache(maxsize=None)
def _scores(B, maxv, direction):
    """A (B, B) fp32 score matrix whose every hinge argument and max-violation runner-up is >= 1e-4 from its decision in float64:
    the fp32 kernel then takes every decision as float64 does and the comparison is element-wise, no row left out.  The entries that are
    too close are drawn again, 100 times at the most; the caller asserts the result with loss_ref.margin_scores_slack."""
    g = np.random.default_rng(B * 4 + maxv)
    sc = (0.3 * np.eye(B) + g.uniform(-0.4, 0.4, (B, B))).astype(np.float32)
    for _ in range(100):
        bad = _too_close(sc, 0.2, maxv, direction)
        if not bad.any():
            sc.setflags(write=False)
            return sc
        sc[bad] = g.uniform(-0.4, 0.4, int(bad.sum())).astype(np.float32)
    raise AssertionError('B=%d: entries within 1e-4 of a decision are left after 100 draws' % B)


@pytest.mark.parametrize('maxv,style,direction', FLAGS)
@pytest.mark.parametrize('B', [1, 2, 65, 257, 1025])      # 1025: the tid-strided loops of the 1024-thread workgroup take a second trip
def test_margin_loss_scores_vs_float64(B, maxv, style, direction):
    from laff_amd import ops
    sc = _scores(B, maxv, direction)
    assert loss_ref.margin_scores_slack(sc, 0.2, maxv, direction) >= 1e-4          # asserted in float64 before the launch
    l64, d64 = loss_ref.margin_scores(sc, 0.2, maxv, style, direction)
    loss, d = ops.margin_loss_scores(dev(sc), 0.2, maxv, style, direction)
    assert abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64)), (loss.item(), l64)
    assert maxdiff(d, d64) <= GRAD_ABS
    # a strided view, ld > B: the same matrix inside a wider NaN one
    wide = torch.full((B, B + 7), float('nan'), dtype=torch.float32, device=DEV)
    wide[:, :B] = dev(sc)
    view = wide[:, :B]
    assert view.stride(0) == B + 7
    l2, d2 = ops.margin_loss_scores(view, 0.2, maxv, style, direction)
    assert l2.item() == loss.item() and tuple(d2.shape) == (B, B) and torch.equal(d2, d)
    # forward only
    l3, d3 = ops.margin_loss_scores(dev(sc), 0.2, maxv, style, direction, want_grad=False)
    assert d3 is None and l3.item() == loss.item()


def _plant_ties(sc):
    """A copy of sc with exact ties planted on the hardest negative of a few rows (S[i, b] = S[i, a], a the row's hardest caption) and
    of a few columns (S[b, j] = S[a, j], a the column's hardest video): b in a's lane of the wave that scans the row (b = a -+ 64), in a
    neighbouring lane (a -+ 1) and far away, below and above a.  Returns (matrix, rows {i: b}, columns {j: b}).  A plant is kept only if
    every other decision of the matrix stays 1e-4 clear (_tie_slack), so the result is asserted, not assumed."""
    S = sc.copy()
    B = S.shape[0]
    rows, cols = {}, {}
    for axis, planted in ((1, rows), (0, cols)):
        for off in (-64, 64, -1, 1, -40, 40):
            for q in range(B):
                if q in planted:
                    continue
                line = S[q, :] if axis == 1 else S[:, q]
                cost = _line_cost(S, q, axis)
                a = int(cost.argmax())
                b = a + off
                if cost[a] <= 0.0 or not 0 <= b < B or b == q:
                    continue
                at = (q, b) if axis == 1 else (b, q)
                keep = S[at]
                S[at] = line[a]
                planted[q] = b
                if _tie_slack(S, rows, cols) >= 1e-4 and _ties_hold(S, rows, cols):
                    break
                S[at] = keep
                del planted[q]
            else:
                raise AssertionError('no place for a tie at offset %d along axis %d' % (off, axis))
    S.setflags(write=False)
    return S, rows, cols


def _line_cost(S, q, axis):
    line = np.asarray(S[q, :] if axis == 1 else S[:, q], np.float64)
    cost = np.maximum(0.2 + line - np.float64(S[q, q]), 0.0)
    cost[q] = 0.0
    return cost


def _hardest(S, q, axis, b):
    """The index that the planted entry b of row / column q ties with."""
    cost = _line_cost(S, q, axis)
    return int([k for k in np.nonzero(cost == cost.max())[0] if k != b][0])


def _ties_hold(S, rows, cols):
    """Every planted entry is one of exactly two equal, positive maxima of its row resp. column."""
    for planted, axis in ((rows, 1), (cols, 0)):
        for q, b in planted.items():
            cost = _line_cost(S, q, axis)
            if not (cost[b] == cost.max() > 0.0 and int((cost == cost.max()).sum()) == 2):
                return False
    return True


def _tie_slack(S, rows, cols):
    """loss_ref.margin_scores_slack at margin 0.2, max_violation, 'bidir', with only the planted entries (row i, column rows[i]) and
    (row cols[j], column j) exempt from the runner-up lead of their row resp. column."""
    S = np.asarray(S, np.float64)
    B = S.shape[0]
    off = ~np.eye(B, dtype=bool)
    slack = np.inf
    for planted, ref, axis in ((rows, np.diag(S)[:, None], 1), (cols, np.diag(S)[None, :], 0)):
        arg = 0.2 + S - ref
        slack = min(slack, np.abs(arg[off]).min())
        cost = np.where(off, np.maximum(arg, 0.0), -np.inf)
        for q, b in planted.items():
            cost[(q, b) if axis == 1 else (b, q)] = -np.inf
        top = np.sort(cost, axis=axis)
        first, second = (top[:, -1], top[:, -2]) if axis == 1 else (top[-1, :], top[-2, :])
        lead = (first - second)[first > 0.0]
        if lead.size:
            slack = min(slack, lead.min())
    return slack


@pytest.mark.parametrize('style', ['sum', 'mean'])
@pytest.mark.parametrize('direction', ['i2t', 't2i', 'bidir'])
def test_margin_loss_scores_ties_take_the_first_maximum(style, direction):
    """Two equal hardest negatives in a row (the wave's arg-max butterfly) or a column (the thread's scan): the gradient goes to the
    one with the smaller index, as torch.max and loss_ref.margin_scores do."""
    from laff_amd import ops
    sc, rows, cols = _plant_ties(_scores(130, True, 'bidir'))
    assert len(rows) == 6 and len(cols) == 6 and _tie_slack(sc, rows, cols) >= 1e-4          # in float64, before the launch
    assert _ties_hold(sc, rows, cols)
    assert {b < _hardest(sc, q, 1, b) for q, b in rows.items()} == {False, True} == {b < _hardest(sc, q, 0, b) for q, b in cols.items()}
    l64, d64 = loss_ref.margin_scores(sc, 0.2, True, style, direction)
    loss, d = ops.margin_loss_scores(dev(sc), 0.2, True, style, direction)
    assert abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64)), (loss.item(), l64)
    assert maxdiff(d, d64) <= GRAD_ABS


def test_compute_loss_with_score_on_autograd():
    from laff_amd import loss as L
    sc = _scores(65, True, 'bidir')
    score = torch.tensor(sc, device=DEV, requires_grad=True)
    crit = L.MarginRankingLossWithScore(margin=0.2, max_violation=True, cost_style='sum', direction='bidir')
    loss, items = L.compute_loss_with_score(crit, score)
    assert items['triplet_loss'] is loss
    (3 * loss).backward()
    l64, d64 = loss_ref.margin_scores(sc, 0.2, True, 'sum', 'bidir')
    assert abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64)) and maxdiff(score.grad, 3 * d64) <= 3 * GRAD_ABS
    # a score matrix that is itself computed on the device stays on the graph
    half = torch.tensor(sc, device=DEV, requires_grad=True)
    L.compute_loss_with_score(crit, half * 1.0)[0].backward()
    assert maxdiff(half.grad, d64) <= GRAD_ABS


def test_empty_batch_is_accepted_by_both_entry_points():
    from laff_amd import ops
    loss, d_s, d_im = ops.dsl_loss(torch.empty((0, 2, 8), device=DEV), torch.empty((0, 2, 8), device=DEV))
    assert loss.item() == 0.0 and d_s.shape == (0, 2, 8) and d_im.shape == (0, 2, 8)
    loss, d = ops.margin_loss_scores(torch.empty((0, 0), device=DEV), 0.2)
    assert loss.item() == 0.0 and d.shape == (0, 0)


# ---------------------------------------------------------------------------------------------- margin ranking loss from embeddings
# what each shape reaches; the staging kind of the grouped GEMM follows K (d for the scores, B for the gradients): kind 2 takes K * 4 a
# multiple of 128 bytes, kind 1 any other multiple of 4, kind 0 the rest
MARGIN_SHAPES = [(1, 1, 8),         # a single pair: loss exactly 0, gradients exactly 0
                 (2, 3, 5),         # the smallest real case, dp = 8 > d, heads != 1
                 (17, 2, 36),       # one row more than the reduction's 16 waves; scores kind 1, gradients kind 0
                 (63, 1, 36), (64, 2, 64), (65, 1, 30),       # either side of one wavefront; (64, 2, 64) is kind 2 for both GEMMs
                 (68, 3, 36),       # kind 1 for both GEMMs, three heads in one group
                 (130, 2, 30),      # Bp = 132 > B and dp = 32 > d, kind 0 for both
                 (257, 1, 64),      # one row past 256; gradients kind 0 with K = 257
                 (64, 8, 128),      # eight heads: the per-head offsets of every buffer
                 (257, 2, 260)]     # the largest; several K-steps in both GEMMs
MARGIN = 0.2
MIN_ACTIVE = 0.1                    # share of the off-diagonal pairs with a positive 'i2t' hinge argument, per head, at B >= 17

# test_margin_loss_vs_float64 prints, per case, the loss and its error, the largest gradient entry and the largest error / bound ratio of
# any gradient element.  MEASURED on the MI355X: not measured yet.  On the CPU a strictly sequential fp32 emulation of the chain (the worst
# summation order, tests/test_losses_host.py) reaches 0.8 % to 2.7 % of the bound at (65, 1, 30) and (130, 2, 30).


@functools.lru_cache(maxsize=None)
def _margin_inputs(B, H, d):
    """(s, im), fp32 (B, H, d): the correlated construction of _inputs with noise 6.0, so that many hinges are active, and with every
    decision of every head >= 1e-4 from flipping in float64 at margin 0.2 under max_violation and 'bidir' -- the strictest of the
    twelve flag combinations, so one input serves them all.  1e-4 is 25 times twice the fp32 score contract (PREC_TOL['fp32'] = 2e-6):
    the fp32 kernel takes every decision as float64 does.  The caption indices with a pair that _too_close reports are drawn again (both
    rows, a fresh latent), 100 times at the most; the caller asserts the result with loss_ref.margin_scores_slack."""
    g = np.random.default_rng(B + H + d)
    P = g.normal(0, 1, (16, H * d)).astype(np.float32)

    def draw(n):
        z = g.normal(0, 1, (n, 16)).astype(np.float32)
        return [(z @ P + 6.0 * g.normal(0, 1, (n, H * d))).astype(np.float32).reshape(n, H, d) for _ in range(2)]

    s, im = draw(B)
    for _ in range(100):
        marked = np.zeros(B, bool)
        for h in range(H):
            bad = _too_close(margin_scores64(s, im, h), MARGIN, True, 'bidir')
            marked |= bad.any(axis=0)
        if not marked.any():
            s.setflags(write=False)
            im.setflags(write=False)
            return s, im
        s[marked], im[marked] = draw(int(marked.sum()))
    raise AssertionError('(%d, %d, %d): pairs within 1e-4 of a decision are left after 100 rounds' % (B, H, d))


def margin_scores64(s, im, h):
    """The float64 score matrix of head h: rows = videos, columns = captions."""
    sh = loss_ref._l2norm(np.asarray(s[:, h], np.float64))[0]
    ih = loss_ref._l2norm(np.asarray(im[:, h], np.float64))[0]
    return ih @ sh.T


def margin_active_share(S):
    """The share of the off-diagonal pairs of S whose 'i2t' hinge argument is positive."""
    off = ~np.eye(S.shape[0], dtype=bool)
    return float(((MARGIN + S - np.diag(S)[:, None])[off] > 0.0).mean())


@functools.lru_cache(maxsize=None)
def _margin_case(B, H, d, maxv, style, direction):
    """Inputs, the float64 reference and the element-wise bounds of one case: computed once, never written to."""
    s, im = _margin_inputs(B, H, d)
    out = loss_ref.margin(s, im, MARGIN, maxv, style, direction)
    for a in out[1:]:
        a.setflags(write=False)
    return (s, im) + out


def _margin_raw(s, im, maxv, style, direction, want_s=True, want_im=True):
    """laff_margin_loss through the binding with the workspace and every output buffer NaN before the launch."""
    import ctypes as C
    from laff_amd import ops
    B, H, d = s.shape
    lib, h = ops._context(s.device)
    nbytes = ops._size_query('laff_margin_loss_workspace_bytes', B, H, d)
    ws = _nan_like((nbytes // 4,))
    loss = _nan_like(())
    d_s = _nan_like(tuple(s.shape)) if want_s else None
    d_im = _nan_like(tuple(s.shape)) if want_im else None
    F = ops.LOSS_FLAGS
    flags = (F['max_violation'] if maxv else 0) | (F['mean'] if style == 'mean' else 0)
    flags |= {'i2t': F['i2t'], 't2i': F['t2i'], 'bidir': F['i2t'] | F['t2i']}[direction]
    ops.check(lib.laff_margin_loss(h, ops._ptr(s), ops._ptr(im), B, H, d, MARGIN, flags, ops._ptr(loss), ops._ptr(d_s), ops._ptr(d_im),
                                   ops._ptr(ws), C.c_size_t(nbytes)))
    return loss, d_s, d_im


@pytest.mark.parametrize('maxv,style,direction', FLAGS)
@pytest.mark.parametrize('B,H,d', MARGIN_SHAPES)
def test_margin_loss_vs_float64(B, H, d, maxv, style, direction):
    """All five launches of laff_margin_loss against loss_ref.margin, every gradient element inside its derived fp32 rounding bound."""
    s, im, l64, ds64, di64, b_s, b_im = _margin_case(B, H, d, maxv, style, direction)
    # in float64, before the launch: every decision is clear and many hinges are active
    for h in range(H):
        S = margin_scores64(s, im, h)
        assert loss_ref.margin_scores_slack(S, MARGIN, maxv, direction) >= 1e-4, h
        assert B < 17 or margin_active_share(S) >= MIN_ACTIVE, h
    ds, di = dev(s), dev(im)
    loss, d_s, d_im = _margin_raw(ds, di, maxv, style, direction)
    got_s, got_i = d_s.cpu().numpy().astype(np.float64), d_im.cpu().numpy().astype(np.float64)
    e_s, e_i = np.abs(got_s - ds64), np.abs(got_i - di64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = max(np.nan_to_num(np.where(b > 0, e / b, 0.0)).max() for e, b in ((e_s, b_s), (e_i, b_im)))
    print('margin B=%d H=%d d=%d maxv=%d %s %s: loss %.9g err %.3g (rel %.3g)  grad max %.3g  worst err/bound %.3g'
          % (B, H, d, maxv, style, direction, l64, abs(loss.item() - l64), abs(loss.item() - l64) / max(1.0, abs(l64)),
             max(np.abs(ds64).max(), np.abs(di64).max()), ratio))
    assert np.isfinite(loss.item()) and torch.isfinite(d_s).all() and torch.isfinite(d_im).all()
    assert abs(loss.item() - l64) <= LOSS_REL * max(1.0, abs(l64)), (loss.item(), l64)
    assert (e_s <= b_s).all(), ('d_s', float(np.where(e_s > b_s, e_s, 0).max()), int((e_s > b_s).sum()), ratio)
    assert (e_i <= b_im).all(), ('d_im', float(np.where(e_i > b_im, e_i, 0).max()), int((e_i > b_im).sum()), ratio)
    if B == 1:
        assert loss.item() == 0.0 and not d_s.any() and not d_im.any()
    # forward only, and each gradient alone (the other pointer null): bit for bit the two-sided call
    l0, a, b = _margin_raw(ds, di, maxv, style, direction, want_s=False, want_im=False)
    assert a is None and b is None and l0.item() == loss.item()
    l1, a, b = _margin_raw(ds, di, maxv, style, direction, want_im=False)
    assert b is None and l1.item() == loss.item() and torch.equal(a, d_s)
    l2, a, b = _margin_raw(ds, di, maxv, style, direction, want_s=False)
    assert a is None and l2.item() == loss.item() and torch.equal(b, d_im)
