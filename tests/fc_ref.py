"""Plain references for the FC projections (TransformNet.forward, eval mode): numpy for the hi/lo operand split, torch float64 for
the products.  No project code in here; tests/test_fc_ref.py shows on the CPU that these references and the tolerances below can tell
a right kernel from a subtly wrong one, tests/test_gpu_fc_routes.py holds every FC route of the library against them.

The documented split (include/laff_hip.h, laff_split_rows): per row, e = the binary exponent of the largest finite-or-infinite
magnitude, read from its bits (NaNs are skipped, as fmaxf skips them); e = 0 for a row whose maximum is zero or infinite, and e is
clamped at -100 from below; s = 2^(9 - e), so the row maximum lands in [512, 1024); hi = float16(x s), lo = float16(x s - hi), both
rounded to nearest even; the planes are Kp = ceil(K / 64) * 64 wide, zero beyond K; rscale = 2^(e - 9) = 1 / s exactly.
"""
import numpy as np
import torch

U = 2.0 ** -24          # the unit of the normalised errors: half an fp32 ulp of 1

# ---- tolerances of tests/test_gpu_fc_routes.py -----------------------------------------------------------------------------------
# Normalised error e = |got - ref| / (2^-24 * absdot), absdot = (sum_k |x_k w_k| + |bias|) |bn_scale| + |bn_shift| per element.
# MEASURED on an MI355X (256 CUs) over the whole CASES table against the float64 references below -- never against another kernel --
# and set to 4 x the maximum, rounded up to one significant digit (the factor covers other boxes and seeds).  Each one is kept only
# because test_fc_ref.py shows it at least 10 x below what eight deliberately wrong kernels produce.
# Maxima of e against fc_exact64 per route and Dk (activation None or relu):
MEASURED = {
    'F32_REG': {77: 3.39, 512: 4.30},
    'F32_TAIL': {100: 1.20, 512: 5.49, 516: 4.14},
    'F32_GLDS': {32: 2.90, 512: 5.52, 2048: 5.21, 2080: 4.10, 4096: 4.23},
    'F16_128': {77: 1.69, 512: 2.25, 1030: 1.36},
    'X3': {96: 3.98, 512: 4.33},
    'X3_FUSED': {32: 3.48, 512: 3.23, 2048: 3.85, 2080: 3.75},
}
EXACT_TOL = {'F32_REG': 20.0, 'F32_TAIL': 30.0, 'F32_GLDS': 30.0, 'F16_128': 9.0, 'X3': 20.0, 'X3_FUSED': 20.0}
# e against fc_contract64 (the fp32 x and W themselves): adds the 2^-22-class error of the dropped lo * lo term and of lo's rounding.
# Measured maxima: fp32 5.52, split 4.36, fused 3.87.
CONTRACT_TOL = {'fp32': 30.0, 'split': 20.0, 'fused': 20.0}
# |got - act64(ref)| absolute for tanh / sigmoid, BatchNorm scales in [0.5, 1.5], on entries whose pre-activation absdot is at most
# ACT_ABSDOT_MAX.  Measured maxima: tanh 3.48e-6 (f32_glds_many), sigmoid 1.63e-6 (fused_dk4096): the pre-activation's error through a
# slope <= 1 (<= 1/4), far above fast_tanh's own 2.4e-7 (gemm_nt.hip), which shows alone where absdot is small (N = 1, Dk = 36: 9e-8).
ACT_TOL = {'tanh': 2e-5, 'sigmoid': 7e-6}
ACT_ABSDOT_MAX = 64.0          # sum |x w| + |bias| of N(0, 1) inputs is 0.64 sqrt(Dk) + 0.1: 41 at Dk = 4096

ACTS = (None, 'tanh', 'relu', 'sigmoid')


def split_ref(x):
    """x (N, K) float32 (numpy) -> hi, lo (N, Kp) float16, rscale (N,) float32, exponent (N,) int: the documented split."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, K = x.shape
    Kp = -(-K // 64) * 64
    m = np.fmax.reduce(np.abs(x), axis=1, initial=np.float32(0)).astype(np.float32)       # fmax: a NaN never wins
    be = ((m.view(np.uint32) >> 23) & 0xff).astype(np.int64)
    e = np.where((m > 0) & (be != 0xff), np.maximum(be - 127, -100), 0)
    s = np.ldexp(np.float32(1), (9 - e).astype(np.int32)).astype(np.float32)
    hi = np.zeros((N, Kp), np.float16)
    lo = np.zeros((N, Kp), np.float16)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        t = (x * s[:, None]).astype(np.float32)
        h = t.astype(np.float16)
        hi[:, :K] = h
        lo[:, :K] = (t - h.astype(np.float32)).astype(np.float16)
    rscale = np.ldexp(np.float32(1), (e - 9).astype(np.int32)).astype(np.float32)
    return hi, lo, rscale, e


def split_ref_t(x):
    """split_ref in torch, for matrices that live on a device: x (N, K) float32 -> hi, lo (N, Kp) float16, rscale (N,) float32."""
    N, K = x.shape
    Kp = -(-K // 64) * 64
    a = x.abs()
    m = torch.where(a.isnan(), torch.zeros_like(a), a).amax(1) if K else x.new_zeros(N)
    be = (m.view(torch.int32) >> 23) & 0xff
    e = torch.where((m > 0) & (be != 0xff), (be - 127).clamp(min=-100), torch.zeros_like(be))
    one = torch.ones_like(m)
    s = torch.ldexp(one, 9 - e)
    t = x * s[:, None]
    h = t.half()
    hi = torch.zeros((N, Kp), dtype=torch.float16, device=x.device)
    lo = torch.zeros((N, Kp), dtype=torch.float16, device=x.device)
    hi[:, :K] = h
    lo[:, :K] = (t - h.float()).half()
    return hi, lo, torch.ldexp(one, e - 9)


def act64(pre, act):
    if act in (None, '', 'none'):
        return pre
    if act == 'tanh':
        return torch.tanh(pre)
    if act == 'relu':
        return torch.relu(pre)
    if act == 'sigmoid':
        return torch.sigmoid(pre)
    raise ValueError(act)


def epilogue64(prod, bias=None, act=None, bn_scale=None, bn_shift=None):
    """act(prod + bias) * bn_scale + bn_shift in float64 (absent stages skipped)."""
    y = prod if bias is None else prod + bias.double()[None, :]
    y = act64(y, act)
    if bn_scale is not None:
        y = y * bn_scale.double()[None, :] + bn_shift.double()[None, :]
    return y


def fc_contract64(x, w, bias=None, act=None, bn_scale=None, bn_shift=None):
    """The user-facing contract: float64 all the way from the fp32 x (N, K) and W (D, K)."""
    return epilogue64(x.double() @ w.double().T, bias, act, bn_scale, bn_shift)


def fc_exact64(xo, wo, bias=None, act=None, bn_scale=None, bn_shift=None):
    """The float64 result from the operands the kernel forms.  xo / wo: an fp32 matrix (the fp32 routes: the same as fc_contract64), or
    (hi, lo, rscale) of the split routes: (lo hi' + hi lo' + hi hi') rscale_x rscale_w, the three products the kernel adds up."""
    if torch.is_tensor(xo):
        return fc_contract64(xo, wo, bias, act, bn_scale, bn_shift)
    xh, xl, xr = xo
    wh, wl, wr = wo
    xh, xl, wh, wl = xh.double(), xl.double(), wh.double(), wl.double()
    prod = torch.cat([xl, xh, xh], 1) @ torch.cat([wh, wl, wh], 1).T
    return epilogue64(prod * xr.double()[:, None] * wr.double()[None, :], bias, act, bn_scale, bn_shift)


def absdot(x, w, bias=None, bn_scale=None, bn_shift=None):
    """The magnitude the rounding errors of one output element scale with: (sum_k |x_k w_k| + |bias|) |bn_scale| + |bn_shift|."""
    a = x.double().abs() @ w.double().abs().T
    if bias is not None:
        a = a + bias.double().abs()[None, :]
    if bn_scale is not None:
        a = a * bn_scale.double().abs()[None, :] + bn_shift.double().abs()[None, :]
    return a


ACT_SLOPE = {'tanh': 1.0, 'sigmoid': 0.25}          # the largest derivative


def absdot_act(x, w, bias=None, act=None, bn_scale=None, bn_shift=None):
    """absdot for an output that went through `act`.  None and relu pass the pre-activation's error on unchanged (or drop it): absdot
    itself.  tanh and sigmoid pass it on through a slope of at most ACT_SLOPE and add the rounding of their own result, which is of
    magnitude up to 1 whatever the pre-activation was: (max(slope (sum_k |x_k w_k| + |bias|), 1)) |bn_scale| + |bn_shift|.  The floor
    of 1 matters only where absdot is tiny (zero or 1e-6 rows, Dk = 32 under sigmoid); N(0, 1) rows have 0.64 sqrt(Dk) >= 3.6."""
    if act not in ACT_SLOPE:
        return absdot(x, w, bias, bn_scale, bn_shift)
    a = (absdot(x, w, bias) * ACT_SLOPE[act]).clamp(min=1.0)
    if bn_scale is not None:
        a = a * bn_scale.double().abs()[None, :] + bn_shift.double().abs()[None, :]
    return a


def norm_err(got, ref, ad):
    """max over the finite reference entries of |got - ref| / (2^-24 absdot); rows whose absdot is zero must match exactly."""
    ok = torch.isfinite(ref) & torch.isfinite(ad)
    d = (got.double() - ref).abs()
    e = torch.where(ad > 0, d / (U * ad), torch.where(d > 0, torch.full_like(d, float('inf')), torch.zeros_like(d)))
    e = torch.where(ok, e, torch.zeros_like(e))
    return float(e.max()) if e.numel() else 0.0


# ---- the inputs of the GPU suite (and of the sensitivity tests, which must judge the tolerances on the same data) -------------------
PLANT_MIN_ROWS = 1000
PLANTS = ('zero', 'x3e4', 'x1e-6', 'tiny', 'inf', 'nan')


def plant_rows(x, rows):
    """Plants the six edge rows of the split into x (torch, in place) at `rows`: all zero, scaled by 3e4 and by 1e-6, largest magnitude
    2^-105 (below the exponent clamp), one inf, one NaN."""
    K = x.shape[1]
    r = dict(zip(PLANTS, rows))
    x[r['zero']] = 0
    x[r['x3e4']] *= 3e4
    x[r['x1e-6']] *= 1e-6
    x[r['tiny']] = x[r['tiny']].clamp(-1, 1) * 2.0 ** -105
    x[r['tiny'], K // 2] = 2.0 ** -105
    x[r['inf'], K // 3] = float('inf')
    x[r['nan'], (2 * K) // 3] = float('nan')
    return x


def plant_positions(N):
    """Rows of the six plants in an N-row input: spread over the row tiles, the last row among them."""
    return [1, N // 5, N // 3 + 1, N // 2 + 2, (3 * N) // 4, N - 1]


def make_problem(N, Dk, D, seed, bias=True, bn=True, plant=False, device='cpu'):
    """x ~ N(0, 1) (N, Dk), W ~ N(0, 1 / Dk) (D, Dk), bias ~ N(0, 0.1^2), BatchNorm scale in [0.5, 1.5] and shift in [-0.5, 0.5]: the
    pre-activation is N(0, 1.01), so |pre| > 3 for 0.29 % of the entries (tests/test_fc_ref.py counts them) and tanh / sigmoid stay
    where they still pass errors on.  With `plant` (N >= PLANT_MIN_ROWS only: three of the six planted rows saturate, 0.3 % of a
    thousand) the six edge rows of plant_rows are put in.  Generated on the CPU so that every device sees the same data."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Dk, generator=g)
    w = torch.randn(D, Dk, generator=g) / float(Dk) ** 0.5
    b = 0.1 * torch.randn(D, generator=g) if bias else None
    sc = 0.5 + torch.rand(D, generator=g) if bn else None
    sh = torch.rand(D, generator=g) - 0.5 if bn else None
    if plant:
        assert N >= PLANT_MIN_ROWS
        plant_rows(x, plant_positions(N))
    mv = lambda t: None if t is None else t.to(device)
    return mv(x), mv(w), mv(b), mv(sc), mv(sh)
