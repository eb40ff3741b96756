"""float64 restatement of the optimizer step of DESIGN.md 4.21 in numpy: the global gradient norm, the clip coefficient, Adam and
RMSprop (momentum 0, not centered) in torch's order, and the element-by-element error bounds the device tests apply.

Every function takes lists of arrays (one per tensor) and evaluates in float64 whatever the inputs' type is."""
import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32


def f64(ts):
    return [np.asarray(t, dtype=np.float64) for t in ts]


def total_norm(grads):
    """sqrt(sum over every element of g^2)."""
    return float(np.sqrt(sum(float(np.sum(g * g)) for g in f64(grads))))


def clip_coef(total, max_norm):
    """torch.clamp(max_norm / (total + 1e-6), max=1); 1 when max_norm <= 0 (no clipping).  NaN stays NaN."""
    if not max_norm > 0:
        return 1.0
    r = max_norm / (total + 1e-6)
    return 1.0 if r > 1.0 else r


def clipped(grads, c, params=None, wd=0.0):
    """gh = c g (+ wd p)."""
    out = [c * g for g in f64(grads)]
    if wd != 0.0:
        out = [g + wd * p for g, p in zip(out, f64(params))]
    return out


def adam(params, grads, m, v, lr, beta1, beta2, eps, wd, step, c=1.0):
    """One Adam step: (p', m', v')."""
    gh = clipped(grads, c, params, wd)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    m2 = [a + (g - a) * (1.0 - beta1) for a, g in zip(f64(m), gh)]
    v2 = [beta2 * a + (1.0 - beta2) * g * g for a, g in zip(f64(v), gh)]
    p2 = adam_param(params, m2, v2, lr, beta1, beta2, eps, step)
    return p2, m2, v2


def adam_param(params, m2, v2, lr, beta1, beta2, eps, step):
    """The last stage alone, from given new moments: p - (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return [p - (lr / bc1) * (a / (np.sqrt(b) / np.sqrt(bc2) + eps)) for p, a, b in zip(f64(params), f64(m2), f64(v2))]


def rmsprop(params, grads, s, lr, alpha, eps, wd, c=1.0):
    """One RMSprop step: (p', s')."""
    gh = clipped(grads, c, params, wd)
    s2 = [alpha * a + (1.0 - alpha) * g * g for a, g in zip(f64(s), gh)]
    return rmsprop_param(params, gh, s2, lr, eps), s2


def rmsprop_param(params, gh, s2, lr, eps):
    return [p - lr * (g / (np.sqrt(b) + eps)) for p, g, b in zip(f64(params), f64(gh), f64(s2))]


# ---- the bounds of tests/test_gpu_optim.py, element by element ----------------------------------------------------------------------
# fp32 arithmetic, one rounding (relative error <= U, first order) per operation of the kernel's sequence in laff_amd/csrc/optim.hip; a
# constant of the launch that is rounded from float64 (1 - beta, beta2, eps, wd, lr, bc1, bc2) counts one more.  c carries 2 U: the
# float64 value rounded once, after a float64 norm.  With G = |c g| + |wd p| >= |gh|:
#   gh = c g + wd p         c 2, the product 1: 3 U |c g|;  wd 1, the product 1: 2 U |wd p|;  the sum 1 on both     ->  <= 4 U G
#   m' = m + (gh - m) w     gh's 4 U w G;  the difference, w = fl(1 - beta1) and the product: 3 U w (G + |m|);  the sum: U (|m| + w G)
#                           = 8 U w G + (1 + 3 w) U |m|                                                             ->  <= 10 U (|m| + w G)
#   v' = b v + (w gh) gh    b and the product: 2 U b v;  w, two products and gh twice: 11 U w G^2;  the sum 1       ->  <= 14 U (b v + w G^2)
#   p' from the device's own m', v':  sqrt 1, fl(bc2) 1/2 and its sqrt 1, the division 1: 3.5 U on sqrt(v') / sqrt(bc2);  fl(eps) 1 on
#                           eps;  their sum 1: 4.5 U on the denominator;  the quotient 1;  fl(lr), fl(bc1), lr / bc1: 3;  the product 1
#                           = 9.5 U |Delta|, inside the 13 U |Delta| of the bound;  the subtraction is the U |p'| term.
#   RMSprop's p':           gh's 4;  sqrt, fl(eps) and the sum: <= 3 on the denominator;  the quotient 1;  fl(lr) 1;  the product 1
#                           = 10 U lr G / (sqrt(s') + eps), inside 13.
#   clip_grad_norm_'s c g:  c 2, the product 1                                                                      ->  3 U |c g|
M_CONST, V_CONST, P_CONST, CLIP_CONST = 10.0, 14.0, 13.0, 3.0


def gmag(params, grads, c, wd):
    return [abs(c) * np.abs(g) + abs(wd) * np.abs(p) for g, p in zip(f64(grads), f64(params))]


def bound_m(m, G, beta1):
    return [M_CONST * U * (np.abs(a) + (1.0 - beta1) * g) for a, g in zip(f64(m), G)]


def bound_v(v, G, beta2):
    return [V_CONST * U * (beta2 * a + (1.0 - beta2) * g * g) for a, g in zip(f64(v), G)]


def bound_p_adam(ref_p, m2, v2, lr, beta1, beta2, eps, step):
    zero = [np.zeros_like(a) for a in f64(m2)]
    delta = adam_param(zero, [np.abs(a) for a in f64(m2)], v2, lr, beta1, beta2, eps, step)       # -|Delta|
    return [U * np.abs(r) + P_CONST * U * np.abs(d) for r, d in zip(ref_p, delta)]


def bound_p_rmsprop(ref_p, G, s2, lr, eps):
    return [U * np.abs(r) + P_CONST * U * lr * g / (np.sqrt(b) + eps) for r, g, b in zip(ref_p, G, f64(s2))]
