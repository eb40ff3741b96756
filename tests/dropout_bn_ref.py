"""Host restatement of laff_dropout_bn_train and its backward: the Philox4x32-10 dropout mask in numpy, and the forward
and backward formulas in float64.  The mask is a function of (seed, row, column) alone, so the reference takes it as an exact input."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# the generator's published known-answer vectors: (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """Ten rounds on uint32 arrays (or scalars) of one shape: counter = (c0, c1, c2, c3), key = (k0, k1); returns the four words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK32, p1 >> 32, p1 & MASK32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def philox_scalar(counter, key):
    """The same in plain Python integers, one call."""
    c, (k0, k1) = [int(x) for x in counter], key
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK32, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def threshold(p):
    """An element is kept iff its word >= floor(p 2^32), in double."""
    return int(np.floor(float(p) * 4294967296.0))


def key_of(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF                  # an int64 tensor's value is read as the unsigned word it is
    return seed & MASK32, seed >> 32


def keep_mask(seed, N, D, p):
    """[N, D] bool: element (n, c) takes word c & 3 of Philox(counter (c >> 2, n, 0, 0), key (seed lo, seed hi))."""
    if p == 0:
        return np.ones((N, D), dtype=bool)
    n, g = np.meshgrid(np.arange(N, dtype=np.uint64), np.arange((D + 3) // 4, dtype=np.uint64), indexing='ij')
    words = np.stack(philox4x32_10((g, n, 0, 0), key_of(seed)), axis=-1).reshape(N, -1)[:, :D]
    return words >= np.uint32(threshold(p))


def keep_scalar(seed, n, c, p):
    return philox_scalar((c >> 2, n, 0, 0), key_of(seed))[c & 3] >= threshold(p)


def scale32(p):
    """What a kept element is multiplied by on the device: 1 / (1 - p) formed in double and rounded to fp32 once."""
    return np.float32(1.0 / (1.0 - float(p)))


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def forward(a, keep, p, gamma=None, beta=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """float64: dict(u, y, and with a BatchNorm stage mean, invstd, running_mean, running_var)."""
    a = _f64(a)
    u = a * keep / (1.0 - p)
    if gamma is None:
        return dict(u=u, y=u)
    N = a.shape[0]
    gamma, beta = _f64(gamma), _f64(beta)
    mean = u.sum(0) / N
    var = ((u - mean) ** 2).sum(0) / N
    invstd = 1.0 / np.sqrt(var + eps)
    return dict(u=u, y=gamma * (u - mean) * invstd + beta, mean=mean, invstd=invstd,
                running_mean=(1.0 - momentum) * _f64(running_mean) + momentum * mean,
                running_var=(1.0 - momentum) * _f64(running_var) + momentum * var * N / (N - 1))


def backward(dy, a, keep, p, gamma=None, mean=None, invstd=None):
    """float64 (da, dgamma, dbeta) from the saved statistics as they are handed in; (da, None, None) without a BatchNorm stage."""
    dy, a = _f64(dy), _f64(a)
    m = keep / (1.0 - p)
    if gamma is None:
        return dy * m, None, None
    N = a.shape[0]
    gamma, mean, invstd = _f64(gamma), _f64(mean), _f64(invstd)
    xhat = (a * m - mean) * invstd
    dbeta, dgamma = dy.sum(0), (dy * xhat).sum(0)
    du = gamma * invstd * (dy - dbeta / N - xhat * dgamma / N)
    return du * m, dgamma, dbeta


def rel_err(got, ref):
    """max |got - ref| / max |ref|; a reference that is zero throughout admits only zeros."""
    got, ref = _f64(got).reshape(-1), _f64(ref).reshape(-1)
    if ref.size == 0:
        return 0.0
    top, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
    if top == 0.0:
        return 0.0 if err == 0.0 else float('inf')
    return err / top
