"""The 'hist' measure (generalised Jaccard / histogram intersection) restated in float64 numpy from its formula:

    J(t, v) = sum_k min(t_k, v_k) / (sum_k max(t_k, v_k) + eps);   S[t, v] = mean over heads of J(T[t, h, :], V[v, h, :])

and the reader of its fixture, tests/golden/hist_sim*.npz (tools/gen_golden_hist.py writes it)."""
import glob
import os

import numpy as np

#: (Nt, Nv, K = H d, H) of the fixture, in its order
CASES = [(1, 1, 1, 1), (5, 7, 3, 1), (65, 130, 37, 1), (130, 65, 515, 1), (33, 129, 111, 3), (64, 257, 128, 8), (257, 64, 512, 1),
         (70, 50, 3981, 1)]
KINDS = ('sigmoid', 'bow', 'signed')
EPS = 1e-8            # the eps the fixture was made with (loss.jaccard_sim's default)


def case_name(c):
    return 't%dv%dk%dh%d' % tuple(c)


def kinds_of(c):
    """'signed' only where a head has at least 16 elements"""
    return KINDS if c[2] // c[3] >= 16 else KINDS[:2]


def hist_sim(T, V, heads=1, eps=EPS):
    """float64 S [Nt, Nv] of T [Nt, H d] (or [Nt, H, d]) against V; one text row at a time, so nothing larger than Nv x K is formed"""
    T, V = np.asarray(T, dtype=np.float64), np.asarray(V, dtype=np.float64)
    if T.ndim == 3:
        heads = T.shape[1]
    T, V = T.reshape(T.shape[0], heads, -1), V.reshape(V.shape[0], heads, -1)
    S = np.empty((T.shape[0], V.shape[0]), dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, t in enumerate(T):
            S[i] = (np.minimum(t[None], V).sum(-1) / (np.maximum(t[None], V).sum(-1) + eps)).mean(-1)
    return S


def load_fixture(golden_dir):
    """{key: array} of the fixture.  It is written as several files of less than 1 MiB each (hist_sim.npz, hist_sim.1.npz, ...); an
    array too large for one file is stored as row blocks 'key#0', 'key#1', ... which are joined here."""
    parts = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, 'hist_sim*.npz'))):
        with np.load(path) as z:
            for k in z.files:
                parts[k] = z[k]
    out, blocks = {}, {}
    for k, a in parts.items():
        if '#' in k:
            name, i = k.split('#')
            blocks.setdefault(name, {})[int(i)] = a
        else:
            out[k] = a
    for name, b in blocks.items():
        out[name] = np.concatenate([b[i] for i in range(len(b))], axis=0)
    return out
