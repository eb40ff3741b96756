#!/usr/bin/env python3
"""Golden vectors for the 'hist' measure (tests/golden/hist_sim*.npz), from the REAL reference.

Runs only in the build container: it imports the reference's loss.py (no stubs needed) and calls its own jaccard_sim per head on
seeded fp32 inputs -- once in fp32 (out32, heads averaged in fp32) and once on float64 copies of the same fp32 inputs (out64);
e_ref = max |out32 - out64| is the reference's own rounding error.  Arrays and scalars only are written.

Cases (tests/hist_ref.py: CASES) x input kinds:
    sigmoid   both sides sigmoid(N(0, 1.5)): concept scores
    bow       texts: sparse counts (5 % density, values 1..3); videos: sigmoid(N(-2, 2))
    signed    N(0.5, 0.5) on both sides, cases with d >= 16 only; the seed is advanced until every pair and head has
              |sum max| >= (sum |t| + sum |v|) / 8, which keeps the division well conditioned

Random fp32 data does not compress, and a committed file stays below 1 MiB: the arrays go greedily into hist_sim.npz, hist_sim.1.npz,
... by their compressed size, an array too large for one file as row blocks 'key#i' (tests/hist_ref.py: load_fixture joins them).

    python tools/gen_golden_hist.py
"""
import glob
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.environ.get('LAFF_REFERENCE', '/root/reference'))
import hist_ref as R  # noqa: E402
import loss as ref_loss  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
FILE_BYTES = 900 << 10           # compressed payload per file
BLOCK_BYTES = 400 << 10          # raw bytes of a row block


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def inputs(kind, g, Nt, Nv, K):
    if kind == 'sigmoid':
        T, V = sigmoid(g.normal(0, 1.5, (Nt, K))), sigmoid(g.normal(0, 1.5, (Nv, K)))
    elif kind == 'bow':
        T = (g.random((Nt, K)) < 0.05) * g.integers(1, 4, (Nt, K))
        V = sigmoid(g.normal(-2, 2, (Nv, K)))
    else:
        T, V = g.normal(0.5, 0.5, (Nt, K)), g.normal(0.5, 0.5, (Nv, K))
    return np.ascontiguousarray(T, dtype=np.float32), np.ascontiguousarray(V, dtype=np.float32)


def reference(T, V, H, dtype):
    """mean over heads of the reference's jaccard_sim (model/model.py:1008-1014 around loss.py:53-65), in `dtype`"""
    t, v = torch.as_tensor(T).to(dtype).view(T.shape[0], H, -1), torch.as_tensor(V).to(dtype).view(V.shape[0], H, -1)
    return torch.stack([ref_loss.jaccard_sim(t[:, h], v[:, h], eps=R.EPS) for h in range(H)], dim=0).mean(dim=0).numpy()


def well_conditioned(T, V, H):
    t, v = T.astype(np.float64).reshape(T.shape[0], H, -1), V.astype(np.float64).reshape(V.shape[0], H, -1)
    for row in t:
        union = np.abs(np.maximum(row[None], v).sum(-1))
        if (union < (np.abs(row).sum(-1)[None] + np.abs(v).sum(-1)) / 8).any():
            return False
    return True


def write(arrays):
    for old in glob.glob(os.path.join(OUT, 'hist_sim*.npz')):
        os.remove(old)
    pieces = []
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= BLOCK_BYTES:
            pieces.append((k, a))
            continue
        rows = max(1, BLOCK_BYTES // (a.nbytes // a.shape[0]))
        pieces += [('%s#%d' % (k, i), a[r:r + rows]) for i, r in enumerate(range(0, a.shape[0], rows))]
    files, used = [{}], 0
    for k, a in pieces:
        n = len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + 256
        if used + n > FILE_BYTES and files[-1]:
            files.append({})
            used = 0
        files[-1][k] = a
        used += n
    for i, f in enumerate(files):
        path = os.path.join(OUT, 'hist_sim%s.npz' % ('.%d' % i if i else ''))
        np.savez_compressed(path, **f)
        assert os.path.getsize(path) < (1 << 20), path
        print('wrote %s (%.1f KB, %d arrays)' % (path, os.path.getsize(path) / 1024, len(f)))


def main():
    arrays = {}
    for ci, c in enumerate(R.CASES):
        Nt, Nv, K, H = c
        for ki, kind in enumerate(R.kinds_of(c)):
            for seed in range(1000):
                T, V = inputs(kind, np.random.default_rng(100000 * ci + 1000 * ki + seed), Nt, Nv, K)
                if kind != 'signed' or well_conditioned(T, V, H):
                    break
            else:
                raise SystemExit('%s %s: no well-conditioned seed' % (R.case_name(c), kind))
            out32, out64 = reference(T, V, H, torch.float32), reference(T, V, H, torch.float64)
            e_ref = float(np.abs(out32 - out64).max())
            assert out32.dtype == np.float32 and out64.dtype == np.float64 and out32.shape == out64.shape == (Nt, Nv)
            assert e_ref <= 1e-6, (c, kind, e_ref)
            print('%-18s %-8s seed %2d  e_ref %.2e  mean %.3f' % (R.case_name(c), kind, seed, e_ref, float(out64.mean())))
            p = '%s/%s/' % (R.case_name(c), kind)
            arrays.update({p + 'T': T, p + 'V': V, p + 'out32': out32, p + 'out64': out64, p + 'e_ref': np.float64(e_ref),
                           p + 'params': np.array(c, dtype=np.int64)})
    write(arrays)


if __name__ == '__main__':
    main()
