#!/usr/bin/env python3
"""Golden vectors for the re-ranking functions (tests/golden/rerank.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden) and calls the
reference's own model/ReRank.py re_ranking and re_ranking_tkb_simple on seeded fp32 similarity blocks built from cluster-planted unit
embeddings.  Every case is run twice: on the fp32 blocks as they are, and on float64 copies with the reference's internal buffers
widened too (its `np.float32` / `torch.Tensor` resolve to float64 for that run: the module sees a numpy / torch proxy); e_ref is the
largest difference between the two.  Arrays and scalars only are written.

A case is accepted only when it sits on no tie: in every row of D the k1 + 2 smallest values differ pairwise by at least 1e-6 (the
same for the neighbour-count lists), and the two runs agree to 1e-6.  The seed of a case is advanced until that holds.

    python tools/gen_golden_rerank.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import rerank_ref as R  # noqa: E402
from model import ReRank as ref_rr  # noqa: E402

#: name -> (Q, G, k1, k2, non-symmetric gg)
CASES = {
    'q1g40k5': (1, 40, 5, 3, False),          # half-even rounding 2.5 -> 2
    'q3g70k6': (3, 70, 6, 1, False),          # the k2 = 1 branch
    'q2g60k7': (2, 60, 7, 2, False),          # half-even rounding 3.5 -> 4
    'q5g130k20': (5, 130, 20, 6, False),      # the reference's default k1 and k2
    'q2g50k6asym': (2, 50, 6, 3, True),       # gg[a, b] != gg[b, a]: pins the transpose
}
MIN_GAP = 1e-6
DIM = 24


class _Numpy64:
    float32 = np.float64

    def __getattr__(self, n):
        return getattr(np, n)


class _Torch64:
    @staticmethod
    def Tensor(a):
        return torch.as_tensor(np.asarray(a), dtype=torch.float64)

    def __getattr__(self, n):
        return getattr(torch, n)


def run64(fn, *a, **k):
    keep = ref_rr.np, ref_rr.torch
    ref_rr.np, ref_rr.torch = _Numpy64(), _Torch64()
    try:
        return np.asarray(fn(*[np.asarray(x, dtype=np.float64) for x in a], **k), dtype=np.float64)
    finally:
        ref_rr.np, ref_rr.torch = keep


def blocks(seed, Q, Gn, asym):
    """fp32 similarity blocks of Q + G unit embeddings planted around (Q + G) // 8 + 2 cluster centres"""
    g = G.rng(seed)
    n = Q + Gn
    centres = g.normal(0, 1, (n // 8 + 2, DIM))
    e = centres[g.integers(0, len(centres), n)] + 0.45 * g.normal(0, 1, (n, DIM))
    e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    q, v = e[:Q], e[Q:]
    qq, qg, gg = q @ q.T, q @ v.T, v @ v.T
    if asym:
        gg = gg + (0.03 * g.normal(0, 1, gg.shape)).astype(np.float32) * (1 - np.eye(len(v), dtype=np.float32))
    return [np.ascontiguousarray(a, dtype=np.float32) for a in (qg, qq, gg)]


def list_gap(x, k):
    """smallest difference among the k + 1 largest values of every row of x"""
    s = -np.sort(-np.asarray(x, dtype=np.float64), axis=1)[:, :k + 1]
    return float(-np.diff(s, axis=1).max())


def main():
    arrays = {}
    for name, (Q, Gn, k1, k2, asym) in CASES.items():
        topk = Gn // 2
        for seed in range(1000):
            qg, qq, gg = blocks(1000 * len(name) + seed, Q, Gn, asym)
            gap = R.neighbour_gap(qg, qq, gg, k1)
            gap_t = min(list_gap(gg, k1), list_gap(qg, topk))
            if gap < MIN_GAP or gap_t < MIN_GAP:
                continue
            out32 = np.asarray(ref_rr.re_ranking(qg, qq, gg, k1=k1, k2=k2), dtype=np.float32)
            out64 = run64(ref_rr.re_ranking, qg, qq, gg, k1=k1, k2=k2)
            tkb32 = np.asarray(ref_rr.re_ranking_tkb_simple(qg, qq, gg, topK=topk, k1=k1), dtype=np.float32)
            tkb64 = run64(ref_rr.re_ranking_tkb_simple, qg, qq, gg, topK=topk, k1=k1)
            e_ref, e_tkb = float(np.abs(out32 - out64).max()), float(np.abs(tkb32 - tkb64).max())
            if e_ref <= 1e-6 and e_tkb <= 1e-6:
                break
        else:
            raise SystemExit('%s: no seed without a near-tie' % name)
        assert out64.dtype == np.float64 and out32.shape == out64.shape == (Q, Gn)
        assert not asym or np.abs(gg - gg.T).max() > 1e-3
        print('%-12s seed %3d  gap %.2e  tkb gap %.2e  e_ref %.2e  e_tkb %.2e' % (name, seed, gap, gap_t, e_ref, e_tkb))
        arrays.update({name + '/q_g': qg, name + '/q_q': qq, name + '/g_g': gg, name + '/out32': out32, name + '/out64': out64,
                       name + '/e_ref': np.float64(e_ref), name + '/gap': np.float64(gap), name + '/tkb32': tkb32,
                       name + '/tkb64': tkb64, name + '/e_tkb': np.float64(e_tkb),
                       name + '/params': np.array([Q, Gn, k1, k2, topk], dtype=np.int64)})
    G.save('rerank', **arrays)


if __name__ == '__main__':
    main()
