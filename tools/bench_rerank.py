#!/usr/bin/env python3
"""Queries per second of k-reciprocal re-ranking on the device at the reference's defaults (topK = 3000, k1 = 20, k2 = 6: one problem
of 3,001 items per query), against the reference's Python loop.

    python tools/bench_rerank.py [--queries 32] [--topk 3000] [--k1 20] [--k2 6] [--reps 3] [--reference]

--reference times the reference's own `re_ranking` on one of the problems on this host's CPU (build container only: it is imported
through tools/gen_golden.py); without it the speed-up line uses --reference-seconds (2.5 s per query, measured on the build host).
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from laff_amd import ops  # noqa: E402
from laff_amd.model import ReRank  # noqa: E402


def problem(g, dev, K, dim=64):
    """one query against K candidates: unit embeddings planted around K // 20 centres"""
    centres = torch.randn(max(2, K // 20), dim, generator=g, device=dev)
    e = centres[torch.randint(0, centres.shape[0], (K + 1,), generator=g, device=dev)] + 0.6 * torch.randn(K + 1, dim, generator=g, device=dev)
    e = torch.nn.functional.normalize(e, dim=1)
    return (e[:1] @ e[1:].T).contiguous(), torch.ones(1, 1, device=dev), (e[1:] @ e[1:].T).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--queries', type=int, default=32)
    ap.add_argument('--topk', type=int, default=3000)
    ap.add_argument('--k1', type=int, default=20)
    ap.add_argument('--k2', type=int, default=6)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--reference', action='store_true')
    ap.add_argument('--reference-seconds', type=float, default=2.5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    probs = [problem(g, dev, a.topk) for _ in range(a.queries)]
    need = ops.rerank_workspace_bytes([(1, a.topk)], a.k1, a.k2)
    ReRank.re_ranking_batched(probs[:2], k1=a.k1, k2=a.k2)                 # warm-up: module load, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        outs = ReRank.re_ranking_batched(probs, k1=a.k1, k2=a.k2)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[len(times) // 2]
    ref_s, ref_src = a.reference_seconds, 'given'
    if a.reference:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import gen_golden  # noqa: F401
        from model import ReRank as ref_rr
        qg, qq, gg = (t.cpu().numpy() for t in probs[0])
        t0 = time.perf_counter()
        want = ref_rr.re_ranking(qg, qq, gg, k1=a.k1, k2=a.k2)
        ref_s, ref_src = time.perf_counter() - t0, 'measured'
        print('max |device - reference| on that problem: %.2e' % float(abs(outs[0].cpu().numpy() - want).max()), file=sys.stderr)
    print(json.dumps({'bench': 'rerank', 'queries': a.queries, 'items': a.topk + 1, 'k1': a.k1, 'k2': a.k2,
                      'seconds_median': dt, 'queries_per_s': a.queries / dt, 'ms_per_query': 1e3 * dt / a.queries,
                      'workspace_bytes_per_query': need, 'reference_s_per_query': ref_s, 'reference_source': ref_src,
                      'speedup_vs_reference': ref_s / (dt / a.queries)}))


if __name__ == '__main__':
    main()
