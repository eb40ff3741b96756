#!/usr/bin/env python3
"""Element pairs per second of ops.sim_hist (the 'hist' / Jaccard measure) at retrieval sizes, against the reference's own formulation
run with torch on the same device (row-chunked torch.minimum / torch.maximum + sum).

    python tools/bench_hist.py [--nt 10000] [--nv 3000] [--reps 7] [--warmup 2] [--chunk 16]

Two shapes: K = 3981 with H = 1 (a bag-of-words sized concept space) and K = 4096 with H = 8.  Times are device events around one
call, the median of --reps after --warmup.  The share of the fp32 VALU issue rate counts VALU_PER_PAIR issue slots per element pair
(v_min_f32, v_max_f32 and two adds; the compiler pairs the adds into v_pk_add_f32, which occupies two slots) against 256 CUs x 4 SIMDs x
32 lanes per clock at the 2.4 GHz peak clock.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from laff_amd import ops  # noqa: E402

VALU_PER_PAIR = 4.0
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2] * 1e-3


def torch_hist(T, V, H, eps, chunk):
    """the reference's formulation (loss.py:43-50 per head, model/model.py:1008-1014 over heads), `chunk` text rows at a time"""
    t, v = T.view(T.shape[0], H, -1), V.view(V.shape[0], H, -1)
    out = torch.empty((T.shape[0], V.shape[0]), device=T.device)
    for r in range(0, T.shape[0], chunk):
        x = t[r:r + chunk, None]
        out[r:r + chunk] = (torch.minimum(x, v[None]).sum(-1) / (torch.maximum(x, v[None]).sum(-1) + eps)).mean(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, default=10000)
    ap.add_argument('--nv', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=16)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    for K, H in ((3981, 1), (4096, 8)):
        T = torch.sigmoid(1.5 * torch.randn(a.nt, K, generator=g, device=dev))
        V = torch.sigmoid(1.5 * torch.randn(a.nv, K, generator=g, device=dev))
        out = ops.alloc_scores(a.nt, a.nv, dev)
        dt = timed(lambda: ops.sim_hist(T, V, heads=H, eps=1e-8, out=out), a.warmup, a.reps)
        rows = min(a.nt, 512)                                    # the baseline on a slice of the text rows, scaled
        dt_ref = timed(lambda: torch_hist(T[:rows], V, H, 1e-8, a.chunk), 1, 3) * a.nt / rows
        diff = float((torch_hist(T[:rows], V, H, 1e-8, a.chunk) - out[:rows]).abs().max())
        pairs = float(a.nt) * a.nv * K
        print(json.dumps({'bench': 'sim_hist', 'Nt': a.nt, 'Nv': a.nv, 'K': K, 'H': H, 'seconds_median': dt,
                          'pairs_per_s': pairs / dt, 'valu_issue_share': pairs * VALU_PER_PAIR / dt / LANE_OPS_PER_S,
                          'torch_seconds_scaled': dt_ref, 'torch_rows_timed': rows, 'speedup_vs_torch': dt_ref / dt,
                          'max_abs_diff_vs_torch': diff}), flush=True)


if __name__ == '__main__':
    main()
