#!/usr/bin/env python3
"""Times the W2VV++-sized concat towers three ways on one device in one process, interleaved round by round:

  (a) concat   ops.fc_concat_act_bn_grouped: both towers in ONE segmented-K launch, nothing concatenated, the bow feature stays CSR
  (b) cat      what the parent library offers: torch.cat of the dense features with the bow densified, then ops.fc_act_bn per tower
  (c) gather   torch.cat of the dense features only -> ops.fc_act_bn without an epilogue, + ops.fc_gather_act_bn of the CSR bow
               through the transposed column block, then bias / tanh / BatchNorm as torch element-wise kernels

Text: Nt captions, rnn 1024 + CSR bow over 10,000 columns (~10 entries a row) + w2v 500; video: Nv x (2048 + 2048); D = 2048.
Each round times every variant once with device events; the medians and minima over the rounds are reported, with the bytes each
variant allocates (torch.cuda.max_memory_allocated over one call) and, as a yardstick for the dense part, ops.fc_act_bn on ONE dense
segment of the same total K against fc_concat on that same single segment.

    python tools/bench_w2vvpp.py [--nt 40000] [--nv 10000] [--rounds 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from laff_amd import ops  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

D, V, RNN, W2V, VIS = 2048, 10000, 1024, 500, (2048, 2048)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nt', type=int, default=40000)
    ap.add_argument('--nv', type=int, default=10000)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_w2vvpp.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    Nt, Nv = a.nt, a.nv
    g = np.random.default_rng(0)
    torch.manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device='cuda')
    Kt, Kv = RNN + V + W2V, sum(VIS)
    Wt_, Wv = rnd(D, Kt) / np.sqrt(RNN + W2V + 10), rnd(D, Kv) / np.sqrt(Kv)
    vec = lambda: (rnd(D) * 0.1, torch.rand(D, device='cuda') + 0.5, rnd(D) * 0.1)
    (bt, st, ht), (bv, sv, hv) = vec(), vec()
    rnn, w2v = rnd(Nt, RNN), rnd(Nt, W2V)
    vis = [rnd(Nv, w) for w in VIS]
    nnz = g.integers(5, 16, Nt)
    indptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int32)
    cols = g.integers(0, V, int(indptr[-1])).astype(np.int32)
    bow = torch.sparse_csr_tensor(torch.from_numpy(indptr).cuda(), torch.from_numpy(cols).cuda(), torch.ones(len(cols), device='cuda'), size=(Nt, V))
    wt_bow = Wt_[:, RNN:RNN + V].t().contiguous()
    W_dense = torch.cat([Wt_[:, :RNN], Wt_[:, RNN + V:]], dim=1).contiguous()       # (c): the weight columns of the dense text features

    def concat():
        return ops.fc_concat_act_bn_grouped([
            dict(segments=vis, weight=Wv, bias=bv, bn_scale=sv, bn_shift=hv, activation='tanh'),
            dict(segments=[rnn, bow, w2v], weight=Wt_, weight_t={1: wt_bow}, bias=bt, bn_scale=st, bn_shift=ht, activation='tanh')])

    def cat():
        xt = torch.cat([rnn, bow.to_dense(), w2v], dim=1)
        xv = torch.cat(vis, dim=1)
        return ops.fc_act_bn_grouped([dict(x=xv, weight=Wv, bias=bv, bn_scale=sv, bn_shift=hv, activation='tanh'),
                                      dict(x=xt, weight=Wt_, bias=bt, bn_scale=st, bn_shift=ht, activation='tanh')])

    def gather():
        xt = torch.cat([rnn, w2v], dim=1)
        xv = torch.cat(vis, dim=1)
        yv, yt = ops.fc_act_bn_grouped([dict(x=xv, weight=Wv, bias=bv, bn_scale=sv, bn_shift=hv, activation='tanh'), dict(x=xt, weight=W_dense)])
        yt += ops.fc_gather_act_bn(bow, wt_bow)
        return yv, torch.tanh(yt.add_(bt)).mul_(st).add_(ht)

    variants = {'concat': concat, 'cat': cat, 'gather': gather}
    ref = concat()
    diffs = {k: [float((x - y).abs().max()) for x, y in zip(ref, f())] for k, f in variants.items() if k != 'concat'}
    x1 = rnd(Nt, RNN + W2V)
    W1 = rnd(D, RNN + W2V) / np.sqrt(RNN + W2V)
    single = {'fc_act_bn_1seg': lambda: ops.fc_act_bn(x1, W1, bt, st, ht, 'tanh'),
              'fc_concat_1seg': lambda: ops.fc_concat_act_bn([x1], W1, bt, st, ht, 'tanh')}
    everything = dict(variants, **single)
    for _ in range(a.warmup):
        for f in everything.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in everything}
    for _ in range(a.rounds):
        for k, f in everything.items():
            times[k].append(event_ms(f))
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'Nt': Nt, 'Nv': Nv, 'D': D, 'rounds': a.rounds,
           'text_K': Kt, 'text_nnz_per_row': float(nnz.mean()), 'concat_matrix_bytes': 4 * (Nt * Kt + Nv * Kv),
           'max_abs_diff_vs_concat': diffs}
    for k in everything:
        res[k + '_ms_median'] = float(np.median(times[k]))
        res[k + '_ms_min'] = float(np.min(times[k]))
    for k, f in variants.items():
        res[k + '_peak_bytes'] = peak_bytes(f)
    flop1 = 2.0 * Nt * (RNN + W2V) * D
    res['fc_act_bn_1seg_tflops'] = flop1 / (res['fc_act_bn_1seg_ms_median'] * 1e-3) / 1e12
    res['fc_concat_1seg_tflops'] = flop1 / (res['fc_concat_1seg_ms_median'] * 1e-3) / 1e12
    res['concat_not_slower'] = res['concat_ms_median'] <= min(res['cat_ms_median'], res['gather_ms_median'])
    res['concat_saves_the_matrix'] = res['cat_peak_bytes'] - res['concat_peak_bytes'] >= res['concat_matrix_bytes']
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
