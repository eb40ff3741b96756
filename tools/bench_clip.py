#!/usr/bin/env python3
"""Times the CLIP text encoder (clip_text.ClipTxtEncoder, laff_clip_encode) against the reference-shaped path on the device.

ViT-B/32 text (width 512, 8 heads, 12 layers, embed 512; random weights at CLIP's init scales).  For each case (N captions, seeded
MSR-VTT-like: 1 + Poisson(8) words, at most 40, from a small word list) three things are timed with device events around work
that ends in a synchronise:
  device     the encode call on a prepared ragged batch (ids / row_off already on the device, workspace allocated), per precision
  encoder    ClipTxtEncoder.forward from caption strings (tokenising on the host and the row-budget chunking included), fp16
  ref_path   the reference's encode_text shape on the device (tests/clip_ref.RefTextFp16: torch fp16, all 77 positions,
             nn.MultiheadAttention with the causal mask, fp32 LayerNorm casts) on prepared [N, 77] ids
FLOPs are those of the ragged rows: 24 W^2 per row and layer (in_proj, out_proj, c_fc, c_proj), 2 W L(L+1) per caption and layer
for the causal attention, 2 W E per caption for the projection; TF/s against 2.5 PF (fp16) and 157 TF (fp32).

    python tools/bench_clip.py [--cases 1,64,1000,40000] [--reps 5] [--out FILE.json]
    python tools/bench_clip.py --device-only --cases 40000     # only the fp16 device call (for a rocprofv3 --kernel-trace run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from laff_amd import clip_text as CT  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

W, LAYERS, HEADS, E = 512, 12, 8, 512
PEAK = {'fp16': 2.5e15, 'fp32': 157.3e12}
WORDS = ('a man woman person dog cat is are playing plays guitar piano on the stage in park kitchen street car red blue two '
         'people dancing singing cooking food video of news talking about game minecraft football basketball someone showing '
         'how to make cake water slow motion child baby laughing').split()


def captions(n, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(1 + g.poisson(8.0, n), 40)
    return [' '.join(g.choice(WORDS, L)) for L in lens]


def text_sd(seed=0):
    torch.manual_seed(seed)
    return {k: v.detach() for k, v in CT._ClipText(W, LAYERS, E, 77, 49408).state_dict().items()}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def flops(row_off):
    L = np.diff(row_off).astype(np.float64)
    return LAYERS * (24.0 * W * W * L.sum() + 2.0 * W * (L * (L + 1)).sum()) + 2.0 * W * E * len(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1,64,1000,40000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_clip.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    tok = CT.ClipTokenizer(os.path.join(ROOT, 'tests', 'golden', 'clip_bpe_subset.txt.gz'))
    sd = text_sd()
    encs = {p: CT.ClipTxtEncoder.from_state_dict(sd, tok, precision=p) for p in (('fp16',) if a.device_only else ('fp16', 'fp32'))}
    ref = None
    if not a.device_only:
        from clip_ref import RefTextFp16
        ref = RefTextFp16(sd)
    rows = []
    for n in [int(x) for x in a.cases.split(',')]:
        caps = captions(n, n)
        hb = encs['fp16'].batch(caps)
        b = encs['fp16'].to_device(hb)
        R = int(hb.row_off[-1])
        f = flops(hb.row_off)
        reps = max(1, a.reps if n < 10000 else a.reps // 2)
        r = {'N': n, 'rows': R, 'rows_dense': 77 * n, 'mean_len': R / n, 'gflop_ragged': f / 1e9}
        for p, enc in encs.items():
            ws = torch.empty(enc.workspace_bytes(b), dtype=torch.uint8, device='cuda')
            out = torch.empty((n, E), device='cuda')
            ms = timed(lambda: enc.encode_batch(b, out=out, workspace=ws), reps)
            r['device_%s_ms' % p] = ms
            r['device_%s_tflops' % p] = f / (ms * 1e-3) / 1e12
            r['device_%s_peak_frac' % p] = f / (ms * 1e-3) / PEAK[p]
            del ws
        if not a.device_only:
            r['encoder_ms'] = timed(lambda: encs['fp16']({'caption': caps}), reps)
            dense = torch.from_numpy(tok.tokenize(caps)).cuda()
            r['ref_path_ms'] = timed(lambda: ref(dense), 1 if n >= 10000 else reps)
            ours = encs['fp16'].encode_batch(b).double()
            theirs = ref(dense).double()
            r['max_rel_diff_fp16_vs_ref_path'] = float(((ours - theirs).norm(dim=1) / theirs.norm(dim=1)).max())
            r['speedup_device_vs_ref'] = r['ref_path_ms'] / r['device_fp16_ms']
            r['speedup_encoder_vs_ref'] = r['ref_path_ms'] / r['encoder_ms']
        print(json.dumps(r), flush=True)
        rows.append(r)
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'width': W, 'layers': LAYERS, 'heads': HEADS,
           'embed_dim': E, 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device']}))


if __name__ == '__main__':
    main()
