#!/usr/bin/env python3
"""Times the CLIP image encoder (clip_image.ClipImageEncoder, laff_clip_image_encode) against the reference-shaped path on the device.

ViT-B/32 and ViT-B/16 (width 768, 12 heads, 12 layers, embed 512; random weights at CLIP's init scales), F frames of 224 x 224
(N(0, 1) pixels, already on the device).  Per case, with device events around work that ends in a synchronise:
  device     the encode call (pixels, frame_off and workspace prepared: 8 frames per video), per precision
  encoder    ClipImageEncoder.encode_frames (the frame-budget chunking and per-call workspace included), fp16
  ref_path   the reference's encode_image shape (tests/clip_image_ref.RefImageFp16: torch fp16, F.conv2d, nn.MultiheadAttention over
             all rows, fp32 LayerNorm casts)
FLOPs are the reference's (every row of every block): per frame 2 g^2 W 3p^2 + layers (24 L W^2 + 4 L^2 W) + 2 W E.  The device call
does less (the last block's class rows only), so its TF/s are effective ones.  TF/s against 2.5 PF (fp16) and 157 TF (fp32).

    python tools/bench_clip_image.py [--archs B/32,B/16] [--cases 8,64,1024,8192] [--reps 5] [--out FILE.json]
    python tools/bench_clip_image.py --device-only --archs B/16 --cases 1024     # only the fp16 device call (for rocprofv3)
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

from laff_amd import clip_image as CI  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

ARCH = {'B/32': (768, 12, 12, 32, 224, 512), 'B/16': (768, 12, 12, 16, 224, 512)}
PEAK = {'fp16': 2.5e15, 'fp32': 157.3e12}


def visual_sd(arch, seed=0):
    torch.manual_seed(seed)
    w, layers, heads, patch, res, embed = ARCH[arch]
    return {'visual.' + k: v.detach() for k, v in CI._ClipVisual(w, layers, patch, res, embed).state_dict().items()}


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


def flops(arch, F):
    W, layers, _, p, res, E = ARCH[arch]
    g = res // p
    L = g * g + 1
    return F * (2.0 * g * g * W * 3 * p * p + layers * (24.0 * L * W * W + 4.0 * L * L * W) + 2.0 * W * E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--archs', default='B/32,B/16')
    ap.add_argument('--cases', default='8,64,1024,8192')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_clip_image.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    rows = []
    for arch in a.archs.split(','):
        sd = visual_sd(arch)
        precs = ('fp16',) if a.device_only else ('fp16', 'fp32')
        encs = {p: CI.ClipImageEncoder.from_state_dict(sd, precision=p, max_frames=1024) for p in precs}
        ref = None
        if not a.device_only:
            from clip_image_ref import RefImageFp16
            ref = RefImageFp16(sd)
        for F in [int(x) for x in a.cases.split(',')]:
            pix = torch.randn(F, 3, 224, 224, device='cuda', generator=torch.Generator('cuda').manual_seed(F))
            V = (F + 7) // 8
            foh = np.minimum(np.arange(V + 1) * 8, F).astype(np.int32)
            fo = torch.from_numpy(foh).cuda()
            f = flops(arch, F)
            reps = max(1, a.reps if F < 4096 else a.reps // 2)
            r = {'arch': arch, 'F': F, 'gflop': f / 1e9}
            for p, enc in encs.items():
                ws = torch.empty(enc.workspace_bytes(F), dtype=torch.uint8, device='cuda')
                out = torch.empty((F, 512), device='cuda')
                mean = torch.empty((V, 512), device='cuda')
                ms = timed(lambda: enc.encode_batch(pix, fo, foh, out=out, out_mean=mean, workspace=ws), reps)
                r['device_%s_ms' % p] = ms
                r['device_%s_tflops' % p] = f / (ms * 1e-3) / 1e12
                r['device_%s_peak_frac' % p] = f / (ms * 1e-3) / PEAK[p]
                del ws
            if not a.device_only:
                r['encoder_ms'] = timed(lambda: encs['fp16'].encode_frames(pix), reps)
                r['ref_path_ms'] = timed(lambda: [ref(pix[s:s + 1024]) for s in range(0, F, 1024)], reps)
                r['ref_path_tflops'] = f / (r['ref_path_ms'] * 1e-3) / 1e12
                r['speedup_device_vs_ref'] = r['ref_path_ms'] / r['device_fp16_ms']
                r['speedup_encoder_vs_ref'] = r['ref_path_ms'] / r['encoder_ms']
            print(json.dumps(r), flush=True)
            rows.append(r)
            del pix
            torch.cuda.empty_cache()
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device']}))


if __name__ == '__main__':
    main()
