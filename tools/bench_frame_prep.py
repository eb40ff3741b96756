#!/usr/bin/env python3
"""Times frame preprocessing on the device (frame_prep.FramePreprocessor, laff_frame_preprocess) beside the host path it replaces and
the CLIP image encode that follows it.

F decoded frames of one size (random uint8, generated on the device), R = 224, kind 'clip' (bicubic).  Per case:
  device     the laff_frame_preprocess call (frames, descriptors and tap tables on the device), device events over --reps calls;
             frames/s, and the achieved bytes/s over the ALGORITHMIC bytes: the source window the R x R output depends on, read once,
             plus the fp32 output written once
  host       the path it replaces, on this machine's CPU: Pillow's resize + crop and torch's ToTensor / Normalize where PIL imports,
             else the library's numpy path, over --host-frames frames on --threads threads, scaled to F; plus the H2D copy of the
             preprocessed fp32 pixels from pinned memory (measured on up to 1,024 frames, scaled to F)
  encode     ClipImageEncoder.encode_frames (ViT-B/32, fp16, random weights) of the same F frames' pixels in the same run
The device preprocessing must take less time than the encode (it may never be the slower stage): the tool exits 1 otherwise.

    python tools/bench_frame_prep.py [--cases 1024x640x360,8192x640x360,1024x1920x1080] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from laff_amd import _lib, ops  # noqa: E402
from laff_amd import clip_image as CI  # noqa: E402
from laff_amd import frame_prep as FP  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

B32 = (768, 12, 12, 32, 224, 512)
R = 224


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


def algorithmic_bytes(pre, F, H, W):
    oh, ow, _, _ = pre.plan(H, W)
    hx, hn, _ = pre.taps(W, ow)
    vx, vn, _ = pre.taps(H, oh)
    window = (int((vx + vn).max()) - int(vx.min())) * (int((hx + hn).max()) - int(hx.min())) * 3
    return F * (window + 3 * R * R * 4)


def host_path(pre, H, W, n, threads):
    """(ms per frame on one thread, ms per frame with `threads` threads, what ran) over n random frames."""
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    oh, ow, top, left = pre.plan(H, W)
    mean, std = (torch.from_numpy(v)[:, None, None] for v in (pre.mean, pre.std))
    try:
        from PIL import Image

        def one(img):
            pil = Image.fromarray(img, 'RGB')
            if (ow, oh) != (W, H):
                pil = pil.resize((ow, oh), Image.BICUBIC)
            u8 = np.asarray(pil.crop((left, top, left + R, top + R)))
            return torch.from_numpy(u8.copy()).permute(2, 0, 1).to(torch.float32).div(255).sub(mean).div(std)
        what = 'Pillow %s' % __import__('PIL').__version__
    except ImportError:
        cpu = FP.FramePreprocessor(R, kind=pre.kind, device='cpu')

        def one(img):
            return cpu([img])
        what = 'numpy path of laff_amd.frame_prep'
    one(frames[0])
    t0 = time.perf_counter()
    for f in frames[:max(1, n // 4)]:
        one(f)
    single = (time.perf_counter() - t0) / max(1, n // 4)
    torch.set_num_threads(1)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, frames[:threads]))
        t0 = time.perf_counter()
        list(ex.map(one, frames))
        multi = (time.perf_counter() - t0) / n
    return single * 1e3, multi * 1e3, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1024x640x360,8192x640x360,1024x1920x1080')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-frames', type=int, default=128)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_frame_prep.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    enc = CI.ClipImageEncoder(*B32, precision='fp16', device='cuda', max_frames=1024)
    pre = enc.preprocessor('clip')
    rows, ok = [], True
    for case in a.cases.split(','):
        F, W, H = (int(v) for v in case.split('x'))
        stride = (H * W * 3 + 15) & ~15
        buf = torch.randint(0, 256, (F * stride,), dtype=torch.uint8, device='cuda', generator=torch.Generator('cuda').manual_seed(F))
        oh, ow, _, _ = pre.plan(H, W)
        desc = (_lib.FrameDesc * F)()
        ht, vt = pre._table_index(W, ow), pre._table_index(H, oh)
        for i in range(F):
            desc[i].offset, desc[i].height, desc[i].width, desc[i].htab, desc[i].vtab = i * stride, H, W, ht, vt
        desc_dev = ops.frame_desc_device(desc, F, buf.device)
        taps, taps_host = pre._taps_buffers()
        pix = torch.empty((F, 3, R, R), device='cuda')
        ms = timed(lambda: ops.frame_preprocess(buf, desc, F, R, taps, taps_host, pre.mean, pre.std, out=pix, desc_dev=desc_dev), a.reps)
        nbytes = algorithmic_bytes(pre, F, H, W)
        r = {'F': F, 'width': W, 'height': H, 'R': R, 'device_ms': ms, 'device_frames_per_s': F / (ms * 1e-3),
             'algorithmic_gb': nbytes / 1e9, 'device_gb_per_s': nbytes / (ms * 1e-3) / 1e9}
        single, multi, what = host_path(pre, H, W, a.host_frames if H * W < 1e6 else max(a.threads, a.host_frames // 4), a.threads)
        n_copy = min(F, 1024)
        pinned = torch.empty((n_copy, 3, R, R)).pin_memory()
        h2d = timed(lambda: pix[:n_copy].copy_(pinned, non_blocking=True), 5) * F / n_copy
        r.update({'host_what': what, 'host_ms_per_frame_1_thread': single, 'host_threads': a.threads,
                  'host_ms_per_frame_threads': multi, 'host_ms': multi * F, 'h2d_fp32_ms': h2d, 'host_plus_h2d_ms': multi * F + h2d})
        r['encode_b32_fp16_ms'] = timed(lambda: enc.encode_frames(pix), max(2, a.reps // 4))
        r['device_over_encode'] = ms / r['encode_b32_fp16_ms']
        r['speedup_vs_host_plus_h2d'] = r['host_plus_h2d_ms'] / ms
        r['prep_faster_than_encode'] = bool(ms < r['encode_b32_fp16_ms'])
        ok = ok and r['prep_faster_than_encode']
        print(json.dumps(r), flush=True)
        rows.append(r)
        del buf, pix, pinned
        torch.cuda.empty_cache()
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device'], 'prep_faster_than_encode': ok}))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
