"""Writes tests/golden/frame_prep.npz: small seeded synthetic frames and what Pillow makes of them under torchvision's rules
(Resize(R) short side, bicubic for 'clip' / bilinear for 'slip'; CenterCrop(R) with Python's half-to-even round), plus the fp32
ToTensor / Normalize result of two of them computed with torch on the CPU.  Needs Pillow; run on a development machine:

    python tools/gen_golden_frame_prep.py

The fixture holds frames and recorded outputs only.  It stays well under 1 MB, so the main resolution is 80 rather than 224 (the
full-size GPU tests cover 224 against tests/frame_prep_ref.py, which this fixture pins to Pillow)."""
import json
import os

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER = {'clip': Image.BICUBIC, 'slip': Image.BILINEAR}
NORM = {'clip': ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
        'slip': ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))}
# name: (width, height, R)
FRAMES = {
    'landscape': (144, 108, 80),
    'portrait': (108, 144, 80),
    'square_at_R': (80, 80, 80),
    'enlarged': (64, 48, 80),            # short side below R
    'big_downscale': (256, 144, 32),     # scale 4.5: 18 / 9 taps per output
    'half_73': (173, 90, 80),            # resized to 153 x 80: (153 - 80) / 2 = 36.5 -> 36
    'half_75': (175, 90, 80),            # resized to 155 x 80: (155 - 80) / 2 = 37.5 -> 38
    'odd': (101, 83, 80),
    'short_side_at_R': (110, 80, 80),    # passes through the resize, cropped only
    'small_R_landscape': (100, 75, 64),
    'small_R_portrait': (75, 120, 64),
    'tall_strip': (40, 200, 64),
}
FP32 = {'enlarged': 'clip', 'small_R_portrait': 'slip'}


def synth(w, h, rng):
    """A smooth pattern plus noise, with saturated patches so that the clip to [0, 255] is exercised."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 120 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], axis=-1)
    img += rng.normal(0, 25, img.shape)
    img[(x.astype(int) // 8 + y.astype(int) // 8) % 5 == 0] *= 4.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def resize_size(w, h, R):
    if (w <= h and w == R) or (h <= w and h == R):
        return w, h
    return (R, int(R * h / w)) if w <= h else (int(R * w / h), R)


def main():
    rng = np.random.default_rng(20240607)
    out, meta = {}, {}
    for name, (w, h, R) in FRAMES.items():
        img = synth(w, h, rng)
        out[name + '/frame'] = img
        ow, oh = resize_size(w, h, R)
        top, left = int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))
        meta[name] = {'R': R, 'out_height': oh, 'out_width': ow, 'top': top, 'left': left}
        for kind, flt in FILTER.items():
            pil = Image.fromarray(img, 'RGB')
            if (ow, oh) != (w, h):
                pil = pil.resize((ow, oh), flt)
            u8 = np.asarray(pil.crop((left, top, left + R, top + R)))
            assert u8.shape == (R, R, 3)
            out['%s/%s/u8' % (name, kind)] = u8
            if FP32.get(name) == kind:
                mean, std = (torch.tensor(v, dtype=torch.float32)[:, None, None] for v in NORM[kind])
                t = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)       # ToTensor
                out['%s/%s/pixels' % (name, kind)] = t.sub(mean).div(std).numpy()                               # Normalize
    out['meta'] = np.array(json.dumps(meta))
    path = os.path.join(ROOT, 'tests', 'golden', 'frame_prep.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
