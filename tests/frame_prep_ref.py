"""An independent restatement of the reference's frame preprocessing (torchvision's Resize / CenterCrop / ToTensor / Normalize over
Pillow's 8-bit resample), in plain Python floats and numpy: the WHOLE image is resized, one output index at a time, then cropped.
tests/golden/frame_prep.npz pins it to Pillow itself; it then checks the full-size GPU cases where neither Pillow nor the reference is
present."""
import math

import numpy as np

CLIP = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {'clip': (bicubic, 2.0, CLIP), 'slip': (bilinear, 1.0, IMAGENET)}


def coefficients(size_in, size_out, filt, support):
    """Per output index: (xmin, [integer taps])."""
    scale = size_in / size_out
    fs = scale if scale > 1.0 else 1.0
    sup = support * fs
    inv = 1.0 / fs
    out = []
    for xx in range(size_out):
        c = (xx + 0.5) * scale
        xmin = max(0, int(c - sup + 0.5))
        xmax = min(size_in, int(c + sup + 0.5))
        w = [filt((i + xmin - c + 0.5) * inv) for i in range(xmax - xmin)]
        tot = 0.0
        for v in w:
            tot += v
        if tot != 0.0:
            w = [v / tot for v in w]
        out.append((xmin, [int(v * 4194304.0 - 0.5) if v < 0 else int(v * 4194304.0 + 0.5) for v in w]))
    return out


def resample_axis1(img, size_out, filt, support):
    """img [A, in, 3] uint8 -> [A, size_out, 3] uint8 along axis 1."""
    res = np.empty((img.shape[0], size_out, 3), np.uint8)
    for xx, (xmin, taps) in enumerate(coefficients(img.shape[1], size_out, filt, support)):
        k = np.asarray(taps, np.int64)
        acc = (img[:, xmin:xmin + len(taps), :].astype(np.int64) * k[None, :, None]).sum(axis=1) + (1 << 21)
        res[:, xx, :] = np.clip(acc >> 22, 0, 255)
    return res


def output_size(h, w, R):
    if (w <= h and w == R) or (h <= w and h == R):
        return h, w
    return (int(R * h / w), R) if w <= h else (R, int(R * w / h))


def resize_crop(img, R, kind):
    """[H, W, 3] uint8 -> the resized, center-cropped [R, R, 3] uint8 image; also (oh, ow, top, left)."""
    filt, support, _ = FILTERS[kind]
    h, w = img.shape[:2]
    oh, ow = output_size(h, w, R)
    x = img
    if ow != w:
        x = resample_axis1(x, ow, filt, support)                                    # horizontal first, rounded to uint8
    if oh != h:
        x = resample_axis1(x.transpose(1, 0, 2), oh, filt, support).transpose(1, 0, 2)
    top, left = int(round((oh - R) / 2.0)), int(round((ow - R) / 2.0))
    return np.ascontiguousarray(x[top:top + R, left:left + R]), (oh, ow, top, left)


def normalise(u8, kind):
    """[R, R, 3] uint8 -> [3, R, R] fp32: (u / 255 - mean) / std, every step in fp32."""
    mean, std = FILTERS[kind][2]
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return (x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]


def preprocess(img, R, kind):
    u8, _ = resize_crop(img, R, kind)
    return normalise(u8, kind), u8
