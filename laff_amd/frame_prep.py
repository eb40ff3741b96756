"""Frame preprocessing on the device: decoded RGB uint8 frames of any size -> the CLIP image encoder's [F, 3, R, R] fp32 pixels, a
drop-in for the reference's per-frame torchvision-on-Pillow transform (model/clip/clip.py:58-65: Resize(n_px, BICUBIC), CenterCrop,
ToTensor, Normalize; data_provider.py:274-281 the bilinear 'slip' variant with the ImageNet constants).

The resized, cropped uint8 image equals Pillow's bit for bit: the host derives Pillow's integer taps in float64 once per distinct
(in, out, filter) -- for the R outputs of the cropped window only -- and the device (`laff_frame_preprocess`,
laff_amd/csrc/frame_prep.hip) does integer multiply-adds only, horizontal pass -> uint8 -> vertical pass.  ToTensor and Normalize are
(float(u) / 255 - mean) / std in fp32 with true divides.

Not here: JPEG / video decoding and `convert('RGB')` (the caller hands over decoded RGB frames), the random training crops
(RandomResizedCrop, data_provider.py:224-238), the reference's all-ones placeholder for a missing video, ModifiedResNet towers.
"""
import numpy as np
import torch

#: kind -> (filter, support, mean, std)
KINDS = {
    'clip': ('bicubic', 2.0, (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
    'slip': ('bilinear', 1.0, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
}
MAX_SIDE, MAX_RESOLUTION = 4096, 512
PRECISION_BITS = 22


def sample_frame_indices(n_frames, sample_frame):
    """The reference's 'uniform' frame sampling, which is also what it does when a video has at most sample_frame frames
    (data_provider.py:324-326)."""
    return np.linspace(0, int(n_frames) - 1, int(sample_frame), dtype=int)


def resized_size(height, width, R):
    """torchvision's Resize(R) on a (width, height) image: the short side to R; (out_height, out_width)."""
    if (width <= height and width == R) or (height <= width and height == R):
        return height, width
    if width <= height:
        return int(R * height / width), R
    return R, int(R * width / height)


def crop_offsets(out_height, out_width, R):
    """torchvision's CenterCrop(R): (top, left), halves to even (Python's round)."""
    return int(round((out_height - R) / 2.0)), int(round((out_width - R) / 2.0))


def _filter(name, x):
    x = np.abs(x)
    if name == 'bilinear':
        return np.where(x < 1.0, 1.0 - x, 0.0)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def axis_taps(size_in, size_out, filt, support, first, count):
    """Pillow's 8-bit resample coefficients of one axis (precompute_coeffs + normalize_coeffs_8bpc), in float64, for the outputs
    first .. first + count - 1: (xmin [count], n [count], taps [count, K] int32, zero past n).  size_in == size_out: the axis is not
    resampled (Pillow skips the pass): the identity."""
    if size_in == size_out:
        return (np.arange(first, first + count, dtype=np.int32), np.ones(count, np.int32),
                np.full((count, 1), 1 << PRECISION_BITS, np.int32))
    scale = float(size_in) / float(size_out)
    fs = max(scale, 1.0)
    sup = support * fs
    ss = 1.0 / fs
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - sup + 0.5).astype(np.int64), 0)          # astype truncates toward zero, like C's (int)
    xmax = np.minimum((center + sup + 0.5).astype(np.int64), size_in)
    n = xmax - xmin
    K = int(n.max())
    i = np.arange(K, dtype=np.float64)
    w = _filter(filt, (i[None, :] + xmin[:, None] - center[:, None] + 0.5) * ss)
    w[np.arange(K)[None, :] >= n[:, None]] = 0.0
    ww = np.zeros(count, np.float64)
    for j in range(K):                                                   # Pillow's sum runs in tap order
        ww = ww + w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)
    k[np.arange(K)[None, :] >= n[:, None]] = 0
    return xmin.astype(np.int32), n.astype(np.int32), k.astype(np.int32)


def _resample_rows(img, xmin, n, k):
    """One pass along axis 1 of img [rows, in, 3] uint8 with integer taps -> [rows, count, 3] uint8."""
    acc = np.full((img.shape[0], xmin.shape[0], 3), 1 << (PRECISION_BITS - 1), np.int32)
    last = img.shape[1] - 1
    for i in range(k.shape[1]):
        acc += k[:, i][None, :, None] * img[:, np.minimum(xmin + i, last), :].astype(np.int32)     # (taps past n are zero)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


class FramePreprocessor(object):
    """Resize(R) -> CenterCrop(R) -> ToTensor -> Normalize of decoded frames.  kind 'clip': bicubic, CLIP's mean / std; 'slip':
    bilinear, the ImageNet constants.  Called on a list of [H, W, 3] uint8 numpy arrays or torch tensors (host or device) or on one
    [F, H, W, 3] uint8 tensor: [F, 3, R, R] fp32 on `device` (with return_uint8=True also the resized, cropped [F, R, R, 3] uint8
    image).  device 'cpu': the same integer arithmetic in numpy.  A frame's output does not depend on its batch (bitwise)."""

    def __init__(self, resolution, kind='clip', device='cuda'):
        if kind not in KINDS:
            raise ValueError("FramePreprocessor: kind must be 'clip' or 'slip', got %r" % (kind,))
        R = int(resolution)
        if not 1 <= R <= MAX_RESOLUTION:
            raise NotImplementedError('FramePreprocessor: resolution=%d; 1 .. %d are supported' % (R, MAX_RESOLUTION))
        self.resolution, self.kind, self.device = R, kind, torch.device(device)
        self.filter, self.support, mean, std = KINDS[kind]
        self.mean, self.std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        self._tables = {}             # (in, out) -> (xmin, n, taps) of the cropped window
        self._words = []              # the device tap buffer's host copy, table by table
        self._index = {}              # (in, out) -> word index of the table in the buffer
        self._n_words = 0
        self._dev_taps = None         # (device tensor, host array) of the words so far

    # ---- the rules
    def plan(self, height, width):
        """(out_height, out_width, top, left) of a height x width frame."""
        oh, ow = resized_size(height, width, self.resolution)
        top, left = crop_offsets(oh, ow, self.resolution)
        return oh, ow, top, left

    def taps(self, size_in, size_out):
        """The cropped window's tap table of an axis resized size_in -> size_out, cached."""
        key = (int(size_in), int(size_out))
        if key not in self._tables:
            first = int(round((key[1] - self.resolution) / 2.0))
            self._tables[key] = axis_taps(key[0], key[1], self.filter, self.support, first, self.resolution)
        return self._tables[key]

    # ---- input handling
    @staticmethod
    def _check(shape, dtype, what):
        if dtype not in (np.uint8, torch.uint8) or len(shape) != 3 or shape[2] != 3:
            raise ValueError('FramePreprocessor: %s must be [H, W, 3] uint8 RGB (decode and convert to RGB first), got %s %s'
                             % (what, tuple(shape), dtype))
        if not (1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE):
            raise NotImplementedError('FramePreprocessor: %s is %d x %d; each side 1 .. %d is supported' % (what, shape[0], shape[1], MAX_SIDE))

    def _frame_list(self, frames):
        if isinstance(frames, (np.ndarray, torch.Tensor)):
            if frames.ndim == 3:
                frames = [frames]
            elif frames.ndim == 4:
                frames = list(frames)
            else:
                raise ValueError('FramePreprocessor: expected [F, H, W, 3] or a list of [H, W, 3], got %s' % (tuple(frames.shape),))
        frames = list(frames)
        for i, f in enumerate(frames):
            if not isinstance(f, (np.ndarray, torch.Tensor)):
                raise ValueError('FramePreprocessor: frame %d is a %s; numpy arrays or torch tensors' % (i, type(f).__name__))
            self._check(f.shape, f.dtype, 'frame %d' % i)
        return frames

    def __call__(self, frames, return_uint8=False):
        frames = self._frame_list(frames)
        if self.device.type == 'cpu':
            u8 = self._cpu(frames)
            pix = (u8.permute(0, 3, 1, 2).to(torch.float32).div(255.0).sub(torch.from_numpy(self.mean)[None, :, None, None])
                   .div(torch.from_numpy(self.std)[None, :, None, None])).contiguous()
        else:
            pix, u8 = self._gpu(frames, return_uint8)
        return (pix, u8) if return_uint8 else pix

    # ---- host path: the same integer arithmetic in numpy
    def _cpu(self, frames):
        R = self.resolution
        out = np.empty((len(frames), R, R, 3), np.uint8)
        for i, f in enumerate(frames):
            img = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
            H, W = img.shape[:2]
            oh, ow, _, _ = self.plan(H, W)
            hx, hn, hk = self.taps(W, ow)
            vx, vn, vk = self.taps(H, oh)
            s0, s1 = int(vx.min()), int((vx + vn).max())                                  # only the rows the window depends on
            rows = _resample_rows(img[s0:s1], hx, hn, hk)                                  # [s1 - s0, R, 3]
            out[i] = _resample_rows(rows.transpose(1, 0, 2), vx - s0, vn, vk).transpose(1, 0, 2)
        return torch.from_numpy(out)

    # ---- device path
    def _table_index(self, size_in, size_out):
        """Word index of the (size_in, size_out) table { K, xmin[R], n[R], taps[K][R] } in the device tap buffer."""
        key = (int(size_in), int(size_out))
        if key not in self._index:
            xmin, n, k = self.taps(*key)
            words = np.concatenate([[k.shape[1]], xmin, n, k.T.reshape(-1)]).astype(np.int32)
            self._index[key] = self._n_words
            self._words.append(words)
            self._n_words += words.size
            self._dev_taps = None
        return self._index[key]

    def _taps_buffers(self):
        if self._dev_taps is None:
            host = np.ascontiguousarray(np.concatenate(self._words))
            self._dev_taps = (torch.from_numpy(host).to(self.device), host)
        return self._dev_taps

    def pack(self, frames):
        """frames -> (buffer uint8 on the device: the frames packed HWC, each padded to 16 bytes and copied with one H2D when they
        come from the host; desc: _lib.FrameDesc array)."""
        from . import _lib
        F = len(frames)
        desc = (_lib.FrameDesc * max(F, 1))()
        off = 0
        for i, f in enumerate(frames):
            H, W = int(f.shape[0]), int(f.shape[1])
            oh, ow, _, _ = self.plan(H, W)
            desc[i].offset, desc[i].height, desc[i].width = off, H, W
            desc[i].htab, desc[i].vtab = self._table_index(W, ow), self._table_index(H, oh)
            off += (H * W * 3 + 15) & ~15
        on_dev = [isinstance(f, torch.Tensor) and f.is_cuda for f in frames]
        if all(on_dev) and F:
            buf = torch.empty(max(off, 16), dtype=torch.uint8, device=self.device)
            for i, f in enumerate(frames):
                n = f.numel()
                buf[desc[i].offset:desc[i].offset + n].copy_(f.reshape(-1))
        else:
            host = torch.empty(max(off, 16), dtype=torch.uint8)
            if torch.cuda.is_available():
                host = host.pin_memory()
            hv = host.numpy()
            for i, f in enumerate(frames):
                a = f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else np.ascontiguousarray(f)
                hv[desc[i].offset:desc[i].offset + a.size] = a.reshape(-1)
            buf = host.to(self.device, non_blocking=True)
        return buf, desc

    def _gpu(self, frames, return_uint8):
        from . import ops
        F, R = len(frames), self.resolution
        pix = torch.empty((F, 3, R, R), device=self.device, dtype=torch.float32)
        u8 = torch.empty((F, R, R, 3), device=self.device, dtype=torch.uint8) if return_uint8 else None
        for f0 in range(0, F, ops.FRAME_PREP_MAX_FRAMES):
            f1 = min(F, f0 + ops.FRAME_PREP_MAX_FRAMES)
            buf, desc = self.pack(frames[f0:f1])
            taps, taps_host = self._taps_buffers()
            ops.frame_preprocess(buf, desc, f1 - f0, R, taps, taps_host, self.mean, self.std, pix[f0:f1],
                                 u8[f0:f1] if return_uint8 else None)
        return pix, u8

