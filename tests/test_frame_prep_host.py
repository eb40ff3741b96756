"""Frame preprocessing without a GPU: tests/frame_prep_ref.py (the independent restatement) and the library's CPU path
(laff_amd.frame_prep.FramePreprocessor(device='cpu'), the arithmetic the kernel runs) against tests/golden/frame_prep.npz, which holds
what Pillow itself gives (tools/gen_golden_frame_prep.py)."""
import numpy as np
import pytest
import torch

import frame_prep_ref as REF
from laff_amd import frame_prep as FP

KINDS = ('clip', 'slip')
FP32_BOUND = 4.8e-7          # two fp32 ulps at |x| < 4, which bounds every normalised value


def names(z):
    return sorted(z.json('meta'))


def test_fixture_covers_the_cases(golden):
    z = golden('frame_prep')
    meta = z.json('meta')
    assert len(meta) >= 12
    shapes = {n: z[n + '/frame'].shape for n in meta}
    assert any(h < w for h, w, _ in shapes.values()) and any(h > w for h, w, _ in shapes.values())
    assert any(min(s[:2]) == meta[n]['R'] == max(s[:2]) for n, s in shapes.items())               # square at R
    assert any(min(s[:2]) < meta[n]['R'] for n, s in shapes.items())                              # enlarged
    assert any(min(s[:2]) >= 4 * meta[n]['R'] for n, s in shapes.items())                         # a large downscale
    diffs = {max(m['out_height'], m['out_width']) - m['R'] for m in meta.values()}
    assert 73 in diffs and 75 in diffs                                                            # both half-to-even cases
    assert len({m['R'] for m in meta.values()}) >= 2
    assert sum(1 for k in z.z.files if k.endswith('/pixels')) == 2


def test_restatement_reproduces_pillow_bit_for_bit(golden):
    z = golden('frame_prep')
    for n in names(z):
        m = z.json('meta')[n]
        for kind in KINDS:
            u8, plan = REF.resize_crop(z[n + '/frame'], m['R'], kind)
            assert plan == (m['out_height'], m['out_width'], m['top'], m['left']), (n, kind)
            assert u8.dtype == np.uint8 and np.array_equal(u8, z['%s/%s/u8' % (n, kind)]), (n, kind)


def test_cpu_path_reproduces_pillow_bit_for_bit(golden):
    z = golden('frame_prep')
    meta = z.json('meta')
    for kind in KINDS:
        for R in sorted({m['R'] for m in meta.values()}):
            pre = FP.FramePreprocessor(R, kind=kind, device='cpu')
            group = [n for n in names(z) if meta[n]['R'] == R]
            pix, u8 = pre([z[n + '/frame'] for n in group], return_uint8=True)             # one mixed batch
            assert pix.shape == (len(group), 3, R, R) and pix.dtype == torch.float32 and u8.dtype == torch.uint8
            for i, n in enumerate(group):
                assert np.array_equal(u8[i].numpy(), z['%s/%s/u8' % (n, kind)]), (n, kind)
                alone, alone8 = pre([torch.from_numpy(z[n + '/frame'])], return_uint8=True)    # torch input, alone: the same bits
                assert torch.equal(alone8[0], u8[i]) and torch.equal(alone[0], pix[i])


def test_fp32_stage(golden):
    z = golden('frame_prep')
    seen = 0
    for key in z.z.files:
        if not key.endswith('/pixels'):
            continue
        n, kind, _ = key.split('/')
        want = z[key]
        R = z.json('meta')[n]['R']
        ref = REF.normalise(z['%s/%s/u8' % (n, kind)], kind)
        got = FP.FramePreprocessor(R, kind=kind, device='cpu')([z[n + '/frame']])[0].numpy()
        for name, x in (('restatement', ref), ('cpu path', got)):
            err = float(np.abs(x.astype(np.float64) - want).max())
            print('%s %s %s: max |diff| %.3g, equal %s' % (n, kind, name, err, np.array_equal(x, want)))
            assert x.dtype == np.float32 and x.shape == want.shape
            assert err <= FP32_BOUND
            assert np.array_equal(x, want)          # the same fp32 operations in the same order: equality holds
        assert float(np.abs(want).max()) < 4.0
        seen += 1
    assert seen == 2


def test_sizes_and_crop_offsets():
    # Resize(R): short side to R with int() truncation; unchanged when the short side already is R
    assert FP.resized_size(240, 320, 224) == (224, 298) and FP.resized_size(320, 240, 224) == (298, 224)
    assert FP.resized_size(1080, 1920, 224) == (224, 398) and FP.resized_size(360, 640, 224) == (224, 398)
    assert FP.resized_size(224, 500, 224) == (224, 500) and FP.resized_size(500, 224, 224) == (500, 224)
    assert FP.resized_size(224, 100, 224) == (501, 224)                     # the SHORT side decides: 100 -> 224
    assert FP.resized_size(120, 160, 224) == (224, 298)                     # enlarged
    assert FP.resized_size(7, 7, 224) == (224, 224)
    # CenterCrop: halves to even
    assert FP.crop_offsets(224, 224 + 75, 224) == (0, 38) and FP.crop_offsets(224, 224 + 73, 224) == (0, 36)
    assert FP.crop_offsets(224 + 75, 224, 224) == (38, 0) and FP.crop_offsets(224 + 73, 224, 224) == (36, 0)
    assert FP.crop_offsets(224, 398, 224) == (0, 87) and FP.crop_offsets(224, 225, 224) == (0, 0) and FP.crop_offsets(224, 227, 224) == (0, 2)
    for h, w, R in ((90, 173, 80), (90, 175, 80), (480, 640, 224), (33, 4000, 64), (1000, 3, 17)):
        pre = FP.FramePreprocessor(R, device='cpu')
        oh, ow, top, left = pre.plan(h, w)
        assert (oh, ow) == REF.output_size(h, w, R) and min(oh, ow) == R
        assert 0 <= top <= oh - R and 0 <= left <= ow - R
        # the window's tap table is the full axis' table, cut at the crop
        for size_in, size_out, first in ((w, ow, left), (h, oh, top)):
            xmin, n, k = pre.taps(size_in, size_out)
            assert xmin.shape == (R,) and int(xmin.min()) >= 0 and int((xmin + n).max()) <= size_in and int(n.min()) >= 1
            if size_in != size_out and size_out <= 4096:
                full = REF.coefficients(size_in, size_out, REF.bicubic, 2.0)[first:first + R]
                assert [int(v) for v in xmin] == [c[0] for c in full]
                assert [list(map(int, k[j, :n[j]])) for j in range(R)] == [c[1] for c in full]


@pytest.mark.parametrize('sample_frame', [1, 8, 16])
def test_sample_frame_indices(sample_frame):
    for n in (1, sample_frame - 1, sample_frame, sample_frame + 1, 3 * sample_frame + 5, 1000):
        if n < 1:
            continue
        got = FP.sample_frame_indices(n, sample_frame)
        assert np.array_equal(got, np.linspace(0, n - 1, sample_frame, dtype=int)) and got.shape == (sample_frame,)
        assert got[0] == 0 and got.max() <= n - 1 and np.all(np.diff(got) >= 0)
        if sample_frame > 1:
            assert got[-1] == n - 1


def test_refusals():
    pre = FP.FramePreprocessor(32, device='cpu')
    ok = np.zeros((40, 50, 3), np.uint8)
    assert pre([ok]).shape == (1, 3, 32, 32) and pre(np.zeros((2, 40, 50, 3), np.uint8)).shape == (2, 3, 32, 32)
    for bad in (np.zeros((40, 50, 3), np.float32), np.zeros((40, 50, 3), np.int32), np.zeros((40, 50, 4), np.uint8),
                np.zeros((40, 50), np.uint8), np.zeros((3, 40, 50), np.uint8), torch.zeros(40, 50, 3), torch.zeros(40, 50, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            pre([bad])
    with pytest.raises(ValueError):
        pre(np.zeros((2, 2, 40, 50, 3), np.uint8))
    with pytest.raises(ValueError):
        pre(['frame.jpg'])
    with pytest.raises(ValueError):
        FP.FramePreprocessor(32, kind='imagenet', device='cpu')
    for R in (0, -1, 513):
        with pytest.raises(NotImplementedError):
            FP.FramePreprocessor(R, device='cpu')
    for shape in ((4097, 10, 3), (10, 4097, 3), (0, 10, 3)):
        with pytest.raises(NotImplementedError):
            pre([np.zeros(shape, np.uint8)])
    assert FP.FramePreprocessor(512, device='cpu').resolution == 512 and pre([np.zeros((1, 1, 3), np.uint8)]).shape == (1, 3, 32, 32)


def test_c_abi_refuses_before_any_gpu_work():
    """The limits of include/laff_hip.h are checked on the host, before the ctx is looked at."""
    import ctypes as C
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.laff_frame_preprocess_workspace_bytes(8, 224, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_frame_preprocess_workspace_bytes(8, 513, C.byref(n)) == -5
    pre = FP.FramePreprocessor(16, device='cpu')
    xmin, cnt, k = pre.taps(40, 16)
    words = np.concatenate([[k.shape[1]], xmin, cnt, k.T.reshape(-1)]).astype(np.int32)
    desc = (_lib.FrameDesc * 1)()
    mean, std = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    one = C.c_void_p(16)                     # a non-null placeholder: nothing is dereferenced on the device before the checks end

    def call(R=16, F=1, h=40, w=40, off=0, nbytes=40 * 40 * 3, tab=0, tw=words, sd=std):
        desc[0].offset, desc[0].height, desc[0].width, desc[0].htab, desc[0].vtab = off, h, w, tab, tab
        return lib.laff_frame_preprocess(None, one, nbytes, one, C.cast(desc, C.c_void_p), F, R, one, C.c_void_p(tw.ctypes.data), tw.size,
                                         mean, sd, one, None, None, 0)
    assert call() == -1 and b'null ctx' in lib.laff_last_error()              # every check passed; only the ctx is missing
    assert call(F=0) == 0
    assert call(R=0) == -5 and call(R=513) == -5 and call(F=65536) == -5
    assert call(h=4097) == -5 and call(w=0) == -5 and b'each side' in lib.laff_last_error()
    assert call(nbytes=40 * 40 * 3 - 1) == -1 and b'outside' in lib.laff_last_error()
    assert call(off=1, nbytes=40 * 40 * 3 + 1) == -1 and b'null ctx' in lib.laff_last_error()     # an unaligned offset is legal
    assert call(off=-1) == -1
    assert call(tab=5) == -1 and call(tab=-1) == -1
    assert call(h=39) == -1 and b'vertical table entry' in lib.laff_last_error()    # the table reads row 39 of a 39-row frame
    assert call(w=39) == -1 and b'horizontal table entry' in lib.laff_last_error()
    bad = words.copy()
    bad[1] = -1
    assert call(tw=bad) == -1
    bad = words.copy()
    bad[0] = 100
    assert call(tw=bad) == -1 and b'runs past' in lib.laff_last_error()
    assert call(sd=(C.c_float * 3)(1, 0, 1)) == -1
    # a vertical tap count whose single output row does not fit the LDS image is refused, not approximated
    R = 512
    K = 65536 // (3 * R) + 1
    big = np.concatenate([[K], np.zeros(R), np.full(R, K), np.zeros(K * R)]).astype(np.int32)
    assert call(R=R, h=4096, w=4096, nbytes=4096 * 4096 * 3, tw=big) == -5 and b'LDS' in lib.laff_last_error()


def test_live_pillow_on_seeded_random_sizes():
    """Additional, where Pillow is installed: random sizes and both filters against Image.resize itself."""
    Image = pytest.importorskip('PIL.Image')
    rng = np.random.default_rng(7)
    for kind, flt in (('clip', Image.BICUBIC), ('slip', Image.BILINEAR)):
        for R in (224, 48):
            pre = FP.FramePreprocessor(R, kind=kind, device='cpu')
            for _ in range(6):
                h, w = (int(v) for v in rng.integers(20, 700, 2))
                img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                oh, ow, top, left = pre.plan(h, w)
                pil = Image.fromarray(img, 'RGB')
                if (ow, oh) != (w, h):
                    pil = pil.resize((ow, oh), flt)
                want = np.asarray(pil)[top:top + R, left:left + R]
                assert np.array_equal(pre([img], return_uint8=True)[1][0].numpy(), want), (kind, R, h, w)
                assert np.array_equal(REF.resize_crop(img, R, kind)[0], want), (kind, R, h, w)


def test_frame_prep_hip_kernel_has_no_spills_no_scratch_and_no_float_before_the_normalise(tmp_path):
    """frame_prep_kernel: 0 VGPR / SGPR spills, no scratch, no MFMA; the resample is integer only, so the only floating-point
    divides are the normalise's."""
    import os
    import re
    import subprocess
    import sys
    from conftest import ROOT
    from laff_amd import build
    assert 'frame_prep.hip' in build.SOURCES
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'frame_prep.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'frame_prep.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'frame_prep', quiet=True)
    assert len(stats) == 1, sorted(stats)
    text = open(asm[0]).read()
    for name, st in stats.items():
        assert st['scratch'] == 0 and st['mfma'] == 0, (name, st)
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
