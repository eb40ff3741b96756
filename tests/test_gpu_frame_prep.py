"""Frame preprocessing on the device (laff_frame_preprocess, laff_amd/csrc/frame_prep.hip) against the Pillow fixture and, at full
size, against tests/frame_prep_ref.py (which tests/test_frame_prep_host.py pins to that fixture): the uint8 image bit for bit, the fp32
pixels within two ulps."""
import numpy as np
import pytest
import torch

import frame_prep_ref as REF
from laff_amd import clip_image as CI
from laff_amd import frame_prep as FP

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINDS = ('clip', 'slip')
FP32_BOUND = 4.8e-7          # two fp32 ulps at |x| < 4, which bounds every normalised value


def synth(h, w, seed):
    """A smooth pattern plus noise with saturated patches, seeded."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 120 * np.sin(x / 9.0 + c) * np.cos(y / 6.0 - c) for c in range(3)], axis=-1) + rng.normal(0, 30, (h, w, 3))
    img[(x.astype(int) // 16 + y.astype(int) // 16) % 7 == 0] *= 3.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def check(got_pix, got_u8, frames, R, kind, tag):
    for i, img in enumerate(frames):
        want_pix, want_u8 = REF.preprocess(img, R, kind)
        u8 = got_u8[i].cpu().numpy()
        wrong = int((u8 != want_u8).sum())
        err = float(np.abs(got_pix[i].cpu().numpy().astype(np.float64) - want_pix).max())
        print('%s %s frame %d %s: %d wrong bytes, fp32 max |diff| %.3g' % (tag, kind, i, img.shape, wrong, err))
        assert wrong == 0
        assert err <= FP32_BOUND


def test_fixture_parity(golden):
    z = golden('frame_prep')
    meta = z.json('meta')
    for kind in KINDS:
        for R in sorted({m['R'] for m in meta.values()}):
            group = [n for n in sorted(meta) if meta[n]['R'] == R]
            pre = FP.FramePreprocessor(R, kind=kind, device=DEV)
            pix, u8 = pre([z[n + '/frame'] for n in group], return_uint8=True)
            assert pix.is_cuda and pix.shape == (len(group), 3, R, R) and pix.dtype == torch.float32
            assert u8.shape == (len(group), R, R, 3) and u8.dtype == torch.uint8
            for i, n in enumerate(group):
                assert np.array_equal(u8[i].cpu().numpy(), z['%s/%s/u8' % (n, kind)]), (n, kind)
                key = '%s/%s/pixels' % (n, kind)
                if key in z:
                    err = float(np.abs(pix[i].cpu().numpy().astype(np.float64) - z[key]).max())
                    print('fixture %s %s: fp32 max |diff| %.3g' % (n, kind, err))
                    assert err <= FP32_BOUND
            assert torch.equal(pre([z[n + '/frame'] for n in group]), pix)         # without the uint8 copy: the same pixels


@pytest.mark.parametrize('kind', KINDS)
def test_full_size_mixed_batch(kind):
    sizes = [(1080, 1920), (720, 1280), (360, 640), (640, 360), (120, 160), (224, 224), (224, 301), (1080, 1920)]
    frames = [synth(h, w, 100 + i) for i, (h, w) in enumerate(sizes)]
    pre = FP.FramePreprocessor(224, kind=kind, device=DEV)
    pix, u8 = pre(frames, return_uint8=True)
    check(pix, u8, frames, 224, kind, 'mixed')


def test_other_resolutions_and_extreme_shapes():
    for R, sizes in ((512, [(2160, 3840), (600, 512), (50, 70)]), (64, [(1080, 1920), (4096, 300), (3, 500)]), (1, [(37, 53)]),
                     (336, [(480, 854)])):
        frames = [synth(h, w, R + i) for i, (h, w) in enumerate(sizes)]
        pix, u8 = FP.FramePreprocessor(R, kind='clip', device=DEV)(frames, return_uint8=True)
        check(pix, u8, frames, R, 'clip', 'R=%d' % R)


def test_alone_in_a_batch_and_at_an_unaligned_offset():
    from laff_amd import _lib, ops
    R = 224
    frames = [synth(h, w, 7 + i) for i, (h, w) in enumerate([(360, 640), (1080, 1920), (333, 251), (120, 160)])]
    for kind in KINDS:
        pre = FP.FramePreprocessor(R, kind=kind, device=DEV)
        pix, u8 = pre(frames, return_uint8=True)
        for i, f in enumerate(frames):
            a_pix, a_u8 = pre([f], return_uint8=True)                               # alone (another row tiling for the small ones)
            assert torch.equal(a_pix[0], pix[i]) and torch.equal(a_u8[0], u8[i]), (kind, i)
            d_pix = pre([torch.from_numpy(f).to(DEV)])                              # from a device tensor
            assert torch.equal(d_pix[0], pix[i])
        rev_pix = pre(frames[::-1])
        assert torch.equal(rev_pix.flip(0), pix)
        # frames packed back to back behind an odd byte offset: no alignment is assumed
        desc = (_lib.FrameDesc * len(frames))()
        off, parts = 3, [np.zeros(3, np.uint8)]
        for i, f in enumerate(frames):
            oh, ow, _, _ = pre.plan(*f.shape[:2])
            desc[i].offset, desc[i].height, desc[i].width = off, f.shape[0], f.shape[1]
            desc[i].htab, desc[i].vtab = pre._table_index(f.shape[1], ow), pre._table_index(f.shape[0], oh)
            parts += [f.reshape(-1), np.zeros(1 + i, np.uint8)]
            off += f.size + 1 + i
        assert any(desc[i].offset % 2 for i in range(len(frames))) and any(desc[i].offset % 4 for i in range(len(frames)))
        buf = torch.from_numpy(np.concatenate(parts)).to(DEV)
        taps, taps_host = pre._taps_buffers()
        out8 = torch.empty(len(frames), R, R, 3, dtype=torch.uint8, device=DEV)
        out = ops.frame_preprocess(buf, desc, len(frames), R, taps, taps_host, pre.mean, pre.std, out_u8=out8)
        assert torch.equal(out, pix) and torch.equal(out8, u8)


def test_graph_capture_replays_the_eager_result():
    from laff_amd import ops
    R = 224
    frames = [synth(h, w, 40 + i) for i, (h, w) in enumerate([(360, 640), (720, 1280), (160, 120)])]
    pre = FP.FramePreprocessor(R, kind='clip', device=DEV)
    buf, desc = pre.pack(frames)
    taps, taps_host = pre._taps_buffers()
    desc_dev = ops.frame_desc_device(desc, len(frames), buf.device)
    out = torch.empty(len(frames), 3, R, R, device=DEV)
    out8 = torch.empty(len(frames), R, R, 3, dtype=torch.uint8, device=DEV)
    args = (buf, desc, len(frames), R, taps, taps_host, pre.mean, pre.std)
    ops.frame_preprocess(*args, out=out, out_u8=out8, desc_dev=desc_dev)                   # eager first
    torch.cuda.synchronize()
    want, want8 = out.clone(), out8.clone()
    assert torch.equal(want, pre(frames))
    out.zero_()
    out8.zero_()
    s = torch.cuda.Stream()                                                                 # one stream, no parallel branches
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            ops.frame_preprocess(*args, out=out, out_u8=out8, desc_dev=desc_dev)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out8, want8)


def test_refusals_launch_nothing():
    import ctypes as C
    from laff_amd import _lib, ops
    lib = _lib.load()
    R = 64
    frames = [synth(90, 130, 1)]
    pre = FP.FramePreprocessor(R, device=DEV)
    buf, desc = pre.pack(frames)
    taps, taps_host = pre._taps_buffers()
    desc_dev = ops.frame_desc_device(desc, 1, buf.device)
    out = torch.full((1, 3, R, R), 7.0, device=DEV)
    _, h = ops._context(buf.device)
    mean, std = (C.c_float * 3)(*pre.mean), (C.c_float * 3)(*pre.std)

    def call(nbytes=buf.numel(), R_=R):
        return lib.laff_frame_preprocess(h, C.c_void_p(buf.data_ptr()), nbytes, C.c_void_p(desc_dev.data_ptr()), C.cast(desc, C.c_void_p),
                                         1, R_, C.c_void_p(taps.data_ptr()), C.c_void_p(taps_host.ctypes.data), taps_host.size, mean, std,
                                         C.c_void_p(out.data_ptr()), None, None, 0)
    assert call(nbytes=90 * 130 * 3 - 1) == -1 and b'outside' in lib.laff_last_error()
    assert call(R_=513) == -5
    desc[0].height = 4097
    assert call() == -5
    desc[0].height = 89                                     # the vertical table reads row 89
    assert call() == -1 and b'vertical table entry' in lib.laff_last_error()
    desc[0].height = 90
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0                                      # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.equal(out, pre(frames))
    with pytest.raises(ValueError):
        pre([np.zeros((8, 8, 3), np.float32)])


# ---- through the encoder
ARCH = (128, 2, 2, 16, 64, 32)       # width, layers, heads, patch, resolution, embed


def small_encoder(precision='fp16'):
    torch.manual_seed(11)
    return CI.ClipImageEncoder(*ARCH, precision=precision, device=DEV)


def test_encode_raw_frames_is_preprocess_then_encode():
    frames = [synth(h, w, 60 + i) for i, (h, w) in enumerate([(360, 640), (200, 150), (64, 64), (50, 40), (1080, 1920)])]
    for precision in ('fp16', 'fp32'):
        enc = small_encoder(precision)
        for kind in KINDS:
            pre = FP.FramePreprocessor(enc.input_resolution, kind=kind, device=DEV)
            want = enc.encode_frames(pre(frames))
            got = enc.encode_raw_frames(frames, kind=kind)
            assert got.shape == (len(frames), enc.embed_dim) and torch.equal(got, want), (precision, kind)
            assert bool(torch.isfinite(got).all())
        assert not torch.equal(enc.encode_raw_frames(frames, kind='clip'), enc.encode_raw_frames(frames, kind='slip'))
    enc = small_encoder()
    same = np.stack([synth(120, 160, 70 + i) for i in range(5)])
    assert torch.equal(enc.encode_raw_frames(torch.from_numpy(same)), enc.encode_raw_frames(list(same)))   # one [F, H, W, 3] tensor
    full = CI.ClipImageEncoder(768, 1, 12, 32, 224, 512, precision='fp16', device=DEV)                    # at the B/32 resolution
    assert torch.equal(full.encode_raw_frames(frames[:2]), full.encode_frames(full.preprocessor()(frames[:2])))


def test_video_features_raw_and_frame_loader():
    enc = small_encoder()
    counts = [1, 4, 2, 3]
    sizes = [(360, 640), (640, 360), (100, 100), (240, 320)]
    vids = [[synth(h, w, 1000 + 10 * v + j) for j in range(c)] for v, (c, (h, w)) in enumerate(zip(counts, sizes))]
    pre = enc.preprocessor()
    fp32 = tuple(pre(v) for v in vids)
    want = enc.video_features(fp32)
    got = enc.video_features_raw(vids)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(enc.video_features_raw([np.stack(v) for v in vids]), want))

    class Loader:
        batch_size, dataset = 2, list(range(4))

        def __init__(self, raw, stacked=False):
            self.raw, self.stacked = raw, stacked

        def __len__(self):
            return 2

        def __iter__(self):
            for s in (0, 2):
                src = ([torch.from_numpy(np.stack(v)) for v in vids] if self.stacked else vids) if self.raw else fp32
                yield {'vis_feat_dict': {'other': torch.ones(2, 3)}, 'vis_frame_feat_dict': {}, 'idxs': [s, s + 1],
                       'vis_ids': ('v%d' % s, 'v%d' % (s + 1)), 'vis_origin_frame_tuple': tuple(src[s:s + 2])}

    def run(loader):
        return list(CI.ClipFrameLoader(loader, enc, mean_name='mean_clip', frame_name='clip_frame'))
    ref = run(Loader(False))
    for got in (run(Loader(True)), run(Loader(True, stacked=True)),
                list(CI.ClipFrameLoader(Loader(True), enc, mean_name='mean_clip', frame_name='clip_frame',
                                        preprocessor=FP.FramePreprocessor(enc.input_resolution, device=DEV)))):
        assert len(got) == len(ref) == 2
        for g, r in zip(got, ref):
            assert torch.equal(g['vis_feat_dict']['mean_clip'], r['vis_feat_dict']['mean_clip'])
            assert torch.equal(g['vis_feat_dict']['other'], r['vis_feat_dict']['other'])
            assert torch.equal(g['vis_frame_feat_dict']['clip_frame'], r['vis_frame_feat_dict']['clip_frame'])
            assert torch.equal(g['vis_frame_feat_dict']['mask_tensor'], r['vis_frame_feat_dict']['mask_tensor'])
    slip = list(CI.ClipFrameLoader(Loader(True), enc, mean_name='mean_clip', frame_name='clip_frame',
                                   preprocessor=FP.FramePreprocessor(enc.input_resolution, kind='slip', device=DEV)))
    assert not torch.equal(slip[0]['vis_feat_dict']['mean_clip'], ref[0]['vis_feat_dict']['mean_clip'])
