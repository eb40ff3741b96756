"""The CLIP image encoder on a real MI355X: frames -> laff_clip_image_encode, against the reference's own outputs
(tests/golden/clip_image.npz) and the float64 restatement (tests/clip_image_ref.py: every row of every block) at full size."""
import ctypes as C

import numpy as np
import pytest
import torch

from clip_image_ref import RefImageFp16, encode_image64, fixture_config
from laff_amd import clip_image as CI

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rel_err(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


def fixture_encoder(golden, name, precision, **kw):
    cfg, sd, pix = fixture_config(golden('clip_image'), name)
    return cfg, sd, torch.from_numpy(pix), CI.ClipImageEncoder.from_state_dict(sd, precision=precision, device=DEV, **kw)


@pytest.mark.parametrize('precision,bound', [('fp32', 1e-5), ('fp16', 5e-3)])
@pytest.mark.parametrize('name', ['c0', 'c1'])
def test_fixture_parity(golden, name, precision, bound):
    z = golden('clip_image')
    cfg, sd, pix, enc = fixture_encoder(golden, name, precision)
    got = enc.encode_frames(pix)
    want = z[name + '/encode_image']
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_cuda
    err = rel_err(got.cpu().numpy(), want)
    print('fixture %s %s: max rel err %.3g' % (name, precision, err.max()))
    assert err.max() <= bound


# ---- full size, random weights at CLIP's init scales (LayerNorm affines and biases away from 1 / 0), frames ~ N(0, 1)
ARCH = {'B/32': (768, 12, 12, 32, 224, 512), 'B/16': (768, 12, 12, 16, 224, 512), 'L/14': (1024, 24, 16, 14, 224, 768)}
_SD = {}


def full_sd(arch, seed=5):
    if arch not in _SD:
        torch.manual_seed(seed)
        w, layers, heads, patch, res, embed = ARCH[arch]
        m = CI._ClipVisual(w, layers, patch, res, embed)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith('bias'):
                    p.normal_(0, 0.02, generator=g)
                elif 'ln_' in n:
                    p.normal_(1, 0.1, generator=g)
        _SD[arch] = {'visual.' + k: v.detach() for k, v in m.state_dict().items()}
    return _SD[arch]


def frames(F, res=224, seed=0):
    return torch.randn(F, 3, res, res, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize('arch,F', [('B/32', 1), ('B/32', 65), ('B/32', 1024), ('B/16', 64), ('L/14', 3)])
def test_full_size_against_float64(arch, F):
    sd = full_sd(arch)
    pix = frames(F, seed=F)
    want = encode_image64(pix, sd, device=DEV, chunk=128)
    with torch.no_grad():
        ref16 = RefImageFp16(sd, DEV)(pix.to(DEV)).float().cpu().numpy()
    e_torch = rel_err(ref16, want).max()
    for precision, bound in (('fp32', 1e-5), ('fp16', 5e-3)):
        enc = CI.ClipImageEncoder.from_state_dict(sd, precision=precision, device=DEV)
        got = enc.encode_frames(pix, max_frames=256).cpu().numpy()
        e = rel_err(got, want).max()
        print('%s F=%d %s: max rel err %.3g (torch fp16 path %.3g)' % (arch, F, precision, e, e_torch))
        assert e <= bound
        if precision == 'fp16':
            assert e <= e_torch


def test_batch_invariance_bitwise(golden):
    for precision in ('fp16', 'fp32'):
        sd = full_sd('B/32')
        enc = CI.ClipImageEncoder.from_state_dict(sd, precision=precision, device=DEV)
        pix = frames(23, seed=3)
        whole = enc.encode_frames(pix)
        for mf in (1, 4, 7, 16):
            assert torch.equal(enc.encode_frames(pix, max_frames=mf), whole), (precision, mf)
        for i in (0, 11, 22):
            assert torch.equal(enc.encode_frames(pix[i:i + 1])[0], whole[i])


def test_out_mean_is_the_mean_of_the_frames_ragged():
    enc = CI.ClipImageEncoder.from_state_dict(full_sd('B/32'), precision='fp16', device=DEV)
    counts = [1, 5, 2, 8, 3]
    vids = tuple(frames(c, seed=10 + i) for i, c in enumerate(counts))
    mean, feats, mask = enc.video_features(vids)
    alone = enc.encode_frames(torch.cat(vids))
    off = np.concatenate([[0], np.cumsum(counts)])
    assert feats.shape == (5, 8, 512) and mask.shape == (5, 8) and mask.dtype == torch.float32
    for v, c in enumerate(counts):
        assert torch.equal(feats[v, :c], alone[off[v]:off[v + 1]]) and int((feats[v, c:] != 0).sum()) == 0
        assert mask[v].tolist() == [1.0] * c + [0.0] * (8 - c)
        s = np.zeros(512, np.float32)
        for f in range(off[v], off[v + 1]):
            s += alone[f].cpu().numpy()
        assert np.allclose(mean[v].cpu().numpy(), s / np.float32(c), rtol=1e-6, atol=1e-7)
    assert torch.equal(enc(None, vids)['visual_features'], mean)
    m2, _, _ = enc.video_features(vids, max_frames=6)                  # calls of whole videos: the same means
    assert torch.equal(m2, mean)


def test_graph_capture_replays_the_eager_result(golden):
    for precision in ('fp16', 'fp32'):
        cfg, sd, pix, enc = fixture_encoder(golden, 'c1', precision)
        x = pix.to(DEV).contiguous()
        F = x.shape[0]
        fo = torch.tensor([0, 1, F], dtype=torch.int32, device=DEV)
        foh = np.array([0, 1, F], np.int32)
        ws = torch.empty(enc.workspace_bytes(F), dtype=torch.uint8, device=DEV)
        out = torch.empty(F, enc.embed_dim, device=DEV)
        mean = torch.empty(2, enc.embed_dim, device=DEV)
        enc.encode_batch(x, fo, foh, out=out, out_mean=mean, workspace=ws)        # eager first: packs weights, sets attributes
        torch.cuda.synchronize()
        want_o, want_m = out.clone(), mean.clone()
        out.zero_()
        mean.zero_()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                enc.encode_batch(x, fo, foh, out=out, out_mean=mean, workspace=ws)
        torch.cuda.current_stream().wait_stream(s)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_o) and torch.equal(mean, want_m)


def test_packed_weights_follow_parameter_updates(golden):
    cfg, sd, pix, enc = fixture_encoder(golden, 'c0', 'fp32')
    before = enc.encode_frames(pix)
    with torch.no_grad():
        enc.ClipModel.visual.conv1.weight.mul_(0.5)
        enc.ClipModel.visual.transformer.resblocks[1].mlp.c_proj.bias.add_(0.1)
    after = enc.encode_frames(pix)
    sd2 = {k: v.clone() for k, v in ((k, torch.from_numpy(v)) for k, v in sd.items())}
    sd2['visual.conv1.weight'] *= 0.5
    sd2['visual.transformer.resblocks.1.mlp.c_proj.bias'] += 0.1
    want = encode_image64(pix, sd2)
    assert not torch.equal(before, after) and rel_err(after.cpu().numpy(), want).max() <= 1e-5
    enc.load_state_dict({'ClipModel.' + k: torch.from_numpy(v) for k, v in sd.items()})
    assert torch.equal(enc.encode_frames(pix), before)


def test_refusals_launch_nothing(golden):
    from laff_amd import _lib, ops
    cfg, sd, pix, enc = fixture_encoder(golden, 'c0', 'fp16')
    lib = _lib.load()
    x = pix.to(DEV).contiguous()
    F = x.shape[0]
    model = enc._model()
    ws = torch.zeros(enc.workspace_bytes(F), dtype=torch.uint8, device=DEV)
    out = torch.full((F, enc.embed_dim), 7.0, device=DEV)
    mean = torch.full((2, enc.embed_dim), 7.0, device=DEV)
    fo = torch.tensor([0, 2, F], dtype=torch.int32, device=DEV)
    _, h = ops._context(x.device)

    def call(foh, nbytes=ws.numel(), m=model):
        arr = (C.c_int * 3)(*[int(v) for v in foh])
        return lib.laff_clip_image_encode(h, C.c_void_p(x.data_ptr()), F, C.c_void_p(fo.data_ptr()), arr, 2, C.byref(m), 1,
                                          C.c_void_p(out.data_ptr()), enc.embed_dim, C.c_void_p(mean.data_ptr()), enc.embed_dim,
                                          C.c_void_p(ws.data_ptr()), nbytes)
    assert call([0, 2, F], nbytes=ws.numel() - 1) == -1 and b'workspace too small' in lib.laff_last_error()
    assert call([0, 0, F]) == -1 and b'video 0 has 0 frames' in lib.laff_last_error()
    assert call([0, 2, F + 1]) == -1
    bad = _lib.ClipVisual.from_buffer_copy(model)
    bad.heads = 4
    assert call([0, 2, F], m=bad) == -5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mean == 7.0).all()) and int(ws.count_nonzero()) == 0
    assert call([0, 2, F]) == 0                                    # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.equal(out, enc.encode_frames(pix))


def test_predict_from_frames_end_to_end(golden):
    """A FrameLAFF model (the mean feature + the per-frame feature, frame_feat_with_video_feat=True) fed through ClipFrameLoader from
    frame tensors gives the score matrix and ranks of predict() fed the same features directly; its ranks are the float64 ranks of
    its own embeddings."""
    from oracle import laff_oracle as O
    from laff_amd import predictor
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    cfg_, sd, _, enc = fixture_encoder(golden, 'c0', 'fp16')
    E, H, D = enc.embed_dim, 4, 256
    cfg = make_config({'mean_clip': E}, {'CLIP': 48}, D, H, 'FrameLAFF', frame_feats={'clip_frame': E}, batch_norm=True,
                      vis_frame_attention='attention_noAveNoAverageMul', vis_frame_addFC=False, frame_feat_with_video_feat=True)
    torch.manual_seed(3)
    model = get_model('FrameLAFF', DEV, cfg).eval()
    Nv, Nt, bs = 40, 120, 16
    g = torch.Generator().manual_seed(21)
    counts = [1 + (i * 5) % 8 for i in range(Nv)]
    vids = [torch.randn(c, 3, 32, 32, generator=g) for c in counts]
    vis_ids = ['v%d' % i for i in range(Nv)]
    txt_ids = ['v%d#%d' % (i % Nv, i // Nv) for i in range(Nt)]
    clip_txt = torch.randn(Nt, 48, generator=g).to(DEV)

    class Frames:
        batch_size, dataset = bs, list(range(Nv))

        def __len__(self):
            return (Nv + bs - 1) // bs

        def __iter__(self):
            for s in range(0, Nv, bs):
                e = min(Nv, s + bs)
                yield {'vis_feat_dict': {}, 'idxs': list(range(s, e)), 'vis_ids': tuple(vis_ids[s:e]), 'vis_frame_feat_dict': {},
                       'vis_origin_frame_tuple': tuple(vids[s:e])}

    class Feats(Frames):
        def __iter__(self):
            for b in Frames.__iter__(self):
                mean, fr, mask = enc.video_features(b['vis_origin_frame_tuple'])
                yield dict(b, vis_feat_dict={'mean_clip': mean}, vis_frame_feat_dict={'clip_frame': fr, 'mask_tensor': mask},
                           vis_origin_frame_tuple=(None,) * len(b['idxs']))

    class Txt:
        batch_size, dataset = 50, list(range(Nt))

        def __len__(self):
            return (Nt + 49) // 50

        def __iter__(self):
            for s in range(0, Nt, 50):
                e = min(Nt, s + 50)
                yield {'CLIP_encoding': clip_txt[s:e]}, list(range(s, e)), tuple(txt_ids[s:e])
    loader = CI.ClipFrameLoader(Frames(), enc, mean_name='mean_clip', frame_name='clip_frame')
    S1, t1, v1 = model.predict(Txt(), loader, 'cosine')
    r1 = model.last_t2v_ranks.cpu().numpy()
    ve = model.video_all_embs.cpu().numpy()
    S2, t2, v2 = model.predict(Txt(), Feats(), 'cosine')
    r2 = model.last_t2v_ranks.cpu().numpy()
    assert list(t1) == list(t2) == txt_ids and list(v1) == list(v2) == vis_ids
    assert np.array_equal(S1, S2) and np.array_equal(r1, r2)
    te = model.txt_net({'CLIP_encoding': clip_txt}).detach().cpu().numpy()
    gt = predictor.gt_columns(txt_ids, vis_ids)
    want = O.count_ranks(O.txt2vis_matrix_f64(te.reshape(Nt, H, -1), ve.reshape(Nv, H, -1)), gt)
    assert np.array_equal(r1, want)
    assert len(set(want.tolist())) > 5
