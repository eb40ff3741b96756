"""The CLIP text encoder on a real MI355X: caption strings -> ClipTokenizer -> laff_clip_encode, against the reference's own outputs
(tests/golden/clip_text.npz) and the float64 restatement (tests/clip_ref.py: all 77 positions, dense causal mask) at full size."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from clip_ref import RefTextFp16, encode_text64, full_text_sd
from conftest import GOLDEN
from laff_amd import clip_text as CT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BPE = os.path.join(GOLDEN, 'clip_bpe_subset.txt.gz')
_SHARED = {}


def shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


def tokenizer():
    return shared('tok', lambda: CT.ClipTokenizer(BPE))


def fixture_encoder(golden, precision):
    z = golden('clip_text')
    return z, CT.ClipTxtEncoder.from_state_dict(full_text_sd(z), tokenizer(), precision=precision, device=DEV)


def rel_err(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


@pytest.mark.parametrize('precision,bound', [('fp32', 1e-5), ('fp16', 5e-3)])
def test_fixture_parity(golden, precision, bound):
    z, enc = fixture_encoder(golden, precision)
    got = enc({'caption': z.json('captions')})['text_features']
    want = z['encode_text']
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_cuda
    g = got.cpu().numpy()
    if precision == 'fp32':
        assert np.abs(g - want).max() <= bound
    assert rel_err(g, want).max() <= bound


# ---- full size: ViT-B/32 text (512 / 8 / 12 / 512) and ViT-L/14 text (768 / 12 / 12 / 768), random weights at CLIP's init scales
def full_sd(width, layers, embed, seed):
    """A text state dict with CLIP.initialize_parameters' scales, plus LayerNorm affines and biases away from 1 / 0."""
    torch.manual_seed(seed)
    m = CT._ClipText(width, layers, embed, 77, 49408)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias'):
                p.normal_(0, 0.02, generator=g)
            elif '.ln_' in '.' + n:
                p.normal_(1, 0.1, generator=g)
    return {k: v.detach() for k, v in m.state_dict().items()}


def dense_ids(g, n):
    """n rows of 77 ids: a planted <|endoftext|> at a random position (lengths 1..77, row 0 of 77 included), or a truncated row
    (<|startoftext|> first, no <|endoftext|>: the reference pools position 0), with random BPE ids everywhere else."""
    ids = g.integers(0, 49406, (n, 77))
    ids[:, 0] = 49406
    p = g.integers(0, 77, n)
    p[0], p[-1] = 76, 0
    trunc = g.random(n) < 0.1
    trunc[0] = False
    for i in range(n):
        if not trunc[i]:
            ids[i, p[i]] = 49407
    return ids


def ragged(ids):
    p = ids.argmax(axis=1)
    row_off = np.zeros(len(ids) + 1, np.int32)
    row_off[1:] = np.cumsum(p + 1)
    flat = np.concatenate([ids[i, :p[i] + 1] for i in range(len(ids))]).astype(np.int32)
    return CT.ClipBatch(flat, row_off, row_off)


def full_encoder(cfg, precision):
    width, layers, embed = cfg

    def make():
        sd = full_sd(width, layers, embed, seed=width)
        return sd, {p: CT.ClipTxtEncoder.from_state_dict(sd, tokenizer(), precision=p, device=DEV) for p in ('fp32', 'fp16')}
    sd, encs = shared(cfg, make)
    return sd, encs[precision]


@pytest.mark.parametrize('cfg', [(512, 12, 512), (768, 12, 768)])
@pytest.mark.parametrize('N', [1, 65, 4097])
def test_full_size_against_float64(cfg, N):
    sd, e32 = full_encoder(cfg, 'fp32')
    _, e16 = full_encoder(cfg, 'fp16')
    ids = dense_ids(np.random.default_rng(N + cfg[0]), N)
    b = e32.to_device(ragged(ids))
    want = encode_text64(ids, sd, device=DEV)
    err32 = rel_err(e32.encode_batch(b).cpu().numpy().astype(np.float64), want)
    err16 = rel_err(e16.encode_batch(b).cpu().numpy().astype(np.float64), want)
    ref = RefTextFp16(sd)(torch.from_numpy(ids).to(DEV)).float().cpu().numpy().astype(np.float64)
    err_ref = rel_err(ref, want)
    print('N=%d cfg=%s: fp32 max %.2e  fp16 max %.2e mean %.2e  torch-fp16 max %.2e mean %.2e'
          % (N, cfg, err32.max(), err16.max(), err16.mean(), err_ref.max(), err_ref.mean()))
    assert err32.max() <= 1e-5
    assert err16.max() <= 5e-3
    assert err16.max() <= err_ref.max() and err16.mean() <= err_ref.mean()


def test_batch_invariance_is_bitwise():
    """A caption's feature is the same alone, inside a batch of 4,097 and under different chunk sizes (row budgets)."""
    _, enc = full_encoder((512, 12, 512), 'fp16')
    g = np.random.default_rng(41)
    words = ['dog', 'cat', 'man', 'playing', 'guitar', 'on', 'the', 'stage', 'a', 'red', 'car', 'is', 'running', '3d', "it's", '!!']
    caps = [' '.join(g.choice(words, int(g.integers(0, 30)))) for _ in range(4097)]
    caps[7] = ' '.join(['word'] * 100)                             # cut at 77 tokens
    big = enc.encode(caps)
    for budget in (77, 1000, 12345):
        assert torch.equal(enc.encode(caps, max_rows=budget), big)
    for i in (0, 7, 4096):
        assert torch.equal(enc.encode([caps[i]])[0], big[i])
        dup = enc.encode([caps[(i + 1) % 4097], caps[i], caps[i]])
        assert torch.equal(dup[1], big[i]) and torch.equal(dup[2], big[i])
    order = g.permutation(4097)
    assert torch.equal(enc.encode([caps[i] for i in order]), big[torch.as_tensor(order, device=DEV)])


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_packed_weights_follow_the_parameters(golden, precision):
    z, enc = fixture_encoder(golden, precision)
    caps = z.json('captions')
    first = enc({'caption': caps})['text_features'].cpu().numpy()
    g = np.random.default_rng(5)
    sd = full_text_sd(z)
    new = {k: (a * 0.8 + g.normal(0, 0.02, a.shape)).astype(np.float32) for k, a in sd.items()}
    enc.ClipModel.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=True)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    want = encode_text64(z['ids'], new)
    tol = 1e-5 if precision == 'fp32' else 5e-3
    assert rel_err(got, want).max() <= tol and np.abs(got - first).max() > 1e-2
    with torch.no_grad():                                          # an in-place change of one parameter is seen as well
        enc.ClipModel.transformer.resblocks[1].mlp.c_proj.weight.mul_(-1.0)
        enc.ClipModel.text_projection.copy_(torch.from_numpy(new['text_projection'] * 2).to(DEV))
    new['transformer.resblocks.1.mlp.c_proj.weight'] = -new['transformer.resblocks.1.mlp.c_proj.weight']
    new['text_projection'] = new['text_projection'] * 2
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    assert rel_err(got, encode_text64(z['ids'], new)).max() <= tol


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_graph_capture_replays_the_eager_result(precision):
    _, enc = full_encoder((512, 12, 512), precision)
    ids = dense_ids(np.random.default_rng(3), 1000)
    b = enc.to_device(ragged(ids))
    ws = torch.empty(enc.workspace_bytes(b), dtype=torch.uint8, device=DEV)
    eager = enc.encode_batch(b, workspace=ws).clone()
    out = torch.full_like(eager, float('nan'))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        enc.encode_batch(b, out=out, workspace=ws)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_refusals_launch_nothing():
    """Head dim 32, width 1088, context 78 and a malformed row_off: an error code, and the output buffer is untouched."""
    from laff_amd import _lib, ops
    _, enc = full_encoder((512, 12, 512), 'fp16')
    b = enc.to_device(ragged(dense_ids(np.random.default_rng(9), 8)))
    enc.encode_batch(b)                                            # builds the packed weights
    model = enc._model()
    lib, h = ops._context(torch.device(DEV))
    out = torch.full((8, 512), 7.0, device=DEV)
    ws = torch.zeros(enc.workspace_bytes(b) * 2, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def call(m, roh):
        roh = np.ascontiguousarray(roh, np.int32)
        return lib.laff_clip_encode(h, C.c_void_p(b.ids.data_ptr()), C.c_void_p(b.row_off.data_ptr()),
                                    roh.ctypes.data_as(C.POINTER(C.c_int)), 8, int(roh[-1]), C.byref(m), 1,
                                    C.c_void_p(out.data_ptr()), 512, C.c_void_p(ws.data_ptr()), ws.numel())

    def variant(**kw):
        fields = {f: getattr(model, f) for f, _ in _lib.ClipText._fields_}
        fields.update(kw)
        return _lib.ClipText(**fields)
    roh = b.row_off_host
    assert call(variant(heads=16), roh) == -5 and b'head dim' in lib.laff_last_error()
    assert call(variant(width=1088, heads=17), roh) == -5 and b'width=1088' in lib.laff_last_error()
    assert call(variant(context_length=78), roh) == -5 and b'context_length=78' in lib.laff_last_error()
    bad = roh.copy()
    bad[3] = bad[2]
    assert call(model, bad) == -1 and b'row_off' in lib.laff_last_error()
    bad = roh.copy()
    bad[1] = bad[0] + 78
    assert call(model, bad) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(ws.count_nonzero()) == 0
    assert call(model, roh) == 0                                   # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.equal(out, enc.encode_batch(b))


def test_predict_from_caption_strings_end_to_end(golden):
    """tiny_c1 (bow + no-transform CLIP of dim 64) with ClipTxtEncoder plugged into txt_net.encoder.CLIP_encoder: predict() from
    caption strings gives the score matrix and ranks of predict() fed the same features as 'CLIP_encoding', and its ranks are the
    float64 ranks of its own embeddings."""
    from oracle import laff_oracle as O
    from laff_amd import predictor, synth
    Nt, Nv, H, d, _ = synth.WORKLOADS['tiny_c1']
    spec = synth.SPECS['tiny_c1']
    model = synth.build_model(H, d, torch.device(DEV), spec=spec)
    vis, txt, _, _ = synth.make_features(Nt, Nv, torch.device(DEV), spec=spec)
    bow = txt['bow_encoding']
    bow = bow.to_dense() if bow.layout != torch.strided else bow
    z, clip = fixture_encoder(golden, 'fp16')
    model.txt_net.encoder.CLIP_encoder = clip
    g = np.random.default_rng(17)
    words = ['a', 'man', 'woman', 'dog', 'plays', 'guitar', 'dances', 'in', 'the', 'park', 'kitchen', 'car', 'news', 'cat', 'red']
    caps = [' '.join(g.choice(words, int(g.integers(2, 14)))) for _ in range(Nt)]
    vis_ids = ['v%d' % i for i in range(Nv)]
    txt_ids = ['v%d#%d' % (i // 20, i % 20) for i in range(Nt)]
    vis_np = {n: v.cpu() for n, v in vis.items()}
    feats = clip.encode(caps)

    class Vis:
        batch_size, dataset = 16, list(range(Nv))

        def __len__(self):
            return 2

        def __iter__(self):
            for s in range(0, Nv, 16):
                e = min(Nv, s + 16)
                yield {'vis_feat_dict': {n: v[s:e] for n, v in vis_np.items()}, 'idxs': list(range(s, e)), 'vis_ids': tuple(vis_ids[s:e]),
                       'vis_frame_feat_dict': {}, 'vis_origin_frame_tuple': (None,) * (e - s)}

    class Txt:
        batch_size, dataset = 100, list(range(Nt))

        def __init__(self, with_clip):
            self.with_clip = with_clip

        def __len__(self):
            return (Nt + 99) // 100

        def __iter__(self):
            for s in range(0, Nt, 100):
                e = min(Nt, s + 100)
                d_ = {'caption': caps[s:e], 'bow_encoding': bow[s:e]}
                if self.with_clip:
                    d_['CLIP_encoding'] = feats[s:e]
                yield d_, list(range(s, e)), tuple(txt_ids[s:e])
    S1, t1, v1 = model.predict(Txt(False), Vis(), 'cosine')
    r1 = model.last_t2v_ranks.cpu().numpy()
    S2, t2, v2 = model.predict(Txt(True), Vis(), 'cosine')
    r2 = model.last_t2v_ranks.cpu().numpy()
    assert list(t1) == list(t2) == txt_ids and list(v1) == list(v2) == vis_ids
    assert np.array_equal(S1, S2) and np.array_equal(r1, r2)
    te = model.txt_net({'caption': caps, 'bow_encoding': bow}).detach().cpu().numpy()
    ve = model.video_all_embs.cpu().numpy()
    gt = predictor.gt_columns(txt_ids, vis_ids)
    want = O.count_ranks(O.txt2vis_matrix_f64(te.reshape(Nt, H, -1), ve.reshape(Nv, H, -1)), gt)
    assert np.array_equal(r1, want)
    assert len(set(want.tolist())) > 8
