"""The NetVLAD text encoder on a real MI355X: captions -> W2Vec table rows -> laff_netvlad_encode, against the reference's own outputs
(tests/golden/netvlad_text.npz) and the float64 restatement (tests/netvlad_ref.py) at the reference's sizes."""
import ctypes as C

import numpy as np
import pytest
import torch

from netvlad_ref import netvlad_features
from laff_amd import txt2vec as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def fixture_encoder(golden, K):
    z = golden('netvlad_text')
    w2v = T.W2Vec(z.json('words'), z['table'], stopwords=z.json('stopwords'))
    enc = T.NetVLADTxtEncoder(w2v, num_clusters=K, device=DEV)
    enc.load_state_dict({k: torch.from_numpy(a) for k, a in z.sub('k%d/sd/' % K).items()}, strict=True)
    return z, enc


@pytest.mark.parametrize('K', [8, 32])
def test_fixture_parity(golden, K):
    z, enc = fixture_encoder(golden, K)
    got = enc({'caption': z.json('captions')})['text_features']
    want = z['k%d/out' % K]
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_cuda
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-5


# ---- the reference's sizes: a 100k-word table of width 500 (300), 32 clusters (8, 64) -----------------------------------------
V_FULL = 100000
_SHARED = {}


def full_w2v(D, seed=0):
    key = ('w2v', D)
    if key not in _SHARED:
        g = np.random.default_rng(seed)
        table = g.normal(0, 1, (V_FULL, D)).astype(np.float32)
        table[7] = 0.0                                                    # a zero-norm row ('w7')
        _SHARED[key] = T.W2Vec(['w%d' % i for i in range(V_FULL)], table, stopwords=('a', 'the'))
    return _SHARED[key]


def full_encoder(K, D, seed=0):
    key = ('enc', K, D)
    if key not in _SHARED:
        torch.manual_seed(seed)
        _SHARED[key] = T.NetVLADTxtEncoder(full_w2v(D), num_clusters=K, device=DEV)
    return _SHARED[key]


def captions(g, n, hi=14):
    """n captions of 1..hi words, a few unknown words and stop words among them."""
    caps = []
    for L in g.integers(1, hi + 1, n):
        ws = ['w%d' % i for i in g.integers(0, V_FULL, L)]
        if L > 3:
            ws[1], ws[2] = 'notaword', 'the'
        caps.append(' '.join(ws))
    return caps


def want_rows(enc, caps, rows):
    v = enc.netvlad
    return netvlad_features([enc.t2v_w2v.raw_ids(caps[i]) for i in rows], enc.t2v_w2v.table.numpy(),
                            v.fc1.weight.detach().cpu().numpy(), v.centeroids.detach().cpu().numpy())


@pytest.mark.parametrize('K,D,N', [(32, 500, 1), (32, 500, 4097), (32, 500, 40000), (8, 300, 2000), (64, 300, 2000)])
def test_full_size_against_float64(K, D, N):
    enc = full_encoder(K, D)
    g = np.random.default_rng(N + K)
    caps = captions(g, N)
    got = enc({'caption': caps})['text_features']
    assert tuple(got.shape) == (N, K * D) and bool(torch.isfinite(got).all())
    rows = np.unique(np.concatenate([[0, N - 1], g.integers(0, N, min(N, 64))]))
    err = float(np.abs(got[torch.as_tensor(rows, device=DEV)].cpu().numpy() - want_rows(enc, caps, rows)).max())
    print('K=%d D=%d N=%d: max |err| vs float64 = %.3g' % (K, D, N, err))
    assert err <= 5e-6


def test_edge_captions():
    """Empty, punctuation only, stop words only, unknown only, a zero-norm row, repeats, and 300+ distinct known words (38 LDS chunks
    carried through the output row)."""
    enc = full_encoder(32, 500)
    g = np.random.default_rng(77)
    long_caps = [' '.join('w%d' % i for i in g.choice(V_FULL, n, replace=False)) for n in (8, 9, 17, 333, 700)]
    caps = ['', '?!', 'the a the', 'zebra quokka', 'w7', 'w7 w8', 'w8 w8 w9 w8', 'the w7 zebra'] + long_caps
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    err = float(np.abs(got - want_rows(enc, caps, range(len(caps)))).max())
    print('edge captions: max |err| vs float64 = %.3g' % err)
    assert err <= 5e-6
    assert not got[0].any() and not got[1].any() and not got[2].any()
    assert np.array_equal(got[3], got[4])                               # unknown only == one zero-norm row: -c_k/|c_k|/sqrt(K)
    assert len(enc.t2v_w2v.raw_ids(caps[-1])[0]) == 700


def test_batch_invariance():
    """A caption's row is bitwise the same alone, inside a shuffled batch, in a smaller batch and duplicated."""
    enc = full_encoder(32, 500)
    g = np.random.default_rng(99)
    caps = captions(g, 3001, hi=40) + [' '.join('w%d' % i for i in range(1000, 1350))]
    big = enc({'caption': caps})['text_features']
    order = g.permutation(len(caps))
    shuf = enc({'caption': [caps[i] for i in order]})['text_features']
    assert torch.equal(shuf, big[torch.as_tensor(order, device=DEV)])
    part = enc({'caption': caps[500:700]})['text_features']
    assert torch.equal(part, big[500:700])
    for i in (0, 1, 17, len(caps) - 1):
        alone = enc({'caption': [caps[i]]})['text_features']
        assert torch.equal(alone[0], big[i])
        dup = enc({'caption': [caps[i]] * 3 + [caps[(i + 1) % len(caps)]]})['text_features']
        for k in range(3):
            assert torch.equal(dup[k], big[i])


def test_output_follows_the_weights(golden):
    z, enc = fixture_encoder(golden, 32)
    caps = z.json('captions')
    first = enc({'caption': caps})['text_features'].cpu().numpy()
    g = np.random.default_rng(5)
    new = {k: torch.from_numpy((a * 0.5 + g.normal(0, 0.05, a.shape)).astype(np.float32)) for k, a in z.sub('k32/sd/').items()}
    enc.load_state_dict(new, strict=True)
    rows = [enc.t2v_w2v.raw_ids(c) for c in caps]
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    want = netvlad_features(rows, z['table'], new['netvlad.fc1.weight'].numpy(), new['netvlad.centeroids'].numpy())
    assert np.abs(got - want).max() <= 1e-5 and np.abs(got - first).max() > 1e-2
    with torch.no_grad():                                               # an in-place change of one parameter is seen as well
        enc.netvlad.centeroids.mul_(-1.0)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    want = netvlad_features(rows, z['table'], new['netvlad.fc1.weight'].numpy(), -new['netvlad.centeroids'].numpy())
    assert np.abs(got - want).max() <= 1e-5


def test_graph_capture_replays_the_eager_result():
    from laff_amd import ops
    enc = full_encoder(32, 500)
    caps = captions(np.random.default_rng(3), 1000, hi=30)
    ids, row_off, zero_rows = enc.t2v_w2v.ragged(caps)
    b = enc.to_device(ids, row_off, zero_rows)
    ws = torch.empty(ops.netvlad_workspace_bytes(len(ids), 32), dtype=torch.uint8, device=DEV)
    eager = enc.encode_batch(*b, workspace=ws).clone()
    out = torch.full_like(eager, float('nan'))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        enc.encode_batch(*b, out=out, workspace=ws)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_refusals_launch_nothing():
    """Bad offsets, K and ldo on real device buffers: an error, and the output keeps its sentinel."""
    from laff_amd import _lib, ops
    enc = full_encoder(32, 500)
    v, table = enc.netvlad, enc.t2v_w2v.device_table(DEV)
    ids = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32, device=DEV)
    ro = torch.tensor([0, 3, 5], dtype=torch.int32, device=DEV)
    zr = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((2, 32 * 500), 7.0, device=DEV)
    ws = torch.empty(ops.netvlad_workspace_bytes(5, 32), dtype=torch.uint8, device=DEV)
    lib, h = ops._context(table.device)
    P = ops._ptr

    def call(roh=(0, 3, 5), K=32, ldo=32 * 500, R=5):
        r = (C.c_int * len(roh))(*roh)
        return lib.laff_netvlad_encode(h, P(table), V_FULL, 500, P(ids), P(ro), r, P(zr), 2, R, P(v.fc1.weight), P(v.centeroids), K,
                                       P(out), ldo, P(ws), ws.numel())
    assert call(roh=(0, 3, 4)) == -1 and call(roh=(0, 6, 5), R=5) == -1 and call(K=65) == -5 and call(ldo=100) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    with pytest.raises(ValueError, match='zero_rows'):
        ops.netvlad_encode(table, ids, ro, [0, 3, 5], zr[:1], v.fc1.weight.detach(), v.centeroids.detach())
    assert _lib.load() is lib


def test_text_tower_end_to_end_from_caption_strings():
    """LAFF text side w2v + NetVLAD + CLIP with the w2v and NetVLAD encoders plugged in (one shared W2Vec): predict() from caption
    strings + CLIP features; the text embeddings match the oracle tower fed the float64 NetVLAD features, and the T2V ranks are the
    float64 ones."""
    from oracle import laff_oracle as O
    from laff_amd import predictor
    from laff_amd.config import make_config
    from laff_amd.model import get_model
    g = np.random.default_rng(21)
    H_heads, D, K, Dw = 4, 1024, 16, 40
    vid_dims = {'clip_ft': 512, 'x3d': 256}
    words = ['w%d' % i for i in range(400)]
    w2v = T.W2Vec(words, g.normal(0, 1, (len(words), Dw)).astype(np.float32), stopwords=('the',))
    cfg = make_config(vid_dims, {'w2v': Dw, 'CLIP': 512, 'NetVLAD': K}, D, H_heads, 'LAFF', batch_norm=True)
    torch.manual_seed(8)
    model = get_model('LAFF', DEV, cfg).eval()
    vlad = T.NetVLADTxtEncoder(w2v, num_clusters=K, device=DEV)
    enc = model.txt_net.encoder
    enc.w2v_encoder, enc.NetVLAD_encoder = T.W2VTxtEncoder(w2v, DEV), vlad
    assert model.txt_net.encoder_name_list == ['w2v_encoder', 'CLIP_encoder', 'NetVLAD_encoder']
    Nv, per = 64, 2
    vis_ids = ['v%d' % i for i in range(Nv)]
    txt_ids = ['v%d#%d' % (i, k) for i in range(Nv) for k in range(per)]
    Nt = len(txt_ids)
    caps = [' '.join('w%d' % i for i in g.integers(0, 500, int(g.integers(1, 12)))) for _ in range(Nt)]
    caps[0], caps[1] = '', 'the zebra'
    caption_of = dict(zip(txt_ids, caps))
    clip = g.normal(0, 1, (Nt, 512)).astype(np.float32)
    vis = {n: g.normal(0, 1, (Nv, d)).astype(np.float32) for n, d in vid_dims.items()}

    class Vis:
        batch_size, dataset = 32, list(range(Nv))

        def __len__(self):
            return 2

        def __iter__(self):
            for s in range(0, Nv, 32):
                yield {'vis_feat_dict': {n: torch.from_numpy(v[s:s + 32]) for n, v in vis.items()}, 'idxs': list(range(s, s + 32)),
                       'vis_ids': tuple(vis_ids[s:s + 32]), 'vis_frame_feat_dict': {}, 'vis_origin_frame_tuple': (None,) * 32}

    class Txt:
        batch_size, dataset = 50, list(range(Nt))

        def __len__(self):
            return (Nt + 49) // 50

        def __iter__(self):
            for s in range(0, Nt, 50):
                e = min(Nt, s + 50)
                yield ({'caption': [caption_of[i] for i in txt_ids[s:e]], 'CLIP_encoding': torch.from_numpy(clip[s:e])},
                       list(range(s, e)), tuple(txt_ids[s:e]))
    scores, out_txt, out_vis = model.predict(Txt(), Vis(), 'cosine', record_emb=True)
    assert list(out_txt) == txt_ids and list(out_vis) == vis_ids
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    v = vlad.netvlad
    feats = {'w2v_encoder': np.stack([w2v.encoding(c) for c in caps]).astype(np.float32), 'CLIP_encoder': clip,
             'NetVLAD_encoder': netvlad_features([w2v.raw_ids(c) for c in caps], w2v.table.numpy(), v.fc1.weight.detach().cpu().numpy(),
                                                 v.centeroids.detach().cpu().numpy())}
    tspecs = [O.feature_spec(sd, 'txt_net.transform_layer.%s_transform.' % e, feats[e], 'tanh', H_heads, False)
              for e in model.txt_net.encoder_name_list]
    vspecs = [O.feature_spec(sd, 'vis_net.VisMutiTransformNet.%s.' % n, vis[n], 'tanh', H_heads, False) for n in vid_dims]
    te = O.fuse_tower(tspecs, O.attention_from_sd(sd, 'txt_net.attention_layer.', H_heads, False, False), H_heads)
    ve = O.fuse_tower(vspecs, O.attention_from_sd(sd, 'vis_net.attention_layer.', H_heads, False, False), H_heads)
    cap = {'caption': caps, 'CLIP_encoding': torch.from_numpy(clip)}
    got_te = model.txt_net(cap).detach().cpu().numpy().reshape(te.shape)
    assert np.abs(got_te - te).max() <= 5e-6 * max(1.0, float(np.abs(te).max()))
    assert np.abs(model.video_all_embs.cpu().numpy().reshape(ve.shape) - ve).max() <= 5e-6
    gt = predictor.gt_columns(out_txt, out_vis)
    want = O.count_ranks(O.txt2vis_matrix_f64(te.reshape(Nt, H_heads, -1), ve.reshape(Nv, H_heads, -1)), gt)
    assert np.array_equal(model.last_t2v_ranks.cpu().numpy(), want)
    assert len(set(want.tolist())) > 8
