"""The GRU caption encoder on a real MI355X: captions -> token ids -> laff_gru_encode, against the reference's own outputs
(tests/golden/gru_encoder.npz) and the float64 restatement (tests/gru_ref.py) at the reference's sizes."""
import numpy as np
import pytest
import torch

from gru_ref import gru_features
from laff_amd import txt2vec as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def fixture_encoder(golden, net, pooling):
    z = golden('gru_encoder')
    v = T.Vocabulary('gru')
    for w in z.json('vocab'):
        v.add(w)
    c = z.json('cfg')
    enc = T.GruTxtEncoder(T.IdxVec(v), c['we_dim'], c['H'], bidirectional=net == 'bigru', pooling=pooling, device=DEV)
    enc.load_state_dict({k: torch.from_numpy(a) for k, a in z.sub(net + '/sd/').items()}, strict=True)
    return z, enc


@pytest.mark.parametrize('net,pooling', [('gru', 'mean'), ('gru', 'last'), ('gru', 'mean_last'), ('bigru', 'mean'), ('bigru', 'last')])
def test_fixture_parity(golden, net, pooling):
    z, enc = fixture_encoder(golden, net, pooling)
    got = enc({'caption': z.json('captions')})['text_features']
    want = z['%s_%s' % (net, pooling)]
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_cuda
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-5


# ---- the reference's sizes: V = 11,286 words, we_dim = 500, rnn_size = 1024 -----------------------------------------------
V_FULL = 11286


def full_vocab():
    v = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + ['w%d' % i for i in range(V_FULL - 4)]:
        v.add(w)
    return v


def captions(g, n, lo=2, hi=128):
    """n captions of lengths lo..hi tokens (with <start>/<end>), a few unknown words among them."""
    lens = g.integers(lo, hi + 1, n)
    lens[0] = hi
    caps = []
    for L in lens:
        ws = ['w%d' % i for i in g.integers(0, V_FULL - 4, L - 2)]
        if L > 4:
            ws[1] = 'notaword'
        caps.append(' '.join(ws))
    return caps


def full_encoder(H, bidirectional=False, pooling='mean', seed=0):
    torch.manual_seed(seed)
    return T.GruTxtEncoder(T.IdxVec(full_vocab()), 500, H, bidirectional=bidirectional, pooling=pooling, device=DEV)


def sd64(enc):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in enc.state_dict().items()}


def check_rows(enc, caps, got, rows, pooling, bidirectional):
    """The float64 restatement of the given rows only (rows are independent of each other)."""
    ids = [enc.t2v_idx.encoding(caps[i]) for i in rows]
    want = gru_features(ids, sd64(enc), pooling, bidirectional)
    return float(np.abs(got[rows] - want).max())


_SHARED = {}


def shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


@pytest.mark.parametrize('N', [1, 63, 65, 4097])
@pytest.mark.parametrize('net,pooling', [('gru', 'mean'), ('gru', 'last'), ('bigru', 'mean')])
def test_full_size_against_float64(N, net, pooling):
    bi = net == 'bigru'
    enc = shared((net, pooling), lambda: full_encoder(1024, bi, pooling, seed=1 if bi else 0))
    g = np.random.default_rng(N)
    caps = captions(g, N)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    assert got.shape == (N, 2048 if bi and pooling == 'mean' else 1024) and np.isfinite(got).all()
    rows = np.unique(np.concatenate([[0, N - 1], g.integers(0, N, min(N, 48))]))
    assert check_rows(enc, caps, got, rows, pooling, bi) <= 1e-5


@pytest.mark.parametrize('H', [512, 2048])
def test_other_hidden_sizes(H):
    enc = full_encoder(H, seed=H)
    g = np.random.default_rng(H)
    caps = captions(g, 300)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    rows = np.unique(np.concatenate([[0], g.integers(0, 300, 24)]))
    assert check_rows(enc, caps, got, rows, 'mean', False) <= 1e-5


@pytest.mark.parametrize('net', ['gru', 'bigru'])
def test_batch_invariance(net):
    """A caption's features are bitwise the same alone, inside a shuffled batch of 4,097 and duplicated."""
    bi = net == 'bigru'
    enc = shared((net, 'mean'), lambda: full_encoder(1024, bi, 'mean', seed=1 if bi else 0))
    g = np.random.default_rng(99)
    caps = captions(g, 4097)
    big = enc({'caption': caps})['text_features']
    order = g.permutation(4097)
    shuf = enc({'caption': [caps[i] for i in order]})['text_features']
    assert torch.equal(shuf, big[torch.as_tensor(order, device=DEV)])
    for i in (0, 1, 17, 4096):
        alone = enc({'caption': [caps[i]]})['text_features']
        assert torch.equal(alone[0], big[i])
        dup = enc({'caption': [caps[i]] * 5 + [caps[(i + 1) % 4097]]})['text_features']
        for k in range(5):
            assert torch.equal(dup[k], big[i])


def test_tables_follow_the_weights(golden):
    """P and the packed W_hh are rebuilt after load_state_dict: the output follows the new weights."""
    z, enc = fixture_encoder(golden, 'gru', 'mean')
    caps = z.json('captions')
    first = enc({'caption': caps})['text_features'].cpu().numpy()
    assert np.abs(first - z['gru_mean']).max() <= 1e-5
    g = np.random.default_rng(5)
    new = {k: torch.from_numpy((a * 0.5 + g.normal(0, 0.05, a.shape)).astype(np.float32)) for k, a in z.sub('gru/sd/').items()}
    enc.load_state_dict(new, strict=True)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    want = gru_features([np.array(w) for w in z.json('ids')], {k: v.numpy().astype(np.float64) for k, v in new.items()})
    assert np.abs(got - want).max() <= 1e-5 and np.abs(got - first).max() > 1e-2
    with torch.no_grad():                                          # an in-place change of one parameter is seen as well
        enc.rnn.bias_hh_l0.add_(0.25)
    new['rnn.bias_hh_l0'] = new['rnn.bias_hh_l0'] + 0.25
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    want = gru_features([np.array(w) for w in z.json('ids')], {k: v.numpy().astype(np.float64) for k, v in new.items()})
    assert np.abs(got - want).max() <= 1e-5


@pytest.mark.parametrize('net', ['gru', 'bigru'])
def test_graph_capture_replays_the_eager_result(net):
    from laff_amd import ops
    bi = net == 'bigru'
    enc = shared((net, 'mean'), lambda: full_encoder(1024, bi, 'mean', seed=1 if bi else 0))
    caps = captions(np.random.default_rng(3), 1000, hi=40)
    b = enc.to_device(enc.t2v_idx.batch(caps))
    ws = torch.empty(ops.gru_workspace_bytes(len(caps), 1024, 1, bi, 'mean'), dtype=torch.uint8, device=DEV)
    eager = enc.encode_batch(b, workspace=ws).clone()
    out = torch.full_like(eager, float('nan'))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        enc.encode_batch(b, out=out, workspace=ws)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_text_tower_end_to_end_from_caption_strings():
    """LAFF text side rnn(1024) + bow + w2v + CLIP with all three computed encoders plugged in: predict() from caption strings +
    CLIP features; the text embeddings match the oracle tower fed the float64 GRU features, and the T2V ranks are the float64 ones."""
    from oracle import laff_oracle as O
    from laff_amd import predictor
    from laff_amd.config import make_config
    from laff_amd.model import get_model
    g = np.random.default_rng(21)
    H_heads, D = 4, 1024
    vid_dims = {'clip_ft': 512, 'x3d': 256}
    bow_words = ['w%d' % i for i in range(0, 300)]
    w2v_words = ['w%d' % i for i in range(0, 400, 2)]
    cfg = make_config(vid_dims, {'rnn': 1024, 'bow': len(bow_words), 'w2v': 20, 'CLIP': 512}, D, H_heads, 'LAFF', batch_norm=True)
    torch.manual_seed(8)
    model = get_model('LAFF', DEV, cfg).eval()
    gru = T.GruTxtEncoder(T.IdxVec(full_vocab()), 500, 1024, device=DEV)
    bow = T.BowVec(bow_words, stopwords=())
    w2v = T.W2Vec(w2v_words, g.normal(0, 1, (len(w2v_words), 20)).astype(np.float32), stopwords=())
    enc = model.txt_net.encoder
    enc.rnn_encoder, enc.bow_encoder, enc.w2v_encoder = gru, T.BoWTxtEncoder(bow, DEV), T.W2VTxtEncoder(w2v, DEV)
    Nv, per = 64, 2
    vis_ids = ['v%d' % i for i in range(Nv)]
    txt_ids = ['v%d#%d' % (i, k) for i in range(Nv) for k in range(per)]
    Nt = len(txt_ids)
    caps = captions(g, Nt, hi=30)
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
    # the oracle on the float64 GRU features of the same captions
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    feats = {'rnn_encoder': gru_features([gru.t2v_idx.encoding(c) for c in caps], sd64(gru)),
             'bow_encoder': np.stack([bow.encoding(c) for c in caps]).astype(np.float32),
             'w2v_encoder': np.stack([w2v.encoding(c) for c in caps]).astype(np.float32), 'CLIP_encoder': clip}
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
