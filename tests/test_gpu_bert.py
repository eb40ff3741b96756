"""The BERT text encoder on a real MI355X: caption strings -> BertTokenizer -> laff_bert_encode, against the reference's own outputs
(tests/golden/bert_text.npz) and the float64 restatement (tests/bert_ref.py: padded batches with the dense key mask) at bert-base
and bert-large shapes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from bert_ref import RefBert, encode64, full_bert_sd, padded
from conftest import GOLDEN
from laff_amd import bert_text as BT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
VOCAB = os.path.join(GOLDEN, 'bert_vocab.txt')
_SHARED = {}


def shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


def fixture_encoder(golden, precision):
    z = golden('bert_text')
    return z, BT.BertTxtEncoder.from_state_dict(full_bert_sd(z), BT.BertTokenizer(VOCAB), precision=precision, device=DEV)


def rel_err(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_fixture_parity(golden, precision):
    z, enc = fixture_encoder(golden, precision)
    got = enc({'caption': z.json('captions')})['text_features']
    want = z['pooler_output']
    assert got.shape == want.shape and got.dtype == torch.float32 and got.is_cuda
    g = got.cpu().numpy()
    err = np.abs(g - want).max() if precision == 'fp32' else rel_err(g, want).max()
    print('fixture %s: %.2e' % (precision, err))
    assert err <= (1e-5 if precision == 'fp32' else 5e-3)


# ---- full size: bert-base (768 / 12 heads / 12 layers / 3072, vocab 30,522) and the bert-large shape (1024 / 16 / 24 / 4096)
BASE, LARGE = (768, 12, 12, 3072), (1024, 16, 24, 4096)


def config(shape):
    W, H, layers, inter = shape
    return {'hidden_size': W, 'num_attention_heads': H, 'num_hidden_layers': layers, 'intermediate_size': inter,
            'max_position_embeddings': 512, 'vocab_size': 30522, 'type_vocab_size': 2, 'layer_norm_eps': 1e-12}


def full_sd(shape, seed):
    """BertConfig's init (std 0.02) with the LayerNorm affines and biases moved off 1 / 0."""
    torch.manual_seed(seed)
    W, _, layers, inter = shape
    m = BT._BertModel(W, layers, inter, 512, 30522, 2)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith('bias'):
                p.normal_(0, 0.02, generator=g)
            elif 'LayerNorm' in n:
                p.normal_(1, 0.1, generator=g)
    return {k: v.detach() for k, v in m.state_dict().items()}


def full_encoder(shape, precision):
    """The shape's encoders in both precisions; their tokenizer is the fixture vocabulary's (ids below 377 of the 30,522)."""
    def make():
        sd = full_sd(shape, seed=shape[0])
        tok = BT.BertTokenizer(VOCAB)
        return sd, {p: BT.BertTxtEncoder.from_state_dict(sd, tok, precision=p, device=DEV, config=config(shape))
                    for p in ('fp32', 'fp16')}
    sd, encs = shared(shape, make)
    return sd, encs[precision]


SPECIAL_LENGTHS = [1, 2, 63, 64, 65, 128, 129, 511, 512]


def lengths(g, n):
    """Caption lengths over 1..512 with the tile edges included; for larger n mostly MSR-VTT-like (5..30) with a tenth uniform."""
    L = g.integers(1, 513, n) if n < 1000 else np.where(g.random(n) < 0.1, g.integers(1, 513, n), g.integers(5, 31, n))
    L[:min(n, len(SPECIAL_LENGTHS))] = SPECIAL_LENGTHS[:n] if n < len(SPECIAL_LENGTHS) else SPECIAL_LENGTHS
    if n == 1:
        L[0] = 512
    return L


def ragged(g, lens, vocab=30522):
    row_off = np.zeros(len(lens) + 1, np.int32)
    row_off[1:] = np.cumsum(lens)
    ids = g.integers(104, vocab, int(row_off[-1])).astype(np.int32)
    ids[row_off[:-1]] = 101
    ids[row_off[1:][lens > 1] - 1] = 102
    return BT.BertBatch(ids, row_off, row_off)


def float64(b, sd, chunk=32):
    """The float64 restatement, padded, in chunks of similar length (any padding is exact; sorting only saves work)."""
    lens = np.diff(b.row_off_host)
    order = np.argsort(lens, kind='stable')
    ids, mask = padded(b.row_off_host, b.ids)
    out = np.empty((len(lens), sd['pooler.dense.bias'].shape[0]))
    for s in range(0, len(order), chunk):
        sel = order[s:s + chunk]
        out[sel] = encode64(ids[sel], mask[sel], sd, device=DEV, chunk=chunk)
    return out


def torch_path(b, sd, dtype, chunk=32):
    ref = RefBert(sd, dtype)
    lens = np.diff(b.row_off_host)
    order = np.argsort(lens, kind='stable')
    ids, mask = padded(b.row_off_host, b.ids)
    out = np.empty((len(lens), sd['pooler.dense.bias'].shape[0]))
    for s in range(0, len(order), chunk):
        sel = order[s:s + chunk]
        L = int(lens[sel].max())
        out[sel] = ref(torch.from_numpy(ids[sel, :L]).to(DEV), torch.from_numpy(mask[sel, :L]).to(DEV)).double().cpu().numpy()
    return out


@pytest.mark.parametrize('N', [1, 65, 4097])
def test_bert_base_against_float64(N):
    sd, e32 = full_encoder(BASE, 'fp32')
    _, e16 = full_encoder(BASE, 'fp16')
    g = np.random.default_rng(N)
    b = ragged(g, lengths(g, N))
    db = e32.to_device(b)
    want = float64(b, sd)
    err32 = rel_err(e32.encode_batch(db).cpu().numpy().astype(np.float64), want)
    err16 = rel_err(e16.encode_batch(db).cpu().numpy().astype(np.float64), want)
    err_ref = rel_err(torch_path(b, sd, torch.float16), want)
    print('bert-base N=%d rows=%d: fp32 max %.2e  fp16 max %.2e mean %.2e  torch-fp16 max %.2e mean %.2e'
          % (N, b.row_off_host[-1], err32.max(), err16.max(), err16.mean(), err_ref.max(), err_ref.mean()))
    assert err32.max() <= 1e-5
    assert err16.max() <= 5e-3


def test_bert_large_shape_against_float64():
    sd, e32 = full_encoder(LARGE, 'fp32')
    _, e16 = full_encoder(LARGE, 'fp16')
    g = np.random.default_rng(24)
    b = ragged(g, np.array([1, 2, 17, 64, 65, 200, 512]))
    db = e32.to_device(b)
    want = float64(b, sd)
    err32 = rel_err(e32.encode_batch(db).cpu().numpy().astype(np.float64), want)
    err16 = rel_err(e16.encode_batch(db).cpu().numpy().astype(np.float64), want)
    print('bert-large: fp32 max %.2e  fp16 max %.2e' % (err32.max(), err16.max()))
    assert err32.max() <= 1e-5
    assert err16.max() <= 5e-3


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_batch_invariance_is_bitwise(precision):
    """A caption's feature is the same alone, inside a batch and under different chunk sizes (row budgets)."""
    _, enc = full_encoder(BASE, precision)
    g = np.random.default_rng(41)
    words = ['dog', 'cat', 'man', 'playing', 'guitar', 'on', 'the', 'stage', 'a', 'red', 'car', 'is', 'running', '3', "it's", '!!',
             'café', '中文']
    caps = [' '.join(g.choice(words, int(g.integers(0, 30)))) for _ in range(1500)]
    caps[7] = ' '.join(['word'] * 600)                               # cut at 512 tokens
    caps[8] = ''
    big = enc.encode(caps)
    for budget in (512, 3000, 12345):
        assert torch.equal(enc.encode(caps, max_rows=budget), big)
    for i in (0, 7, 8, 1499):
        assert torch.equal(enc.encode([caps[i]])[0], big[i])
        dup = enc.encode([caps[(i + 1) % 1500], caps[i], caps[i]])
        assert torch.equal(dup[1], big[i]) and torch.equal(dup[2], big[i])
    order = g.permutation(1500)
    assert torch.equal(enc.encode([caps[i] for i in order]), big[torch.as_tensor(order, device=DEV)])


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_packed_weights_follow_the_parameters(golden, precision):
    z, enc = fixture_encoder(golden, precision)
    caps = z.json('captions')
    first = enc({'caption': caps})['text_features'].cpu().numpy()
    g = np.random.default_rng(5)
    sd = full_bert_sd(z)
    new = {k: (a * 0.8 + g.normal(0, 0.02, a.shape)).astype(np.float32) for k, a in sd.items()}
    enc.BertModel.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=True)
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    tol = 1e-5 if precision == 'fp32' else 5e-3
    assert rel_err(got, encode64(z['ids'], z['mask'], new)).max() <= tol and np.abs(got - first).max() > 1e-2
    with torch.no_grad():                                              # an in-place change of one parameter is seen as well
        enc.BertModel.encoder.layer[1].attention.self.value.weight.mul_(-1.0)
        enc.BertModel.pooler.dense.bias.copy_(torch.from_numpy(new['pooler.dense.bias'] * 2).to(DEV))
    new['encoder.layer.1.attention.self.value.weight'] = -new['encoder.layer.1.attention.self.value.weight']
    new['pooler.dense.bias'] = new['pooler.dense.bias'] * 2
    got = enc({'caption': caps})['text_features'].cpu().numpy()
    assert rel_err(got, encode64(z['ids'], z['mask'], new)).max() <= tol


@pytest.mark.parametrize('precision', ['fp32', 'fp16'])
def test_graph_capture_replays_the_eager_result(precision):
    _, enc = full_encoder(BASE, precision)
    g = np.random.default_rng(3)
    b = enc.to_device(ragged(g, lengths(g, 1000)))
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
    """Head dim 32, width 1088, an intermediate size off the GEMM's step, 513 positions and malformed row offsets: an error code,
    and the output and the workspace are untouched."""
    from laff_amd import _lib, ops
    _, enc = full_encoder(BASE, 'fp16')
    g = np.random.default_rng(9)
    b = enc.to_device(ragged(g, lengths(g, 8)))
    enc.encode_batch(b)                                                # builds the packed weights
    model = enc._model()
    lib, h = ops._context(torch.device(DEV))
    out = torch.full((8, 768), 7.0, device=DEV)
    ws = torch.zeros(enc.workspace_bytes(b) * 2, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()

    def call(m, roh):
        roh = np.ascontiguousarray(roh, np.int32)
        return lib.laff_bert_encode(h, C.c_void_p(b.ids.data_ptr()), C.c_void_p(b.row_off.data_ptr()),
                                    roh.ctypes.data_as(C.POINTER(C.c_int)), 8, int(roh[-1]), C.byref(m), 1,
                                    C.c_void_p(out.data_ptr()), 768, C.c_void_p(ws.data_ptr()), ws.numel())

    def variant(**kw):
        fields = {f: getattr(model, f) for f, _ in _lib.BertText._fields_}
        fields.update(kw)
        return _lib.BertText(**fields)
    roh = b.row_off_host
    assert call(variant(heads=24), roh) == -5 and b'head dim' in lib.laff_last_error()
    assert call(variant(width=1088, heads=17), roh) == -5 and b'width=1088' in lib.laff_last_error()
    assert call(variant(intermediate=3000), roh) == -5 and b'intermediate=3000' in lib.laff_last_error()
    assert call(variant(max_position=513), roh) == -5 and b'max_position=513' in lib.laff_last_error()
    bad = roh.copy()
    bad[3] = bad[2]
    assert call(model, bad) == -1 and b'row_off' in lib.laff_last_error()
    bad = roh.copy()
    bad[1:] += 512 - (bad[1] - bad[0]) + 1                             # caption 0 of 513 rows
    assert call(model, bad) == -1 and b'513 rows' in lib.laff_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(ws.count_nonzero()) == 0
    assert call(model, roh) == 0                                       # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.equal(out, enc.encode_batch(b))


def test_predict_from_caption_strings_end_to_end(golden):
    """A tiny LAFF model with bow and bert (the fixture's 128-wide encoder) among its text features: predict() from caption strings,
    with BertTxtEncoder in txt_net.encoder.bert_encoder, gives the score matrix and ranks of predict() fed the same features as
    'bert_encoding'."""
    from laff_amd.config import make_config
    from laff_amd.model import get_model
    Nt, Nv, H = 240, 32, 2
    torch.manual_seed(7)
    cfg = make_config({'clip_ft': 64, 'x3d': 96}, {'bow': 333, 'bert': 128}, H * 64, H, 'LAFF', batch_norm=True)
    model = get_model('LAFF', torch.device(DEV), cfg).eval()
    _, bert = fixture_encoder(golden, 'fp32')
    model.txt_net.encoder.bert_encoder = bert.eval()
    g = np.random.default_rng(17)
    words = ['a', 'man', 'woman', 'dog', 'plays', 'guitar', 'dances', 'in', 'the', 'park', 'kitchen', 'car', 'news', 'cat', 'red']
    caps = [' '.join(g.choice(words, int(g.integers(2, 14)))) for _ in range(Nt)]
    vis = {'clip_ft': torch.from_numpy(g.normal(size=(Nv, 64)).astype(np.float32)),
           'x3d': torch.from_numpy(g.normal(size=(Nv, 96)).astype(np.float32))}
    bow = torch.from_numpy((g.random((Nt, 333)) < 0.02).astype(np.float32)).to(DEV)
    vis_ids = ['v%d' % i for i in range(Nv)]
    txt_ids = ['v%d#%d' % (i // 8, i % 8) for i in range(Nt)]
    feats = bert.encode(caps)

    class Vis:
        batch_size, dataset = 16, list(range(Nv))

        def __len__(self):
            return 2

        def __iter__(self):
            for s in range(0, Nv, 16):
                e = min(Nv, s + 16)
                yield {'vis_feat_dict': {n: v[s:e] for n, v in vis.items()}, 'idxs': list(range(s, e)), 'vis_ids': tuple(vis_ids[s:e]),
                       'vis_frame_feat_dict': {}, 'vis_origin_frame_tuple': (None,) * (e - s)}

    class Txt:
        batch_size, dataset = 100, list(range(Nt))

        def __init__(self, with_bert):
            self.with_bert = with_bert

        def __len__(self):
            return (Nt + 99) // 100

        def __iter__(self):
            for s in range(0, Nt, 100):
                e = min(Nt, s + 100)
                d_ = {'caption': caps[s:e], 'bow_encoding': bow[s:e]}
                if self.with_bert:
                    d_['bert_encoding'] = feats[s:e]
                yield d_, list(range(s, e)), tuple(txt_ids[s:e])
    S1, t1, v1 = model.predict(Txt(False), Vis(), 'cosine')
    r1 = model.last_t2v_ranks.cpu().numpy()
    S2, t2, v2 = model.predict(Txt(True), Vis(), 'cosine')
    r2 = model.last_t2v_ranks.cpu().numpy()
    assert list(t1) == list(t2) == txt_ids and list(v1) == list(v2) == vis_ids
    assert np.array_equal(S1, S2) and np.array_equal(r1, r2)
    assert np.abs(S1).max() > 0 and len(set(r1.tolist())) > 4
