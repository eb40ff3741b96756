"""The GRU caption encoder's host side, without a GPU: caption -> token ids (txt2vec.IndexVec semantics), the length-sorted batch
layout the step kernel walks, the float64 restatement against the reference's outputs, and the C entry points' argument checks."""
import ctypes as C
import json
import pickle
import sys
import types

import numpy as np
import pytest

from gru_ref import gru_features
from laff_amd import txt2vec as T


def fixture_vocab(golden):
    z = golden('gru_encoder')
    v = T.Vocabulary('gru')
    for w in z.json('vocab'):
        v.add(w)
    return z, v


def fixture_sd(z, net):
    return z.sub(net + '/sd/')


def test_idxvec_encoding_equals_the_reference_ids(golden):
    z, v = fixture_vocab(golden)
    iv = T.IdxVec(v)
    caps, want = z.json('captions'), z.json('ids')
    assert len(caps) == len(want) >= 40
    for c, w in zip(caps, want):
        got = iv.encoding(c)
        assert got.tolist() == w, c
    assert iv.encoding('').tolist() == [1, 2]                      # <start> <end>
    assert max(len(w) for w in want) > 100


def test_batch_layout_is_a_stable_length_sort(golden):
    z, v = fixture_vocab(golden)
    caps, ids = z.json('captions'), z.json('ids')
    b = T.IdxVec(v).batch(caps)
    N = len(caps)
    lens = np.array([len(w) for w in ids])
    assert sorted(b.perm.tolist()) == list(range(N)) and b.perm.dtype == np.int32
    assert np.array_equal(b.lengths, lens[b.perm]) and np.all(np.diff(b.lengths) <= 0)
    for j in range(N - 1):                                         # stable: equal lengths keep their input order
        if b.lengths[j] == b.lengths[j + 1]:
            assert b.perm[j] < b.perm[j + 1]
    assert b.tokens.dtype == np.int32 and b.tokens.shape == (lens.max(), N)
    for j, i in enumerate(b.perm):
        assert b.tokens[:lens[i], j].tolist() == ids[i] and not b.tokens[lens[i]:, j].any()
    assert b.batch_sizes == [int((lens > t).sum()) for t in range(lens.max())]
    assert b.batch_sizes[0] == N and b.batch_sizes[-1] >= 1


def test_batch_sizes_match_torch_packed_sequence(golden):
    import torch
    from torch.nn.utils.rnn import pack_sequence
    z, v = fixture_vocab(golden)
    b = T.IdxVec(v).batch(z.json('captions'))
    packed = pack_sequence([torch.from_numpy(np.array(w)) for w in z.json('ids')], enforce_sorted=False)
    assert packed.batch_sizes.tolist() == b.batch_sizes


@pytest.mark.parametrize('net,pooling', [('gru', 'mean'), ('gru', 'last'), ('gru', 'mean_last'), ('bigru', 'mean'), ('bigru', 'last')])
def test_float64_restatement_reproduces_the_reference(golden, net, pooling):
    z = golden('gru_encoder')
    ids = [np.array(w) for w in z.json('ids')]
    got = gru_features(ids, fixture_sd(z, net), pooling, net == 'bigru')
    want = z['%s_%s' % (net, pooling)]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-6


def test_vocab_call_semantics():
    v = T.Vocabulary('gru')
    for w in ('<pad>', '<start>', '<end>', '<unk>', 'dog'):
        v.add(w)
    assert v('dog') == 4 and v('zebra') == 3
    b = T.Vocabulary('bow')
    b.add('dog')
    assert b('dog') == 0
    with pytest.raises(KeyError):
        b('zebra')


def test_gru_vocab_pickle_loads_through_load_vocab(tmp_path):
    """A gru_5.pkl as the reference's build_vocab writes it (a pickled textlib.Vocabulary)."""
    mod = types.ModuleType('textlib')

    class Vocabulary(object):
        def __init__(self, encoding):
            self.word2idx, self.idx2word, self.encoding = {}, {}, encoding

        def add(self, word):
            if word not in self.word2idx:
                self.word2idx[word] = len(self.word2idx)
                self.idx2word[self.word2idx[word]] = word
    Vocabulary.__module__, Vocabulary.__qualname__ = 'textlib', 'Vocabulary'
    mod.Vocabulary = Vocabulary
    sys.modules['textlib'] = mod
    try:
        src = Vocabulary('gru')
        for w in ('<pad>', '<start>', '<end>', '<unk>', 'a', 'dog'):
            src.add(w)
        path = tmp_path / 'gru_5.pkl'
        with open(path, 'wb') as f:
            pickle.dump(src, f)
    finally:
        del sys.modules['textlib']
    v = T.load_vocab(str(path))
    assert isinstance(v, T.Vocabulary) and len(v) == 6
    assert v('dog') == 5 and v('zebra') == 3
    iv = T.IdxVec(str(path))
    assert iv.encoding('A dog, a zebra').tolist() == [1, 4, 5, 4, 3, 2]


def test_encoder_refuses_unsupported_configurations():
    v = T.Vocabulary('gru')
    for w in ('<pad>', '<start>', '<end>', '<unk>'):
        v.add(w)
    with pytest.raises(NotImplementedError, match='rnn_layer'):
        T.GruTxtEncoder(T.IdxVec(v), 8, 64, rnn_layer=2, device='cpu')
    with pytest.raises(NotImplementedError, match='mean_last'):
        T.GruTxtEncoder(T.IdxVec(v), 8, 64, bidirectional=True, pooling='mean_last', device='cpu')
    with pytest.raises(NotImplementedError, match='32'):
        T.GruTxtEncoder(T.IdxVec(v), 8, 48, device='cpu')


def test_encoder_state_dict_uses_the_reference_names(golden):
    z, v = fixture_vocab(golden)
    for net in ('gru', 'bigru'):
        enc = T.GruTxtEncoder(T.IdxVec(v), 50, 64, bidirectional=net == 'bigru', device='cpu')
        import torch
        sd = {k: torch.from_numpy(a) for k, a in fixture_sd(z, net).items()}
        res = enc.load_state_dict(sd, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert not any(isinstance(m, torch.nn.RNNBase) for m in enc.modules())


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.laff_gru_workspace_bytes(100, 1024, 1, 0, 0, C.byref(n)) == 0 and n.value == 3 * 128 * 1024 * 4
    assert lib.laff_gru_workspace_bytes(100, 1024, 1, 1, 0, C.byref(n)) == 0 and n.value == 2 * 3 * 128 * 1024 * 4
    assert lib.laff_gru_workspace_bytes(100, 1024, 1, 1, 1, C.byref(n)) == 0 and n.value == 3 * 128 * 1024 * 4
    for H in (48, 4096, 16, 0):
        assert lib.laff_gru_workspace_bytes(10, H, 1, 0, 0, C.byref(n)) == -2
        assert b'H=%d' % H in lib.laff_last_error()
    assert lib.laff_gru_workspace_bytes(10, 64, 2, 0, 0, C.byref(n)) == -5 and b'num_layers=2' in lib.laff_last_error()
    assert lib.laff_gru_workspace_bytes(10, 64, 1, 1, 2, C.byref(n)) == -5 and b'mean_last' in lib.laff_last_error()
    assert lib.laff_gru_workspace_bytes(10, 64, 1, 0, 7, C.byref(n)) == -1
    assert lib.laff_gru_workspace_bytes(10, 64, 1, 0, 0, None) == -1
    fake = C.c_void_p(4096)                                        # never dereferenced: every call below fails its checks first
    bs = (C.c_int * 3)(4, 4, 2)

    def enc(H=64, layers=1, bidir=0, pooling=0, tokens=fake, bsz=bs, T_=3, N=4, ws_bytes=1 << 20, ldo=64):
        return lib.laff_gru_encode(None, tokens, fake, fake, bsz, T_, N, 10, H, layers, bidir, pooling, fake, fake, fake,
                                   fake, fake, fake, fake, ldo, fake, ws_bytes)
    assert enc(H=48) == -2 and b'H=48' in lib.laff_last_error()
    assert enc(H=4096) == -2 and b'H=4096' in lib.laff_last_error()
    assert enc(layers=2) == -5 and b'num_layers=2' in lib.laff_last_error()
    assert enc(bidir=1, pooling=2) == -5
    assert enc(tokens=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(bsz=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(bsz=(C.c_int * 3)(4, 2, 3)) == -1 and b'non-increasing' in lib.laff_last_error()
    assert enc(bsz=(C.c_int * 3)(3, 3, 2)) == -1 and b'batch_sizes[0]' in lib.laff_last_error()
    assert enc(ws_bytes=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert enc(ldo=32) == -2 and b'ldo' in lib.laff_last_error()
    assert enc(bidir=1, ldo=64) == -2                              # bigru mean is 2H wide
    assert enc() == -1 and b'null ctx' in lib.laff_last_error()   # valid arguments: only then the ctx
    assert enc(N=0) == 0                                           # the empty problem
    assert lib.laff_gru_pack_whh(None, fake, 48, fake) == -2
    assert lib.laff_gru_pack_whh(None, None, 64, fake) == -1
    assert lib.laff_gru_pack_whh(None, fake, 64, fake) == -1 and b'null ctx' in lib.laff_last_error()
