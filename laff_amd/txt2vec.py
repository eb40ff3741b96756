"""Text-side feature producers that are cheap on the device.

The reference turns every caption into a dense |vocab|-wide count vector on the host (`txt2vec.BowVec._encoding`,
/root/reference/txt2vec.py:56-63) and multiplies it with the FC weight as a dense GEMM (`BoWTxtEncoder`,
model/model.py:399-416), and averages word2vec rows fetched one BigFile read per caption (`W2Vec._encoding`,
txt2vec.py:97-104).  Here the host only tokenises (same rules: textlib.py:27-45) and maps words to ids; the arithmetic is a
gather-sum on the GPU (`laff_fc_gather_act_bn`): bow -> a CSR count matrix that goes straight into the TransformNet
(gather-sum of columns of W), w2v -> mean of table rows.

Stop words are DATA of the deployment (the reference ships `stopwords_en.txt`); pass them in (`stopwords=`), e.g.
`set(open('stopwords_en.txt').read().split())`.

The NetVLAD encoder (`NetVLADTxtEncoder`) shares the W2Vec object and its device table: the host maps captions to table rows
(`W2Vec.ragged`), the soft assignment and the residual pooling run on the GPU (`laff_netvlad_encode`).

The GRU encoder (`GruTxtEncoder`) keeps the same split: the host maps captions to token ids and lays the batch out the way the
step kernel walks it (`IdxVec.batch`); the recurrence runs on the GPU (`laff_gru_encode`).
"""
import collections
import pickle
import re

import numpy as np
import torch
import torch.nn as nn

from .ragged import _Weights, ragged_batch

_NON_ALNUM = re.compile(r"[^A-Za-z0-9]")


def tokenize(text, clean=True, remove_stopword=False, stopwords=()):
    """textlib.TextTool.tokenize(language='en') (textlib.py:27-45)."""
    sent = text
    if clean:
        sent = _NON_ALNUM.sub(' ', sent.replace('\r', ' ')).strip().lower()
    tokens = sent.split()
    if remove_stopword:
        tokens = [t for t in tokens if t not in stopwords]
    return tokens


class Vocabulary(object):
    """Same attributes as textlib.Vocabulary (textlib.py:69-102), so that the reference's vocab pickles load into it."""

    def __init__(self, encoding='bow'):
        self.word2idx, self.idx2word, self.encoding = {}, {}, encoding

    def add(self, word):
        if word not in self.word2idx:
            idx = len(self.word2idx)
            self.word2idx[word] = idx
            self.idx2word[idx] = word

    def find(self, word):
        return self.word2idx.get(word, -1)

    def __getitem__(self, index):
        return self.idx2word[index]

    def __call__(self, word):
        """textlib.Vocabulary.__call__ (textlib.py:102-109): a 'gru' vocabulary maps an unknown word to <unk>, others raise."""
        if word not in self.word2idx:
            if 'gru' in self.encoding:
                return self.word2idx['<unk>']
            raise KeyError('word out of vocab: %s' % word)
        return self.word2idx[word]

    def __len__(self):
        return len(self.word2idx)


class _VocabUnpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if name == 'Vocabulary':           # pickled as textlib.Vocabulary by the reference's build_vocab
            return Vocabulary
        return super().find_class(module, name)


def load_vocab(path):
    """A reference vocabulary pickle (`bow_nsw_5.pkl`, ...) without the reference's `textlib` module on the path."""
    with open(path, 'rb') as f:
        return _VocabUnpickler(f).load()


def _as_vocab(vocab):
    if isinstance(vocab, str):
        return load_vocab(vocab)
    if hasattr(vocab, 'find'):
        return vocab
    v = Vocabulary()
    for w in vocab:
        v.add(w)
    return v


def _csr(rows, ncols, device, dtype=torch.float32):
    """rows: list of (sorted unique column ids, values) -> torch CSR with int32 indices."""
    crow = np.zeros(len(rows) + 1, np.int32)
    crow[1:] = np.cumsum([len(c) for c, _ in rows])
    col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    val = np.concatenate([np.asarray(v, np.float32) for _, v in rows]) if rows else np.zeros(0, np.float32)
    return torch.sparse_csr_tensor(torch.from_numpy(crow).to(device), torch.from_numpy(col.astype(np.int32)).to(device),
                                   torch.from_numpy(val).to(device=device, dtype=dtype), size=(len(rows), ncols))


class BowVec(object):
    """txt2vec.BowVec (stopwords=None) / BowVecNSW (stopwords=set) with norm=0 (the only setting the path uses)."""

    def __init__(self, vocab, stopwords=None, clean=True):
        self.vocab = _as_vocab(vocab)
        self.ndims = len(self.vocab)
        self.stopwords = None if stopwords is None else frozenset(stopwords)
        self.clean = clean

    def __len__(self):
        return self.ndims

    def _ids(self, caption):
        words = tokenize(caption, self.clean, self.stopwords is not None, self.stopwords or ())
        counts = {}
        for w in words:
            i = self.vocab.find(w)
            if i >= 0:
                counts[i] = counts.get(i, 0) + 1
        ids = sorted(counts)
        return ids, [float(counts[i]) for i in ids]

    def encoding(self, caption):
        """Dense count vector (float64), as the reference returns."""
        vec = np.zeros(self.ndims)
        ids, cnt = self._ids(caption)
        vec[ids] = cnt
        return vec

    def csr(self, captions, device):
        """(B, ndims) count matrix in CSR: the input laff_fc_gather_act_bn takes."""
        return _csr([self._ids(c) for c in captions], self.ndims, device)


class W2Vec(object):
    """txt2vec.W2Vec / W2VecNSW: mean of the word2vec rows of the caption's distinct known words."""

    def __init__(self, words, table, stopwords=None, clean=True):
        """words: list of the table's row names; table: (V, ndims) float32 array/tensor (e.g. a BigFile's matrix)."""
        self.index = {w: i for i, w in enumerate(words)}
        self.table = torch.as_tensor(np.asarray(table) if not torch.is_tensor(table) else table, dtype=torch.float32).contiguous()
        self.ndims = int(self.table.shape[1])
        self.stopwords = None if stopwords is None else frozenset(stopwords)
        self.clean = clean
        self._dev = {}

    @classmethod
    def from_bigfile(cls, datadir, stopwords=None):
        from .bigfile import BigFile
        bf = BigFile(datadir)
        mat = np.fromfile(bf.binary_file, dtype=np.float32).reshape(bf.nr_of_images, bf.ndims)
        return cls(list(bf.names), mat, stopwords)

    def raw_ids(self, caption):
        """The row set of the reference's W2Vec.raw_encoding (txt2vec.py:106-114): (the distinct known words' table rows in row
        order, the number of tokens).  With no known word the reference returns that many zero rows instead."""
        words = tokenize(caption, self.clean, self.stopwords is not None, self.stopwords or ())
        return sorted({self.index[w] for w in words if w in self.index}), len(words)   # BigFile.read dedups, drops unknown names

    def _ids(self, caption):
        ids, _ = self.raw_ids(caption)
        return ids, [1.0 / max(1, len(ids))] * len(ids)

    def ragged(self, captions):
        """The captions as laff_netvlad_encode takes them: ids [R] int32 (raw_ids concatenated), row_off [N+1] int32 and zero_rows
        [N] int32 (the token count of a caption without known words, else 0)."""
        rows = [self.raw_ids(c) for c in captions]
        b = ragged_batch([r for r, _ in rows])
        return b.ids, b.row_off, np.array([0 if r else n for r, n in rows], np.int32)

    def encoding(self, caption):
        ids, _ = self._ids(caption)
        if not ids:
            return np.zeros(self.ndims)
        return self.table[ids].numpy().astype(np.float64).mean(axis=0)

    def csr(self, captions, device):
        return _csr([self._ids(c) for c in captions], len(self.index), device)

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.table.to(device)
        return self._dev[key]

    def encode(self, captions, device):
        """(B, ndims) mean-pooled word vectors, computed on the GPU as a gather-sum over the table."""
        from . import ops
        if self.ndims % 4:
            raise NotImplementedError('word-vector width must be a multiple of 4 (got %d)' % self.ndims)
        return ops.fc_gather_act_bn(self.csr(captions, device), self.device_table(device))


class BoWTxtEncoder(nn.Module):
    """Drop-in for model.model.BoWTxtEncoder (model/model.py:399-416): `txt_net.encoder.bow_encoder = BoWTxtEncoder(t2v)`.
    Returns the bag-of-words matrix as CSR; TransformNet projects it with the gather-sum kernel."""

    def __init__(self, t2v_bow, device='cuda'):
        super().__init__()
        self.t2v_bow, self.device = t2v_bow, device

    def forward(self, caption_feat_dict, task3=False):
        return {'text_features': self.t2v_bow.csr(caption_feat_dict['caption'], self.device)}


class W2VTxtEncoder(nn.Module):
    """Drop-in for model.model.W2VTxtEncoder (model/model.py:419-434)."""

    def __init__(self, t2v_w2v, device='cuda'):
        super().__init__()
        self.t2v_w2v, self.device = t2v_w2v, device

    def forward(self, caption_feat_dict, task3=False):
        return {'text_features': self.t2v_w2v.encode(caption_feat_dict['caption'], self.device)}


class _NetVLAD(nn.Module):
    """The parameters of model/Attention.py:862-884 NetVLAD under its names (fc1.weight [K, D], no bias; centeroids [K, D]) and its
    initialisation.  alpha is kept as the reference keeps it: its forward does not use it."""

    def __init__(self, feature_dim, num_clusters=32, alpha=100):
        super().__init__()
        self.num_clusters, self.dim, self.alpha = int(num_clusters), int(feature_dim), alpha
        init_sc = 1.0 / np.sqrt(feature_dim)
        self.fc1 = nn.Linear(self.dim, self.num_clusters, bias=False)
        self.centeroids = nn.Parameter(init_sc * torch.randn(self.num_clusters, self.dim))
        self.fc1.weight = nn.Parameter(init_sc * torch.randn(self.num_clusters, self.dim))


class NetVLADTxtEncoder(nn.Module):
    """Drop-in for model.model.NetVLADTxtEncoder (model/model.py:529-549), inference:
    `txt_net.encoder.NetVLAD_encoder = NetVLADTxtEncoder(t2v_w2v, num_clusters, alpha)`, sharing the W2Vec (and its device table)
    with W2VTxtEncoder.  State-dict keys are the reference's (netvlad.fc1.weight, netvlad.centeroids), so its checkpoints load with
    strict=True.  Output: {'text_features': (N, K * D)}.  The kernel reads the parameters as they are, so every change of them
    (load_state_dict, copy_, a new Parameter) is seen by the next call."""

    def __init__(self, t2v_w2v, num_clusters=32, alpha=100, device='cuda'):
        super().__init__()
        K, D = int(num_clusters), int(t2v_w2v.ndims)
        if not 1 <= K <= 64:
            raise NotImplementedError('NetVLADTxtEncoder: num_clusters=%d; the kernel takes 1 to 64 clusters' % K)
        if D % 4 or not 4 <= D <= 1024:
            raise NotImplementedError('NetVLADTxtEncoder: word-vector width %d; the kernel takes multiples of 4 up to 1024' % D)
        self.t2v_w2v, self.device = t2v_w2v, device
        self.netvlad = _NetVLAD(D, K, alpha).to(device)

    def to_device(self, ids, row_off, zero_rows):
        dev = self.netvlad.centeroids.device
        return (torch.from_numpy(ids).to(dev), torch.from_numpy(row_off).to(dev), row_off, torch.from_numpy(zero_rows).to(dev))

    def encode_batch(self, ids, row_off, row_off_host, zero_rows, out=None, workspace=None):
        """The device half of forward(): W2Vec.ragged's arrays, ids / row_off / zero_rows already on the device."""
        from . import ops
        v = self.netvlad
        return ops.netvlad_encode(self.t2v_w2v.device_table(self.device), ids, row_off, row_off_host, zero_rows,
                                  v.fc1.weight.detach(), v.centeroids.detach(), out=out, workspace=workspace)

    def forward(self, caption_feat_dict, task3=False):
        b = self.to_device(*self.t2v_w2v.ragged(caption_feat_dict['caption']))
        return {'text_features': self.encode_batch(*b)}


GruBatch = collections.namedtuple('GruBatch', ['tokens', 'lengths', 'perm', 'batch_sizes'])
GruBatch.__doc__ = """A batch of captions as the GRU step kernel takes it: rows sorted by length, longest first (stable).
tokens [T_max, N] int32 time-major in sorted order (0 = <pad> past a row's end), lengths [N] int32 sorted, perm [N] int32
(sorted row -> input position), batch_sizes: list of T_max ints, rows still active at step t (PackedSequence.batch_sizes)."""


class IdxVec(object):
    """txt2vec.IndexVec (txt2vec.py:117-131): '<start>' + tokenize(caption) + '<end>' mapped through a 'gru' vocabulary."""

    def __init__(self, vocab, clean=True):
        self.vocab = load_vocab(vocab) if isinstance(vocab, str) else vocab
        self.ndims = len(self.vocab)
        self.clean = clean

    def __len__(self):
        return self.ndims

    def encoding(self, caption):
        words = ['<start>'] + tokenize(caption, self.clean, False) + ['<end>']
        return np.array([self.vocab(w) for w in words])

    def batch(self, captions):
        ids = [self.encoding(c) for c in captions]
        lens = np.array([len(v) for v in ids], dtype=np.int64)
        perm = np.argsort(-lens, kind='stable').astype(np.int32)
        T = int(lens.max()) if len(ids) else 0
        tokens = np.zeros((T, len(ids)), dtype=np.int32)
        for j, i in enumerate(perm):
            tokens[:lens[i], j] = ids[i]
        slens = lens[perm].astype(np.int32)
        batch_sizes = [int((slens > t).sum()) for t in range(T)]
        return GruBatch(tokens, slens, perm, batch_sizes)


class _GruWeights(nn.Module):
    """The parameters of one torch.nn.GRU layer under nn.GRU's own names, held as plain parameters: no nn.GRU object (its .to()
    may call into MIOpen) and no torch RNN call anywhere on the path."""

    def __init__(self, input_size, hidden_size, bidirectional):
        super().__init__()
        k = 1.0 / hidden_size ** 0.5
        for sfx in ('_l0', '_l0_reverse') if bidirectional else ('_l0',):
            for name, shape in (('weight_ih', (3 * hidden_size, input_size)), ('weight_hh', (3 * hidden_size, hidden_size)),
                                ('bias_ih', (3 * hidden_size,)), ('bias_hh', (3 * hidden_size,))):
                self.register_parameter(name + sfx, nn.Parameter(torch.empty(shape).uniform_(-k, k)))   # nn.GRU's init


class GruTxtEncoder(nn.Module):
    """Drop-in for model.model.GruTxtEncoder / BiGruTxtEncoder (model/model.py:323-396), inference:
    `txt_net.encoder.rnn_encoder = GruTxtEncoder(IdxVec(vocab), we_dim, rnn_size, bidirectional, pooling)`.
    State-dict keys are the reference's (we.weight, rnn.weight_ih_l0, ...), so its checkpoints load with strict=True.
    Output: {'text_features': (N, H)} for gru mean / last and bigru last, (N, 2H) for gru mean_last and bigru mean, input order.
    P = we . W_ih^T + b_ih and the packed W_hh are cached and rebuilt whenever a parameter changes (load_state_dict, copy_, ...)."""

    def __init__(self, t2v_idx, we_dim, rnn_size, bidirectional=False, pooling='mean', rnn_layer=1, device='cuda'):
        super().__init__()
        if int(rnn_layer) != 1:
            raise NotImplementedError('GruTxtEncoder: rnn_layer=%d; only rnn_layer = 1 is supported' % rnn_layer)
        if pooling not in ('mean', 'last', 'mean_last'):
            raise ValueError("GruTxtEncoder: pooling must be 'mean', 'last' or 'mean_last', got %r" % (pooling,))
        if bidirectional and pooling == 'mean_last':
            raise NotImplementedError('GruTxtEncoder: bigru_mean_last is not supported (the reference fails on it as well)')
        H = int(rnn_size)
        if H % 32 or not 32 <= H <= 2048:
            raise NotImplementedError('GruTxtEncoder: rnn_size=%d; the kernel takes multiples of 32 up to 2048' % H)
        self.t2v_idx, self.device = t2v_idx, device
        self.rnn_size, self.bigru, self.pooling = H, bool(bidirectional), pooling
        self.we = nn.Embedding(len(t2v_idx.vocab), int(we_dim))
        self.rnn = _GruWeights(int(we_dim), H, self.bigru)
        self.to(device)
        self._weights = _Weights(self, None)

    def _tables(self):
        """(P, packed W_hh, b_hh) per direction, rebuilt when any parameter has changed since the last build."""
        from . import ops

        def build(_):
            r, sets = self.rnn, []
            for sfx in ('_l0', '_l0_reverse') if self.bigru else ('_l0',):
                w_ih, w_hh = getattr(r, 'weight_ih' + sfx), getattr(r, 'weight_hh' + sfx)
                P = ops.fc_act_bn(self.we.weight.detach(), w_ih.detach(), getattr(r, 'bias_ih' + sfx).detach())
                sets.append((P, ops.gru_pack_whh(w_hh.detach()), getattr(r, 'bias_hh' + sfx).detach().contiguous()))
            return sets
        return self._weights.get(build)

    def encode_batch(self, b, out=None, workspace=None):
        """The device half of forward(): a GruBatch (IdxVec.batch) whose arrays are already device tensors."""
        from . import ops
        sets = self._tables()
        rev = sets[1] if self.bigru and self.pooling == 'mean' else None
        return ops.gru_encode(b.tokens, b.lengths, b.perm, b.batch_sizes, sets[0], rev, self.pooling, out=out, workspace=workspace)

    def to_device(self, b):
        dev = self.we.weight.device
        return GruBatch(torch.from_numpy(b.tokens).to(dev), torch.from_numpy(b.lengths).to(dev), torch.from_numpy(b.perm).to(dev),
                        b.batch_sizes)

    def forward(self, caption_feat_dict, task3=False):
        b = self.t2v_idx.batch(caption_feat_dict['caption'])
        return {'text_features': self.encode_batch(self.to_device(b))}
