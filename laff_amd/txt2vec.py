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
(`W2Vec.ragged`), the soft assignment and the residual pooling run on the GPU (`laff_netvlad_encode`; with differentiable=True
in training `laff_netvlad_encode_train` and `laff_netvlad_backward`).

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

#: key of a caption dict under which data.PairProvider hands every encoder its batch input, prepared from the token ids it stored at
#: build: {encoder object: prepared input}.  An encoder whose object is in there uses that input and does no string work; without
#: the key (or without its own entry) it tokenises caption_feat_dict['caption'] as before.  The two ways give the same bits.
#:   BoWTxtEncoder      the batch CSR on the device (with `laff_csc` attached when the provider formed it)
#:   W2VTxtEncoder      the (B, ndims) mean-pooled matrix on the device
#:   GruTxtEncoder      a GruBatch / GruTrainBatch on the device (its own to_device of IdxVec.batch_ids)
#:   NetVLADTxtEncoder  the tuple its own to_device returns (W2Vec.ragged_rows)
PREPARED_KEY = 'laff_prepared'


def prepared_input(caption_feat_dict, encoder):
    """The prepared batch input of `encoder` in a caption dict, or None."""
    prepared = caption_feat_dict.get(PREPARED_KEY) if hasattr(caption_feat_dict, 'get') else None
    return None if prepared is None else prepared.get(encoder)


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
        return self.ragged_rows([self.raw_ids(c) for c in captions])

    @staticmethod
    def ragged_rows(rows):
        """ragged() from the captions' raw_ids results, e.g. ones kept from an earlier pass."""
        b = ragged_batch([r for r, _ in rows])
        return b.ids, b.row_off, np.array([0 if len(r) else n for r, n in rows], np.int32)

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
    Returns the bag-of-words matrix as CSR; TransformNet projects it with the gather-sum kernel.

    with_csc=True: the transposed pattern that the projection's backward reads (ops.csr_transpose) is formed on the host next to the
    CSR and travels as the attribute `laff_csc` of the returned tensor object: (colptr, rows, values) on the CSR's device.  A training
    step that hands this very object to TransformNet then needs no device sort.  The attribute belongs to the Python object: any op on
    the tensor (.to(), indexing, a collate) returns a tensor without it, and the backward transposes on the device instead."""

    def __init__(self, t2v_bow, device='cuda', with_csc=False):
        super().__init__()
        self.t2v_bow, self.device, self.with_csc = t2v_bow, device, with_csc

    def forward(self, caption_feat_dict, task3=False):
        x = prepared_input(caption_feat_dict, self)
        if x is not None:
            return {'text_features': x}
        if not self.with_csc:
            return {'text_features': self.t2v_bow.csr(caption_feat_dict['caption'], self.device)}
        from . import ops
        host = self.t2v_bow.csr(caption_feat_dict['caption'], 'cpu')
        x = host.to(self.device)
        x.laff_csc = tuple(t.to(self.device) for t in ops.csr_transpose(host))
        return {'text_features': x}


class W2VTxtEncoder(nn.Module):
    """Drop-in for model.model.W2VTxtEncoder (model/model.py:419-434)."""

    def __init__(self, t2v_w2v, device='cuda'):
        super().__init__()
        self.t2v_w2v, self.device = t2v_w2v, device

    def forward(self, caption_feat_dict, task3=False):
        x = prepared_input(caption_feat_dict, self)
        if x is not None:
            return {'text_features': x}
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


class _NetvladEncodeFn(torch.autograd.Function):
    """The saving forward (laff_netvlad_encode_train) with laff_netvlad_backward behind it.  Saves out, the reserve and the batch
    arrays; forms only the gradients that needs_input_grad asks for (the word2vec table gets none: the reference feeds its rows
    without a graph).  Once differentiable."""

    @staticmethod
    def forward(ctx, table, batch, fc1_weight, centroids):
        from . import ops
        out, reserve = ops.netvlad_encode_train(table, *batch, fc1_weight.detach(), centroids.detach())
        ctx.save_for_backward(out, reserve, table, fc1_weight, centroids)
        ctx.batch = batch
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from . import ops
        out, reserve, table, fc1_weight, centroids = ctx.saved_tensors
        want = (bool(ctx.needs_input_grad[2]), bool(ctx.needs_input_grad[3]))
        d_fc1, d_cent = ops.netvlad_backward(grad_out, out, reserve, table, *ctx.batch, fc1_weight.detach(), centroids.detach(),
                                             want=want)
        return None, None, d_fc1, d_cent


class NetVLADTxtEncoder(nn.Module):
    """Drop-in for model.model.NetVLADTxtEncoder (model/model.py:529-549):
    `txt_net.encoder.NetVLAD_encoder = NetVLADTxtEncoder(t2v_w2v, num_clusters, alpha)`, sharing the W2Vec (and its device table)
    with W2VTxtEncoder.  State-dict keys are the reference's (netvlad.fc1.weight, netvlad.centeroids), so its checkpoints load with
    strict=True.  Output: {'text_features': (N, K * D)}.  The kernel reads the parameters as they are, so every change of them
    (load_state_dict, copy_, a new Parameter) is seen by the next call.
    Training: with differentiable=True, .train() and enabled gradients, forward / encode_batch run the saving forward
    (laff_netvlad_encode_train, fp32; the same bits) under autograd, and its backward gives the gradients of netvlad.fc1.weight and
    netvlad.centeroids (laff_netvlad_backward).  The switch is explicit: without it .train() changes nothing."""

    def __init__(self, t2v_w2v, num_clusters=32, alpha=100, device='cuda', differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)
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
        if self.differentiable and self.training and torch.is_grad_enabled():
            return self._encode_train((ids, row_off, row_off_host, zero_rows))
        return ops.netvlad_encode(self.t2v_w2v.device_table(self.device), ids, row_off, row_off_host, zero_rows,
                                  v.fc1.weight.detach(), v.centeroids.detach(), out=out, workspace=workspace)

    def _encode_train(self, batch):
        v = self.netvlad
        for p_, nm in ((v.fc1.weight, 'netvlad.fc1.weight'), (v.centeroids, 'netvlad.centeroids')):
            if p_.dtype != torch.float32:
                raise TypeError('the differentiable NetVLAD encoder is fp32 only, %s is %s' % (nm, p_.dtype))
            if not p_.is_cuda:
                raise RuntimeError('the differentiable NetVLAD encoder runs on the device only, %s is a CPU tensor: laff_amd has no '
                                   'CPU path' % nm)
        return _NetvladEncodeFn.apply(self.t2v_w2v.device_table(self.device), batch, v.fc1.weight, v.centeroids)

    def forward(self, caption_feat_dict, task3=False):
        b = prepared_input(caption_feat_dict, self)
        if b is None:
            b = self.to_device(*self.t2v_w2v.ragged(caption_feat_dict['caption']))
        return {'text_features': self.encode_batch(*b)}


GruBatch = collections.namedtuple('GruBatch', ['tokens', 'lengths', 'perm', 'batch_sizes'])
GruBatch.__doc__ = """A batch of captions as the GRU step kernel takes it: rows sorted by length, longest first (stable).
tokens [T_max, N] int32 time-major in sorted order (0 = <pad> past a row's end), lengths [N] int32 sorted, perm [N] int32
(sorted row -> input position), batch_sizes: list of T_max ints, rows still active at step t (PackedSequence.batch_sizes)."""


GruTrainBatch = collections.namedtuple('GruTrainBatch', GruBatch._fields + ('pos', 'flat', 'seg_off', 'seg_tok', 'seg_pos'))
GruTrainBatch.__doc__ = """A GruBatch with what the differentiable encoder adds (GruTxtEncoder.to_device with differentiable=True), int32
device tensors: pos [T_max, N] the packed position off[t] + row of every active entry (off = prefix sum of batch_sizes, 0 elsewhere),
flat [M] the tokens in packed order, and the token segments of the embedding gradient: seg_tok [U] the distinct tokens in ascending
order, seg_off [U + 1], seg_pos [M] each token's packed positions in ascending order."""


def gru_train_arrays(tokens, batch_sizes):
    """The host arrays (pos, flat, seg_off, seg_tok, seg_pos) of a GruTrainBatch from GruBatch.tokens (numpy) and batch_sizes."""
    T, N = tokens.shape
    bs = np.asarray(batch_sizes, dtype=np.int64).reshape(T)
    off = np.concatenate([[0], np.cumsum(bs)]).astype(np.int64)
    active = np.arange(N)[None, :] < bs[:, None]
    pos = np.where(active, off[:T, None] + np.arange(N)[None, :], 0).astype(np.int32)
    flat = tokens[active].astype(np.int32)                    # row-major over (t, row): packed order
    order = np.argsort(flat, kind='stable').astype(np.int32)  # ascending token, ascending position inside a token
    seg_tok, counts = np.unique(flat, return_counts=True)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return pos, flat, seg_off, seg_tok.astype(np.int32), order


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
        return self.batch_ids([self.encoding(c) for c in captions])

    @staticmethod
    def batch_ids(ids):
        """batch() from the captions' encoding() arrays, e.g. ones kept from an earlier pass."""
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


class _GruEncodeFn(torch.autograd.Function):
    """The training encode (laff_gru_encode_train) with laff_gru_backward behind it.  Saves the reserve, X = we[tokens] and the batch
    arrays; forms only the gradients that needs_input_grad asks for.  Once differentiable."""

    @staticmethod
    def forward(ctx, enc, b, we, *rnn):
        from . import ops
        sfxs = ('_l0', '_l0_reverse') if enc.bigru else ('_l0',)
        par = {n + sfx: rnn[4 * d + k] for d, sfx in enumerate(sfxs) for k, n in enumerate(_GRU_PARAMS)}
        ndirs = 2 if enc.bigru and enc.pooling == 'mean' else 1       # bigru + last: the output is the forward half only
        x = ops.gru_gather_rows(we.detach(), b.flat)
        sets = []
        for sfx in sfxs[:ndirs]:
            gi = ops.fc_act_bn(x, par['weight_ih' + sfx].detach(), par['bias_ih' + sfx].detach())
            sets.append((gi, ops.gru_pack_whh(par['weight_hh' + sfx].detach()), par['bias_hh' + sfx].detach().contiguous()))
        out, reserve = ops.gru_encode_train(b.pos, b.lengths, b.perm, b.batch_sizes, sets[0], sets[1] if ndirs == 2 else None,
                                            enc.pooling)
        ctx.save_for_backward(reserve, x, we, *rnn)
        ctx.enc, ctx.batch, ctx.ndirs = enc, b, ndirs
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from . import ops
        reserve, x, we = ctx.saved_tensors[:3]
        rnn, enc, b, ndirs = ctx.saved_tensors[3:], ctx.enc, ctx.batch, ctx.ndirs
        need = ctx.needs_input_grad
        dirs = [(rnn[4 * d].detach(), ops.gru_pack_whh_t(rnn[4 * d + 1].detach())) for d in range(ndirs)]
        want = [[bool(need[3 + 4 * d + k]) for k in range(4)] for d in range(ndirs)]
        d_we, gf, gr = ops.gru_backward(grad_out, b.lengths, b.perm, b.batch_sizes, reserve, x, dirs[0], dirs[1] if ndirs == 2 else None,
                                        enc.pooling, segments=(b.seg_off, b.seg_tok, b.seg_pos) if need[2] else None,
                                        vocab=we.shape[0], want=(want[0], want[1] if ndirs == 2 else None))
        grads = list(gf) + (list(gr) if ndirs == 2 else [None] * (len(rnn) - 4))
        return (None, None, d_we) + tuple(grads)


_GRU_PARAMS = ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')


class GruTxtEncoder(nn.Module):
    """Drop-in for model.model.GruTxtEncoder / BiGruTxtEncoder (model/model.py:323-396), inference:
    `txt_net.encoder.rnn_encoder = GruTxtEncoder(IdxVec(vocab), we_dim, rnn_size, bidirectional, pooling)`.
    State-dict keys are the reference's (we.weight, rnn.weight_ih_l0, ...), so its checkpoints load with strict=True.
    Output: {'text_features': (N, H)} for gru mean / last and bigru last, (N, 2H) for gru mean_last and bigru mean, input order.
    P = we . W_ih^T + b_ih and the packed W_hh are cached and rebuilt whenever a parameter changes (load_state_dict, copy_, ...).
    Training: with differentiable=True, .train() and enabled gradients, forward runs the saving encode (laff_gru_encode_train, fp32,
    from the batch's own input table; the same bits) under autograd, and its backward gives the gradients of we.weight and every
    rnn.* parameter (laff_gru_backward).  The switch is explicit: without it .train() changes nothing."""

    def __init__(self, t2v_idx, we_dim, rnn_size, bidirectional=False, pooling='mean', rnn_layer=1, device='cuda', differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)
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
        if self.differentiable and self.training and torch.is_grad_enabled():
            return self._encode_train(b)
        sets = self._tables()
        rev = sets[1] if self.bigru and self.pooling == 'mean' else None
        return ops.gru_encode(b.tokens, b.lengths, b.perm, b.batch_sizes, sets[0], rev, self.pooling, out=out, workspace=workspace)

    def _encode_train(self, b):
        if not isinstance(b, GruTrainBatch):
            raise TypeError('the differentiable GruTxtEncoder takes a GruTrainBatch (to_device of a host GruBatch)')
        params = [self.we.weight] + [getattr(self.rnn, n + sfx) for sfx in (('_l0', '_l0_reverse') if self.bigru else ('_l0',))
                                     for n in _GRU_PARAMS]
        for p_, nm in zip(params, ['we.weight'] + [n for n, _ in self.rnn.named_parameters()]):
            if p_.dtype != torch.float32:
                raise TypeError('the differentiable GRU encoder is fp32 only, %s is %s' % (nm, p_.dtype))
            if not p_.is_cuda:
                raise RuntimeError('the differentiable GRU encoder runs on the device only, %s is a CPU tensor: laff_amd has no CPU path' % nm)
        return _GruEncodeFn.apply(self, b, *params)

    def to_device(self, b):
        dev = self.we.weight.device
        base = (torch.from_numpy(b.tokens).to(dev), torch.from_numpy(b.lengths).to(dev), torch.from_numpy(b.perm).to(dev),
                b.batch_sizes)
        if not self.differentiable:
            return GruBatch(*base)
        return GruTrainBatch(*base, *[torch.from_numpy(a).to(dev) for a in gru_train_arrays(b.tokens, b.batch_sizes)])

    def forward(self, caption_feat_dict, task3=False):
        b = prepared_input(caption_feat_dict, self)
        if b is None:
            b = self.to_device(self.t2v_idx.batch(caption_feat_dict['caption']))
        return {'text_features': self.encode_batch(b)}
