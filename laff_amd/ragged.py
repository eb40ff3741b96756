"""What the encoders of ragged batches share on the host: the batch layout (`RaggedBatch`, `ragged_batch`), the budgeted chunker
(`_chunks`), the cache of packed weights (`_Weights`) and the base class of the two transformer text encoders (`_TextEncoder`).
Ragged: the items of a batch (a caption's token rows, a video's frames) are concatenated without padding; item i is rows
row_off[i] .. row_off[i+1] - 1 of row_off [N+1] int32, which the entry points take on the device and on the host (laff_amd/ops.py).
This module imports no encoder; the encoders import it."""
import collections

import numpy as np
import torch
import torch.nn as nn

RaggedBatch = collections.namedtuple('RaggedBatch', ['ids', 'row_off', 'row_off_host'])
RaggedBatch.__doc__ = """Captions as laff_clip_encode / laff_bert_encode take them: ids [R] int32 (each caption's token ids, the captions
concatenated), row_off [N+1] int32 (caption i is rows row_off[i] .. row_off[i+1] - 1), row_off_host: the same offsets on the host.
ids / row_off are numpy arrays from a tokenizer's batch() and device tensors after an encoder's to_device()."""


def ragged_batch(rows):
    """A list of id lists -> a RaggedBatch of numpy int32 arrays (an empty list: no ids, row_off = [0]; a row may be empty)."""
    row_off = np.zeros(len(rows) + 1, dtype=np.int32)
    row_off[1:] = np.cumsum([len(r) for r in rows])
    ids = np.fromiter((i for r in rows for i in r), np.int32, int(row_off[-1]))
    return RaggedBatch(ids, row_off, row_off)


def _chunks(off, budget, workspace_bytes, device):
    """The calls of a budgeted encode: (i0, i1, ws) for the consecutive items i0 .. i1 - 1 whose offsets off[i0] .. off[i1] span at
    most budget (one item at least, so a longer item gets a call of its own), with a uint8 workspace of at least
    workspace_bytes(i0, i1) bytes on the device, grown as needed."""
    n, i0, ws = len(off) - 1, 0, None
    while i0 < n:
        i1 = int(np.searchsorted(off, off[i0] + budget, side='right')) - 1     # the items that end within the budget
        i1 = min(max(i1, i0 + 1), n)
        need = workspace_bytes(i0, i1)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
        yield i0, i1, ws
        i0 = i1


class _Weights(object):
    """The device copies of a tower's parameters that its laff_* model struct points at, kept alive with it: f32 / packed return the
    pointer of an fp32 / packed copy of a parameter, blocks the laff_clip_block array of a resblocks module.  get(build) returns the
    struct build(self) makes, rebuilt whenever a parameter of `module` has changed since the last build (load_state_dict, copy_, ...)."""

    def __init__(self, module, precision):
        self.module, self.precision = module, precision
        self._key, self._model, self._keep = None, None, []

    def get(self, build):
        key = tuple((p.data_ptr(), p._version, p.device) for p in self.module.parameters())
        if key != self._key:
            self._keep = []
            with torch.no_grad():
                self._model = build(self)
            self._key = key
        return self._model

    def f32(self, t):
        t = t.detach().float().contiguous()
        self._keep.append(t)
        return t.data_ptr()

    def packed(self, t, transpose=False, padded_cols=None):
        from . import ops
        p = ops.clip_pack_weight(t.detach().float(), self.precision, transpose, padded_cols)
        self._keep.append(p)
        return p.data_ptr()

    def blocks(self, resblocks):
        from . import _lib
        f32, packed = self.f32, self.packed
        blocks = (_lib.ClipBlock * len(resblocks))()
        for i, b in enumerate(resblocks):
            blocks[i] = _lib.ClipBlock(f32(b.ln_1.weight), f32(b.ln_1.bias), packed(b.attn.in_proj_weight), f32(b.attn.in_proj_bias),
                                       packed(b.attn.out_proj.weight), f32(b.attn.out_proj.bias), f32(b.ln_2.weight), f32(b.ln_2.bias),
                                       packed(b.mlp.c_fc.weight), f32(b.mlp.c_fc.bias), packed(b.mlp.c_proj.weight), f32(b.mlp.c_proj.bias))
        self._keep.append(blocks)
        return blocks


class _TextEncoder(nn.Module):
    """The host side ClipTxtEncoder and BertTxtEncoder share.  A subclass sets feature_key (the pre-extracted feature forward() passes
    through), out_width (the feature width), max_len (the rows a caption has at most), vocab_size and max_rows, and defines
    _tokenize(captions) -> RaggedBatch, workspace_bytes(b), encode_batch(b, out, workspace) and _model().  Registers nothing."""

    feature_key = None

    def batch(self, captions):
        """The tokenizer's ragged batch at this encoder's length limit, with the ids checked against its vocabulary."""
        b = self._tokenize(captions)
        if b.ids.size and (int(b.ids.max()) >= self.vocab_size or int(b.ids.min()) < 0):
            raise ValueError('token id %d outside the vocabulary of %d' % (int(b.ids.max()), self.vocab_size))
        return b

    def to_device(self, b):
        dev = next(self.parameters()).device
        return RaggedBatch(torch.from_numpy(b.ids).to(dev), torch.from_numpy(b.row_off).to(dev), b.row_off_host)

    def encode(self, captions, max_rows=None):
        """Caption strings -> (N, out_width), in calls of at most max_rows token rows (one caption never spans two calls)."""
        b = self.batch(captions)
        dev = next(self.parameters()).device
        N, roh = len(captions), b.row_off_host
        out = torch.empty((N, self.out_width), device=dev, dtype=torch.float32)
        if N == 0:
            return out
        budget = max(int(max_rows or self.max_rows), self.max_len)
        ids, ro = torch.from_numpy(b.ids).to(dev), torch.from_numpy(roh).to(dev)
        for c0, c1, ws in _chunks(roh, budget, lambda c0, c1: self.workspace_bytes(RaggedBatch(None, None, roh[c0:c1 + 1] - roh[c0])), dev):
            r0, r1 = int(roh[c0]), int(roh[c1])
            self.encode_batch(RaggedBatch(ids[r0:r1], ro[c0:c1 + 1] - r0, roh[c0:c1 + 1] - r0), out=out[c0:c1], workspace=ws)
        return out

    def forward(self, caption_feat_dict, task3=False):
        if self.feature_key in caption_feat_dict:
            return {'text_features': caption_feat_dict[self.feature_key]}
        return {'text_features': self.encode(caption_feat_dict['caption'])}
