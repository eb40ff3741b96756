"""The CLIP text encoder on the device: caption strings -> CLIP_encoding, a drop-in for the text half of the reference's
`CLIPEncoder` (model/model.py:469-527) over `clip.model.CLIP.encode_text` (model/clip/model.py:153-206, 245-358).

The host tokenises (`ClipTokenizer`: the rules of clip's SimpleTokenizer + clip.tokenize) and lays the batch out ragged
(`ClipTokenizer.batch`); the transformer runs on the GPU (`laff_clip_encode`, laff_amd/csrc/clip.hip).

Ragged layout.  The reference runs all context_length positions of every caption and pools row p_i = argmax(ids_i) (the first
occurrence of the largest id: <|endoftext|>, or the largest id of a caption cut at the context length).  The attention mask is causal,
so no position after p_i reaches row p_i: caption i contributes only its first p_i + 1 rows.  That is exact, not an approximation.

The merges file (`bpe_simple_vocab_16e6.txt.gz` of a CLIP install) is an input of the deployment: pass its path.

Two documented approximations of the host side, both exact in the cases stated:
  * `ftfy.fix_text` is applied when ftfy is importable, otherwise the identity: exact for text that ftfy leaves alone.
  * the split pattern uses the `regex` module (\\p{L}, \\p{N}); without it a stdlib pattern is used that is exact for ASCII text.
"""
import gzip
import html

import numpy as np
import torch
import torch.nn as nn

from .ragged import RaggedBatch as ClipBatch, _TextEncoder, _Weights, _chunks, ragged_batch   # noqa: F401 (_chunks: re-export)

try:
    import ftfy
    _fix_text = ftfy.fix_text
except ImportError:                                       # exact for text ftfy would leave alone
    def _fix_text(text):
        return text

try:
    import regex as _re
    _PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""
except ImportError:
    import re as _re
    _PATTERN = None
# stdlib form, exact for ASCII: letters = \w minus digits and '_'; a digit; a run of what is neither space, letter nor digit
_STDLIB_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[^\W\d_]+|\d|(?:[^\s\w]|_)+"""

SOT, EOT = '<|startoftext|>', '<|endoftext|>'
N_MERGES = 49152 - 256 - 2                                 # the merges the CLIP vocabulary uses (lines 1 .. 48894 of the file)


def byte_symbols():
    """The 256 byte -> printable symbol table of GPT-2 / CLIP BPE: printable Latin-1 bytes map to themselves, the others to
    chr(256 + n) in byte order."""
    keep = set(range(ord('!'), ord('~') + 1)) | set(range(ord('¡'), ord('¬') + 1)) | set(range(ord('®'), ord('ÿ') + 1))
    table, n = {}, 0
    for b in sorted(keep):
        table[b] = chr(b)
    for b in range(256):
        if b not in keep:
            table[b] = chr(256 + n)
            n += 1
    return table


class ClipTokenizer(object):
    """clip.simple_tokenizer.SimpleTokenizer + clip.tokenize (model/clip/simple_tokenizer.py, model/clip/clip.py:162-192):
    clean (ftfy, html.unescape twice, strip), collapse whitespace, lower-case, split, byte-level BPE, <|startoftext|> ... <|endoftext|>,
    cut to context_length without keeping <|endoftext|>.  bpe_path: the CLIP merges file (gzip).  use_regex=False forces the stdlib
    split pattern (exact for ASCII)."""

    def __init__(self, bpe_path, use_regex=True):
        self.bytes = byte_symbols()
        with gzip.open(bpe_path) as f:
            lines = f.read().decode('utf-8').split('\n')
        merges = [tuple(m.split()) for m in lines[1:N_MERGES + 1]]
        symbols = list(self.bytes.values())               # printable bytes first, then the remapped ones, each in byte order
        vocab = symbols + [s + '</w>' for s in symbols] + [a + b for a, b in merges] + [SOT, EOT]
        self.encoder = {}
        for i, tok in enumerate(vocab):
            self.encoder[tok] = i
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]
        self.vocab_size = len(vocab)
        self._cache = {SOT: [SOT], EOT: [EOT]}
        if use_regex and _PATTERN is not None:
            self._re, self._split = _re, _re.compile(_PATTERN, _re.IGNORECASE)
        else:
            import re
            self._re, self._split = re, re.compile(_STDLIB_PATTERN, re.IGNORECASE)

    def _bpe(self, token):
        """Merge the adjacent pair of lowest rank, all its occurrences left to right, until no ranked pair is left."""
        word = self._cache.get(token)
        if word is not None:
            return word
        word = list(token[:-1]) + [token[-1] + '</w>']
        while len(word) > 1:
            best = min(zip(word, word[1:]), key=lambda p: self.ranks.get(p, N_MERGES))
            if best not in self.ranks:
                break
            a, b = best
            out, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    out.append(a + b)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = out
        self._cache[token] = word
        return word

    def clean(self, text):
        text = html.unescape(html.unescape(_fix_text(text))).strip()
        return self._re.sub(r'\s+', ' ', text).strip().lower()

    def encode(self, text):
        """The BPE ids of one caption (without <|startoftext|> / <|endoftext|>)."""
        ids = []
        for piece in self._split.findall(self.clean(text)):
            sym = ''.join(self.bytes[b] for b in piece.encode('utf-8'))
            ids.extend(self.encoder[t] for t in self._bpe(sym))
        return ids

    def tokens(self, text, context_length=77):
        """clip.tokenize's row of one caption, without the zero padding."""
        return ([self.sot] + self.encode(text) + [self.eot])[:context_length]

    def tokenize(self, texts, context_length=77):
        """clip.tokenize: [N, context_length] int64, zero-padded."""
        if isinstance(texts, str):
            texts = [texts]
        out = np.zeros((len(texts), context_length), dtype=np.int64)
        for i, t in enumerate(texts):
            ids = self.tokens(t, context_length)
            out[i, :len(ids)] = ids
        return out

    def batch(self, texts, context_length=77):
        """The ragged batch: caption i keeps its rows 0 .. p_i, p_i = argmax of its ids (first occurrence)."""
        rows = []
        for t in texts:
            ids = self.tokens(t, context_length)
            rows.append(ids[:int(np.argmax(ids)) + 1])
        return ragged_batch(rows)


class _Attn(nn.Module):
    """nn.MultiheadAttention's parameters under its own names, as plain parameters (no torch attention call on the path)."""

    def __init__(self, width):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)


class _Block(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.attn = _Attn(width)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Module()
        self.mlp.c_fc = nn.Linear(width, 4 * width)
        self.mlp.c_proj = nn.Linear(4 * width, width)
        self.ln_2 = nn.LayerNorm(width)


def _init_blocks(resblocks, width, layers):
    """CLIP.initialize_parameters' scales for the residual blocks."""
    proj_std, attn_std, fc_std = width ** -0.5 * (2 * layers) ** -0.5, width ** -0.5, (2 * width) ** -0.5
    for b in resblocks:
        nn.init.normal_(b.attn.in_proj_weight, std=attn_std)
        nn.init.normal_(b.attn.out_proj.weight, std=proj_std)
        nn.init.normal_(b.mlp.c_fc.weight, std=fc_std)
        nn.init.normal_(b.mlp.c_proj.weight, std=proj_std)


def _check_dims(name, precision, width, heads, layers):
    """The constructor refusals both encoders share; name: the class, for the message."""
    if precision not in ('fp16', 'fp32'):
        raise NotImplementedError("%s: precision %r; 'fp16' or 'fp32'" % (name, precision))
    if width % 64 or not 64 <= width <= 1024:
        raise NotImplementedError('%s: width=%d; the kernels take multiples of 64 up to 1024' % (name, width))
    if heads * 64 != width:
        raise NotImplementedError('%s: width=%d heads=%d; only a head dim of 64 is supported' % (name, width, heads))
    if layers < 1:
        raise NotImplementedError('%s: layers=%d; at least one block' % (name, layers))


class _ClipText(nn.Module):
    """The text parameters of clip.model.CLIP under their names there."""

    def __init__(self, width, layers, embed_dim, context_length, vocab_size):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.Sequential(*[_Block(width) for _ in range(layers)])
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        # CLIP.initialize_parameters' scales, so that an encoder that is never loaded still computes something sensible
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        _init_blocks(self.transformer.resblocks, width, layers)
        nn.init.normal_(self.text_projection, std=width ** -0.5)


_IGNORED = ('visual.', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')


class ClipTxtEncoder(_TextEncoder):
    """Drop-in for the text half of model.model.CLIPEncoder (frozen, inference):
    `model.txt_net.encoder.CLIP_encoder = ClipTxtEncoder.from_state_dict(sd, ClipTokenizer(bpe_path))`.
    Parameters keep the reference's names under `ClipModel.` (ClipModel.token_embedding.weight, ClipModel.transformer.resblocks.0.
    attn.in_proj_weight, ...).  precision: 'fp16' (fp16 matrix operands, fp32 accumulation, LayerNorm and residual stream; what
    clip.load does on a GPU, with a more accurate residual) or 'fp32' (fp32 MFMA throughout).
    forward returns caption_feat_dict['CLIP_encoding'] when the dict has it (as the frozen reference does), otherwise encodes
    caption_feat_dict['caption']: {'text_features': (N, embed_dim) fp32}.  A caption's feature is bitwise the same in any batch.
    The packed weights are cached and rebuilt whenever a parameter changes (load_state_dict, copy_, ...).  max_rows bounds the
    token rows per device call (and so the workspace); it does not change any result."""

    feature_key = 'CLIP_encoding'

    def __init__(self, tokenizer, width, layers, heads, embed_dim, context_length=77, vocab_size=49408, precision='fp16',
                 device='cuda', max_rows=1 << 16):
        super().__init__()
        width, layers, heads = int(width), int(layers), int(heads)
        _check_dims('ClipTxtEncoder', precision, width, heads, layers)
        if not 1 <= int(context_length) <= 77:
            raise NotImplementedError('ClipTxtEncoder: context_length=%d; at most 77 positions' % context_length)
        self.tokenizer, self.device, self.precision = tokenizer, device, precision
        self.width, self.layers, self.heads, self.embed_dim = width, layers, heads, int(embed_dim)
        self.context_length, self.vocab_size, self.max_rows = int(context_length), int(vocab_size), int(max_rows)
        self.out_width, self.max_len = self.embed_dim, self.context_length
        self.ClipModel = _ClipText(width, layers, self.embed_dim, self.context_length, self.vocab_size)
        self.to(device)
        self._weights = _Weights(self.ClipModel, precision)

    @staticmethod
    def text_state_dict(sd):
        """The text entries of a CLIP state dict (bare, or with the `ClipModel.` prefix), without the prefix."""
        pre = 'ClipModel.'
        if any(k.startswith(pre) for k in sd):
            sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        return {k: v for k, v in sd.items() if not k.startswith(_IGNORED)}

    @staticmethod
    def dims(sd):
        """(width, layers, heads, embed_dim, context_length, vocab_size) the way clip.model.build_model infers them."""
        sd = ClipTxtEncoder.text_state_dict(sd)
        width = sd['ln_final.weight'].shape[0]
        layers = len(set(k.split('.')[2] for k in sd if k.startswith('transformer.resblocks')))
        return (int(width), layers, int(width) // 64, int(sd['text_projection'].shape[1]), int(sd['positional_embedding'].shape[0]),
                int(sd['token_embedding.weight'].shape[0]))

    @classmethod
    def from_state_dict(cls, sd, tokenizer, precision='fp16', device='cuda', **kw):
        width, layers, heads, embed, ctx, vocab = cls.dims(sd)
        enc = cls(tokenizer, width, layers, heads, embed, ctx, vocab, precision=precision, device=device, **kw)
        text = cls.text_state_dict(sd)
        enc.ClipModel.load_state_dict({k: torch.as_tensor(v, dtype=torch.float32) for k, v in text.items()}, strict=True)
        return enc

    def _model(self):
        """The packed weights and the laff_clip_text struct, rebuilt when any parameter has changed since the last build."""
        from . import _lib
        m = self.ClipModel
        return self._weights.get(lambda w: _lib.ClipText(
            self.width, self.layers, self.heads, self.embed_dim, self.context_length, self.vocab_size, w.f32(m.token_embedding.weight),
            w.f32(m.positional_embedding), w.blocks(m.transformer.resblocks), w.f32(m.ln_final.weight), w.f32(m.ln_final.bias),
            w.packed(m.text_projection, transpose=True)))

    def _tokenize(self, captions):
        """ClipTokenizer.batch at this encoder's context length."""
        return self.tokenizer.batch(captions, self.context_length)

    def workspace_bytes(self, b):
        from . import ops
        return ops.clip_workspace_bytes(int(b.row_off_host[-1]), len(b.row_off_host) - 1, self.width, self.precision)

    def encode_batch(self, b, out=None, workspace=None):
        """The device half of forward(): a ClipBatch on the device, in one call (allocates nothing when out and workspace are given)."""
        from . import ops
        return ops.clip_encode(b.ids, b.row_off, b.row_off_host, self._model(), self.precision, out=out, workspace=workspace)
