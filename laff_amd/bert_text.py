"""The BERT text encoder on the device: caption strings -> bert_encoding (pooler_output), a drop-in for the reference's
`BertTxtEncoder` (model/model.py:437-466) over transformers' `BertTokenizer` + `BertModel`.

The host tokenises (`BertTokenizer`: the rules of transformers 4.3.2's slow BertTokenizer, BasicTokenizer + WordPiece, in pure Python)
and lays the batch out ragged (`BertTokenizer.batch`); the encoder runs on the GPU (`laff_bert_encode`, laff_amd/csrc/bert.hip).

Ragged layout.  The reference pads every caption to the longest of its batch and passes the attention mask, which gives the padded
keys a weight of exactly 0: each caption's rows are its unpadded computation, so caption i contributes only its own rows
[CLS] ... [SEP].  That is exact, not an approximation.  The pooler reads row 0 of each caption (its [CLS] row).

The vocabulary (`vocab.txt` of a BERT checkpoint) is an input of the deployment: pass its path, or load a local checkpoint directory
with `BertTxtEncoder.from_pretrained`.  Nothing is ever fetched.
"""
import json
import os
import re
import unicodedata

import numpy as np
import torch
import torch.nn as nn

from .ragged import RaggedBatch as BertBatch, _TextEncoder, _Weights, ragged_batch

SPECIALS = ('[UNK]', '[SEP]', '[PAD]', '[CLS]', '[MASK]')
MAX_POSITION = 512                                        # what bert.hip's limits take (BertConfig's default as well)


def _is_whitespace(ch):
    return ch in ' \t\n\r' or unicodedata.category(ch) == 'Zs'


def _is_control(ch):
    return ch not in '\t\n\r' and unicodedata.category(ch).startswith('C')


def _is_punctuation(ch):
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith('P')


def _is_cjk(cp):
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or
            0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class BertTokenizer(object):
    """transformers.BertTokenizer (4.3.2, the slow Python tokenizer) as `tokenizer(captions, padding=True, truncation=True)` uses it:
      * the text is split on the special tokens' literal text ([UNK], [SEP], [PAD], [CLS], [MASK]; case-sensitive), which map to
        their ids;
      * BasicTokenizer on the rest: drop NUL, U+FFFD and control characters, map whitespace to spaces, put spaces around CJK
        characters, split on whitespace, lower-case and strip accents (NFD, drop Mn) when do_lower_case, split on punctuation;
      * WordPiece: greedy longest match with '##' continuations; a word of more than 100 characters, or with a piece that matches
        nothing, becomes [UNK];
      * [CLS] + pieces + [SEP], the pieces cut at max_length - 2.
    vocab_path: the checkpoint's vocab.txt (one token per line, id = line number); the special ids are looked up there by name."""

    def __init__(self, vocab_path, do_lower_case=True, max_length=MAX_POSITION, max_input_chars_per_word=100):
        self.vocab = {}
        with open(vocab_path, encoding='utf-8') as f:
            for i, line in enumerate(f):                  # as transformers' load_vocab: id = line number, a repeated token's last
                self.vocab[line.rstrip('\n')] = i
        for s in ('[UNK]', '[CLS]', '[SEP]'):
            if s not in self.vocab:
                raise ValueError('%s: no %s token' % (vocab_path, s))
        if max_length < 2:
            raise ValueError('max_length=%d: [CLS] and [SEP] need 2' % max_length)
        self.unk, self.cls, self.sep = self.vocab['[UNK]'], self.vocab['[CLS]'], self.vocab['[SEP]']
        self.do_lower_case, self.max_length, self.max_chars = bool(do_lower_case), int(max_length), int(max_input_chars_per_word)
        self.vocab_size = max(self.vocab.values()) + 1
        specials = [s for s in SPECIALS if s in self.vocab]
        self._special = re.compile('(' + '|'.join(re.escape(s) for s in specials) + ')')

    def _basic(self, text):
        out = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                out.append(' ')
            elif _is_cjk(cp):
                out.append(' %s ' % ch)
            else:
                out.append(ch)
        words = []
        for w in ''.join(out).split():
            if self.do_lower_case:
                w = ''.join(c for c in unicodedata.normalize('NFD', w.lower()) if unicodedata.category(c) != 'Mn')
            cur = None
            for ch in w:                                   # split on punctuation: every punctuation character is a word
                if _is_punctuation(ch):
                    words.append(ch)
                    cur = None
                else:
                    if cur is None:
                        words.append('')
                        cur = len(words) - 1
                    words[cur] += ch
        return [w for w in words if w]

    def _wordpiece(self, word):
        if len(word) > self.max_chars:
            return [self.unk]
        pieces, start = [], 0
        while start < len(word):
            end = len(word)
            while start < end:
                sub = word[start:end] if start == 0 else '##' + word[start:end]
                if sub in self.vocab:
                    pieces.append(self.vocab[sub])
                    break
                end -= 1
            else:
                return [self.unk]
            start = end
        return pieces

    def encode(self, text):
        """The wordpiece ids of one caption, without [CLS] / [SEP] and uncut."""
        ids = []
        for i, part in enumerate(self._special.split(text)):
            if i % 2:
                ids.append(self.vocab[part])
            else:
                for w in self._basic(part):
                    ids.extend(self._wordpiece(w))
        return ids

    def tokens(self, text):
        """One caption's row: [CLS] + pieces (at most max_length - 2) + [SEP]."""
        return [self.cls] + self.encode(text)[:self.max_length - 2] + [self.sep]

    def batch(self, texts):
        return ragged_batch([self.tokens(t) for t in texts])


class _Layer(nn.Module):
    """One BertLayer's parameters under transformers' names."""

    def __init__(self, width, intermediate):
        super().__init__()
        self.attention = nn.Module()
        self.attention.self = nn.Module()
        for n in ('query', 'key', 'value'):
            setattr(self.attention.self, n, nn.Linear(width, width))
        self.attention.output = nn.Module()
        self.attention.output.dense = nn.Linear(width, width)
        self.attention.output.LayerNorm = nn.LayerNorm(width)
        self.intermediate = nn.Module()
        self.intermediate.dense = nn.Linear(width, intermediate)
        self.output = nn.Module()
        self.output.dense = nn.Linear(intermediate, width)
        self.output.LayerNorm = nn.LayerNorm(width)


class _BertModel(nn.Module):
    """transformers.BertModel's parameters (add_pooling_layer) under their names there, at BertConfig's initializer_range."""

    def __init__(self, width, layers, intermediate, max_position, vocab_size, type_vocab_size):
        super().__init__()
        self.embeddings = nn.Module()
        self.embeddings.word_embeddings = nn.Embedding(vocab_size, width)
        self.embeddings.position_embeddings = nn.Embedding(max_position, width)
        self.embeddings.token_type_embeddings = nn.Embedding(type_vocab_size, width)
        self.embeddings.LayerNorm = nn.LayerNorm(width)
        self.encoder = nn.Module()
        self.encoder.layer = nn.ModuleList([_Layer(width, intermediate) for _ in range(layers)])
        self.pooler = nn.Module()
        self.pooler.dense = nn.Linear(width, width)
        with torch.no_grad():
            for n, p in self.named_parameters():
                if 'LayerNorm' in n:
                    continue
                if n.endswith('bias'):
                    p.zero_()
                else:
                    p.normal_(0, 0.02)


_IGNORED = ('cls.', 'embeddings.position_ids', 'embeddings.token_type_ids')


def _check_config(cfg):
    """The refusals of what bert.hip does not take, from a BertConfig-like dict."""
    name = 'BertTxtEncoder'
    if cfg.get('hidden_act', 'gelu') != 'gelu':
        raise NotImplementedError("%s: hidden_act=%r; only 'gelu' (erf) is supported" % (name, cfg['hidden_act']))
    if cfg.get('position_embedding_type', 'absolute') != 'absolute':
        raise NotImplementedError("%s: position_embedding_type=%r; only 'absolute'" % (name, cfg['position_embedding_type']))
    if cfg.get('is_decoder') or cfg.get('add_cross_attention'):
        raise NotImplementedError('%s: decoder / cross-attention configs are not supported' % name)
    width, heads = int(cfg['hidden_size']), int(cfg['num_attention_heads'])
    if width % 64 or not 64 <= width <= 1024:
        raise NotImplementedError('%s: hidden_size=%d; the kernels take multiples of 64 up to 1024' % (name, width))
    if heads * 64 != width:
        raise NotImplementedError('%s: hidden_size=%d heads=%d; only a head dim of 64 is supported' % (name, width, heads))
    inter = int(cfg['intermediate_size'])
    if inter < 64 or inter % 64:
        raise NotImplementedError('%s: intermediate_size=%d; the GEMM takes positive multiples of 64' % (name, inter))
    if not 1 <= int(cfg['max_position_embeddings']) <= MAX_POSITION:
        raise NotImplementedError('%s: max_position_embeddings=%d; at most %d positions'
                                  % (name, cfg['max_position_embeddings'], MAX_POSITION))
    if int(cfg['num_hidden_layers']) < 1:
        raise NotImplementedError('%s: num_hidden_layers=%d; at least one layer' % (name, cfg['num_hidden_layers']))


class BertTxtEncoder(_TextEncoder):
    """Drop-in for model.model.BertTxtEncoder (frozen, inference):
    `model.txt_net.encoder.bert_encoder = BertTxtEncoder.from_pretrained(local_dir)` (or from_state_dict(sd, BertTokenizer(vocab))).
    Parameters keep transformers' names under `BertModel.` (BertModel.embeddings.word_embeddings.weight, BertModel.encoder.layer.3.
    attention.self.query.weight, BertModel.pooler.dense.bias, ...), so a reference LAFF checkpoint loads by name.
    precision: 'fp32' (the default: the reference runs BERT in fp32; fp32 MFMA throughout) or 'fp16' (fp16 matrix operands, fp32
    accumulation, LayerNorm, softmax and residual stream).
    forward returns caption_feat_dict['bert_encoding'] when the dict has it (as the frozen reference does), otherwise encodes
    caption_feat_dict['caption']: {'text_features': (N, hidden) fp32}.  A caption's feature is bitwise the same in any batch.
    The packed weights are cached and rebuilt whenever a parameter changes (load_state_dict, copy_, ...).  max_rows bounds the
    token rows per device call (and so the workspace); it does not change any result."""

    feature_key = 'bert_encoding'

    def __init__(self, tokenizer, config, precision='fp32', device='cuda', max_rows=1 << 16):
        super().__init__()
        cfg = dict(config)
        _check_config(cfg)
        if precision not in ('fp16', 'fp32'):
            raise NotImplementedError("BertTxtEncoder: precision %r; 'fp16' or 'fp32'" % (precision,))
        self.tokenizer, self.device, self.precision, self.max_rows = tokenizer, device, precision, int(max_rows)
        self.width, self.heads = int(cfg['hidden_size']), int(cfg['num_attention_heads'])
        self.layers, self.intermediate = int(cfg['num_hidden_layers']), int(cfg['intermediate_size'])
        self.max_position, self.vocab_size = int(cfg['max_position_embeddings']), int(cfg['vocab_size'])
        self.type_vocab_size = int(cfg.get('type_vocab_size', 2))
        self.layer_norm_eps = float(cfg.get('layer_norm_eps', 1e-12))
        self.out_width, self.max_len = self.width, self.max_position
        self.BertModel = _BertModel(self.width, self.layers, self.intermediate, self.max_position, self.vocab_size, self.type_vocab_size)
        self.to(device)
        self._weights = _Weights(self.BertModel, precision)

    @staticmethod
    def model_state_dict(sd):
        """The BertModel entries of a state dict (bare, or under `bert.` or `BertModel.`), bare, with LayerNorm.gamma / beta renamed
        to weight / bias and cls.*, embeddings.position_ids and embeddings.token_type_ids left out."""
        for pre in ('BertModel.', 'bert.'):
            if any(k.startswith(pre) for k in sd):
                sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
                break
        out = {}
        for k, v in sd.items():
            if k.startswith(_IGNORED):
                continue
            out[k.replace('LayerNorm.gamma', 'LayerNorm.weight').replace('LayerNorm.beta', 'LayerNorm.bias')] = v
        return out

    @staticmethod
    def config_from_state_dict(sd, num_attention_heads=None, layer_norm_eps=1e-12):
        """A BertConfig-like dict from the shapes (heads: hidden / 64 unless given)."""
        sd = BertTxtEncoder.model_state_dict(sd)
        word = sd['embeddings.word_embeddings.weight']
        width = int(word.shape[1])
        return {'hidden_size': width, 'num_attention_heads': int(num_attention_heads or width // 64),
                'num_hidden_layers': len(set(k.split('.')[2] for k in sd if k.startswith('encoder.layer.'))),
                'intermediate_size': int(sd['encoder.layer.0.intermediate.dense.weight'].shape[0]),
                'max_position_embeddings': int(sd['embeddings.position_embeddings.weight'].shape[0]),
                'vocab_size': int(word.shape[0]), 'type_vocab_size': int(sd['embeddings.token_type_embeddings.weight'].shape[0]),
                'layer_norm_eps': float(layer_norm_eps), 'hidden_act': 'gelu', 'position_embedding_type': 'absolute'}

    @classmethod
    def from_state_dict(cls, sd, tokenizer, precision='fp32', device='cuda', config=None, **kw):
        """The dimensions from the shapes (or config, a BertConfig-like dict), the parameters loaded strictly."""
        config = config if config is not None else cls.config_from_state_dict(sd)
        enc = cls(tokenizer, config, precision=precision, device=device, **kw)
        enc.BertModel.load_state_dict({k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v, dtype=torch.float32)
                                       for k, v in cls.model_state_dict(sd).items()}, strict=True)
        return enc

    @classmethod
    def from_pretrained(cls, local_dir, precision='fp32', device='cuda', **kw):
        """A local checkpoint directory: config.json, vocab.txt, the optional tokenizer_config.json (do_lower_case) and
        pytorch_model.bin (torch.load, weights_only) or model.safetensors (when safetensors is importable)."""
        with open(os.path.join(local_dir, 'config.json')) as f:
            config = json.load(f)
        lower, tc = True, os.path.join(local_dir, 'tokenizer_config.json')
        if os.path.exists(tc):
            with open(tc) as f:
                lower = bool(json.load(f).get('do_lower_case', True))
        tok = BertTokenizer(os.path.join(local_dir, 'vocab.txt'), do_lower_case=lower,
                            max_length=min(int(config['max_position_embeddings']), MAX_POSITION))
        bin_, st = os.path.join(local_dir, 'pytorch_model.bin'), os.path.join(local_dir, 'model.safetensors')
        if os.path.exists(bin_):
            sd = torch.load(bin_, map_location='cpu', weights_only=True)
        elif os.path.exists(st):
            try:
                from safetensors.torch import load_file
            except ImportError:
                raise RuntimeError('%s holds model.safetensors only and safetensors is not importable' % local_dir)
            sd = load_file(st)
        else:
            raise FileNotFoundError('%s: no pytorch_model.bin or model.safetensors' % local_dir)
        return cls.from_state_dict(sd, tok, precision=precision, device=device, config=config, **kw)

    def _model(self):
        """The packed weights and the laff_bert_text struct, rebuilt when any parameter has changed since the last build."""
        from . import _lib
        m = self.BertModel

        def build(w):
            f32, packed = w.f32, w.packed
            blocks = (_lib.BertBlock * self.layers)()
            for i, b in enumerate(m.encoder.layer):
                s = b.attention.self
                qkv_w = torch.cat([s.query.weight, s.key.weight, s.value.weight])
                qkv_b = torch.cat([s.query.bias, s.key.bias, s.value.bias])
                blocks[i] = _lib.BertBlock(packed(qkv_w), f32(qkv_b), packed(b.attention.output.dense.weight),
                                           f32(b.attention.output.dense.bias), f32(b.attention.output.LayerNorm.weight),
                                           f32(b.attention.output.LayerNorm.bias), packed(b.intermediate.dense.weight),
                                           f32(b.intermediate.dense.bias), packed(b.output.dense.weight), f32(b.output.dense.bias),
                                           f32(b.output.LayerNorm.weight), f32(b.output.LayerNorm.bias))
            w._keep.append(blocks)
            e = m.embeddings
            return _lib.BertText(self.width, self.layers, self.heads, self.intermediate, self.max_position, self.vocab_size,
                                 self.layer_norm_eps, f32(e.word_embeddings.weight), f32(e.position_embeddings.weight),
                                 f32(e.token_type_embeddings.weight[0]), f32(e.LayerNorm.weight), f32(e.LayerNorm.bias), blocks,
                                 packed(m.pooler.dense.weight), f32(m.pooler.dense.bias))
        return self._weights.get(build)

    def _tokenize(self, captions):
        """BertTokenizer.batch, cut at this encoder's positions."""
        b = self.tokenizer.batch(captions)
        if len(b.row_off) > 1 and int(np.diff(b.row_off).max()) > self.max_position:
            raise ValueError('a caption of %d tokens: the encoder has %d positions (tokenizer max_length)'
                             % (int(np.diff(b.row_off).max()), self.max_position))
        return b

    def workspace_bytes(self, b):
        from . import ops
        return ops.bert_workspace_bytes(int(b.row_off_host[-1]), len(b.row_off_host) - 1, self.width, self.intermediate, self.precision)

    def encode_batch(self, b, out=None, workspace=None):
        """The device half of forward(): a BertBatch on the device, in one call (allocates nothing when out and workspace are given)."""
        from . import ops
        return ops.bert_encode(b.ids, b.row_off, b.row_off_host, self._model(), self.precision, out=out, workspace=workspace)
