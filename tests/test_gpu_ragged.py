"""The max_rows loop the two transformer text encoders share (laff_amd/ragged.py) on a real MI355X: a row budget below one caption's
length, three device calls at least, bitwise the result of one call."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from laff_amd import bert_text as BT
from laff_amd import clip_text as CT

pytestmark = pytest.mark.gpu
CAPTIONS = ['a man is playing a guitar on the stage and a dog is running', 'a dog', 'a red car', 'the cat is running', 'a']


def chunked_equals_one_call(enc):
    """5 captions of at most 8 rows, one of them longer than max_rows = 4 (which is raised to the 8 rows a caption may have)."""
    off = enc.batch(CAPTIONS).row_off_host
    assert 4 < int(np.diff(off).max()) <= 8 and int(off[-1]) > 16
    whole = enc.encode(CAPTIONS)
    calls, run = [], enc.encode_batch
    enc.encode_batch = lambda b, **kw: calls.append(len(b.row_off_host) - 1) or run(b, **kw)
    chunked = enc.encode(CAPTIONS, max_rows=4)
    assert len(calls) >= 3 and sum(calls) == 5
    assert torch.equal(chunked, whole) and bool(torch.isfinite(whole).all())


def test_clip_max_rows_loop_is_bitwise_one_call():
    torch.manual_seed(5)
    tok = CT.ClipTokenizer(os.path.join(GOLDEN, 'clip_bpe_subset.txt.gz'))
    chunked_equals_one_call(CT.ClipTxtEncoder(tok, 64, 2, 1, 32, context_length=8, device='cuda'))


def test_bert_max_rows_loop_is_bitwise_one_call():
    torch.manual_seed(5)
    tok = BT.BertTokenizer(os.path.join(GOLDEN, 'bert_vocab.txt'), max_length=8)
    cfg = {'hidden_size': 64, 'num_attention_heads': 1, 'num_hidden_layers': 2, 'intermediate_size': 128,
           'max_position_embeddings': 8, 'vocab_size': tok.vocab_size}
    chunked_equals_one_call(BT.BertTxtEncoder(tok, cfg, device='cuda'))
