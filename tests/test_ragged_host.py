"""laff_amd/ragged.py without a GPU: the ragged batch builder, the budgeted chunker, the token-row limit the three transformer entry
points share, and the state-dict keys of the two text encoders over their common base class."""
import ctypes as C

import numpy as np
import pytest
import torch

from laff_amd import bert_text as BT
from laff_amd import clip_text as CT
from laff_amd import ragged


@pytest.mark.parametrize('rows,ids,row_off', [([], [], [0]), ([[7]], [7], [0, 1]), ([[1, 2, 3], [], [4]], [1, 2, 3, 4], [0, 3, 3, 4])])
def test_ragged_batch(rows, ids, row_off):
    b = ragged.ragged_batch(rows)
    assert isinstance(b, ragged.RaggedBatch) and CT.ClipBatch is ragged.RaggedBatch and BT.BertBatch is ragged.RaggedBatch
    assert b.ids.dtype == np.int32 and b.row_off.dtype == np.int32 and b.row_off_host.dtype == np.int32
    assert b.ids.tolist() == ids and b.row_off.tolist() == row_off and b.row_off_host.tolist() == row_off


@pytest.mark.parametrize('budget', [1, 7, 8, 100])
def test_chunks_tile_the_items_within_the_budget(budget):
    off = np.array([0, 3, 3, 10, 11, 30])
    n, at, asked, seen = len(off) - 1, 0, [], []

    def workspace_bytes(i0, i1):
        asked.append(int(off[i1] - off[i0]) * 16 + 16)
        return asked[-1]
    for i0, i1, ws in ragged._chunks(off, budget, workspace_bytes, 'cpu'):
        assert i0 == at and i1 > i0                                 # in order, without gaps, one item at least
        span = int(off[i1] - off[i0])
        assert span <= budget or i1 - i0 == 1                       # within the budget; a longer item comes alone
        if i1 < n:
            assert int(off[i1 + 1] - off[i0]) > budget              # and no chunk stops early
        assert ws.dtype == torch.uint8 and ws.device.type == 'cpu' and ws.numel() >= asked[-1]
        seen.append(ws)
        at = i1
    assert at == n
    for k in range(1, len(seen)):                                   # reused while large enough, replaced only to grow
        grew = asked[k] > seen[k - 1].numel()
        assert (seen[k] is not seen[k - 1]) == grew and (not grew or seen[k].numel() == asked[k])
    assert CT._chunks is ragged._chunks and CT._Weights is ragged._Weights        # the re-export


def test_clip_encode_refuses_more_than_the_token_row_limit_before_its_pointers():
    from laff_amd import _lib
    lib = _lib.load()
    fake = 4096                                                     # never dereferenced
    blk = (_lib.ClipBlock * 2)(*[_lib.ClipBlock(*([fake] * 12)) for _ in range(2)])
    m = _lib.ClipText(128, 2, 2, 64, 77, 49408, fake, fake, blk, fake, fake, fake)
    R = (1 << 22) + 1
    assert lib.laff_clip_encode(None, None, None, None, 1, R, C.byref(m), 1, None, 64, None, 0) == -2      # LAFF_E_SHAPE
    assert b'laff_clip_encode: R=4194305: more than 4,194,304 token rows' in lib.laff_last_error()
    assert lib.laff_clip_encode(None, None, None, None, 1, R - 1, C.byref(m), 1, None, 64, None, 0) == -1  # the limit itself passes
    assert b'null argument' in lib.laff_last_error()


CLIP_KEYS = ['ClipModel.ln_final.bias', 'ClipModel.ln_final.weight', 'ClipModel.positional_embedding', 'ClipModel.text_projection',
             'ClipModel.token_embedding.weight', 'ClipModel.transformer.resblocks.0.attn.in_proj_bias',
             'ClipModel.transformer.resblocks.0.attn.in_proj_weight', 'ClipModel.transformer.resblocks.0.attn.out_proj.bias',
             'ClipModel.transformer.resblocks.0.attn.out_proj.weight', 'ClipModel.transformer.resblocks.0.ln_1.bias',
             'ClipModel.transformer.resblocks.0.ln_1.weight', 'ClipModel.transformer.resblocks.0.ln_2.bias',
             'ClipModel.transformer.resblocks.0.ln_2.weight', 'ClipModel.transformer.resblocks.0.mlp.c_fc.bias',
             'ClipModel.transformer.resblocks.0.mlp.c_fc.weight', 'ClipModel.transformer.resblocks.0.mlp.c_proj.bias',
             'ClipModel.transformer.resblocks.0.mlp.c_proj.weight']
BERT_KEYS = ['BertModel.embeddings.LayerNorm.bias', 'BertModel.embeddings.LayerNorm.weight',
             'BertModel.embeddings.position_embeddings.weight', 'BertModel.embeddings.token_type_embeddings.weight',
             'BertModel.embeddings.word_embeddings.weight', 'BertModel.encoder.layer.0.attention.output.LayerNorm.bias',
             'BertModel.encoder.layer.0.attention.output.LayerNorm.weight', 'BertModel.encoder.layer.0.attention.output.dense.bias',
             'BertModel.encoder.layer.0.attention.output.dense.weight', 'BertModel.encoder.layer.0.attention.self.key.bias',
             'BertModel.encoder.layer.0.attention.self.key.weight', 'BertModel.encoder.layer.0.attention.self.query.bias',
             'BertModel.encoder.layer.0.attention.self.query.weight', 'BertModel.encoder.layer.0.attention.self.value.bias',
             'BertModel.encoder.layer.0.attention.self.value.weight', 'BertModel.encoder.layer.0.intermediate.dense.bias',
             'BertModel.encoder.layer.0.intermediate.dense.weight', 'BertModel.encoder.layer.0.output.LayerNorm.bias',
             'BertModel.encoder.layer.0.output.LayerNorm.weight', 'BertModel.encoder.layer.0.output.dense.bias',
             'BertModel.encoder.layer.0.output.dense.weight', 'BertModel.pooler.dense.bias', 'BertModel.pooler.dense.weight']


def test_the_base_class_registers_nothing():
    clip = CT.ClipTxtEncoder(None, 64, 1, 1, 32, device='cpu')
    assert sorted(clip.state_dict()) == CLIP_KEYS
    cfg = {'hidden_size': 64, 'num_attention_heads': 1, 'num_hidden_layers': 1, 'intermediate_size': 128,
           'max_position_embeddings': 16, 'vocab_size': 50}
    bert = BT.BertTxtEncoder(None, cfg, device='cpu')
    assert sorted(bert.state_dict()) == BERT_KEYS
    assert (clip.feature_key, clip.out_width, clip.max_len) == ('CLIP_encoding', 32, 77)
    assert (bert.feature_key, bert.out_width, bert.max_len) == ('bert_encoding', 64, 16)
