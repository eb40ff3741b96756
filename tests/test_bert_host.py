"""The BERT text encoder's host side, without a GPU: captions -> ids (the slow BertTokenizer's rules), the ragged layout, the float64
restatement against the reference's BertTxtEncoder, the module's state-dict handling, loading and refusals, the C entry points'
argument checks and the ISA of bert.hip's kernels."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from bert_ref import encode64, full_bert_sd, padded
from conftest import GOLDEN, ROOT
from laff_amd import bert_text as BT

VOCAB = os.path.join(GOLDEN, 'bert_vocab.txt')


@pytest.fixture(scope='module')
def tok():
    return BT.BertTokenizer(VOCAB)


def fixture_rows(z):
    """The reference tokenizer's rows of the fixture, without their padding."""
    return [r[m == 1].tolist() for r, m in zip(z['ids'], z['mask'])]


def test_tokenizer_reproduces_the_reference_ids(golden, tok):
    z = golden('bert_text')
    caps = z.json('captions')
    assert len(caps) >= 30 and (tok.unk, tok.cls, tok.sep, tok.vocab['[PAD]'], tok.vocab['[MASK]']) == (100, 101, 102, 0, 103)
    want = fixture_rows(z)
    for c, w in zip(caps, want):
        assert tok.tokens(c) == w, c
    assert want[0] == [101, 102]                                      # ''
    assert len(want[-1]) == 512 and want[-1][-1] == 102               # cut at 510 pieces + [CLS] / [SEP]
    assert want[caps.index('hello [SEP] world')].count(102) == 2      # literal special text maps to the special id
    assert 100 in want[caps.index('[UNK] token [CLS]x[MASK]')] and 103 in want[caps.index('[UNK] token [CLS]x[MASK]')]
    assert 102 not in want[caps.index('lower case [sep] is not special')][1:-1]
    assert want[caps.index('the ' + 'a' * 101 + ' dog')][2] == 100    # a word of more than 100 characters
    assert 100 not in want[caps.index('the ' + 'b' * 100 + ' cat')]   # ... and one of exactly 100
    assert 100 in want[caps.index('an emoji \U0001F642 cat')]           # a character outside the vocabulary
    assert want[caps.index('a café in the naïve city of Zürich')] == tok.tokens('a cafe in the naive city of zurich')


def test_tokenizer_matches_transformers_where_importable(tok, tmp_path):
    """transformers' own BertTokenizer on the fixture vocabulary (a local directory, as the reference loads it), over a wider caption
    set (skipped without transformers)."""
    transformers = pytest.importorskip('transformers')
    (tmp_path / 'vocab.txt').write_text(open(VOCAB, encoding='utf-8').read(), encoding='utf-8')
    (tmp_path / 'tokenizer_config.json').write_text(json.dumps({'do_lower_case': True, 'model_max_length': 512}))
    ref = transformers.BertTokenizer.from_pretrained(str(tmp_path), do_lower_case=True)
    g = np.random.default_rng(3)
    alphabet = list('abcdefghijklmnopqrstuvwxyz ABCXYZ0123456789.,;:!?-\'"()[]{}<>&@#$%^*_+=/\\|~`') + \
        list('éèêëàâäôöûüçñÉÀ中文猫狗一只和ωπ 　\t\n\x00\x07�\U0001F642́')
    caps = [''.join(g.choice(alphabet, int(g.integers(0, 60)))) for _ in range(400)]
    caps += ['[SEP]', '[CLS][SEP]', ' [UNK] ', 'x[PAD]y', '[MASK]', '[sep]', '[Sep]', 'a' * 100, 'a' * 101, 'thé ' * 300,
             'don\'t stop', '...', '́́', 'áb']
    for c in caps:
        want = ref(c, truncation=True)['input_ids']
        assert tok.tokens(c) == want, repr(c)


def test_ragged_layout(golden, tok):
    z = golden('bert_text')
    caps = z.json('captions')
    b = tok.batch(caps)
    rows = fixture_rows(z)
    assert b.ids.dtype == np.int32 and b.row_off.dtype == np.int32 and b.row_off[0] == 0
    assert np.array_equal(np.diff(b.row_off), z['mask'].sum(axis=1))
    for i, r in enumerate(rows):
        assert b.ids[b.row_off[i]:b.row_off[i + 1]].tolist() == r
        assert b.ids[b.row_off[i]] == 101                             # the CLS row the pooler reads
    ids, mask = padded(b.row_off, b.ids)
    assert np.array_equal(ids, z['ids']) and np.array_equal(mask, z['mask'])
    assert b.row_off[-1] < 0.1 * z['ids'].size                        # the ragged rows are well under the padded work
    empty = tok.batch([])
    assert empty.ids.size == 0 and empty.row_off.tolist() == [0]


def test_float64_restatement_reproduces_the_reference(golden):
    z = golden('bert_text')
    got = encode64(z['ids'], z['mask'], full_bert_sd(z))
    want = z['pooler_output']
    assert got.shape == want.shape == (len(z.json('captions')), 128)
    assert np.abs(got - want).max() <= 1e-5


def test_float64_ragged_equals_padded(golden, tok):
    """Each caption alone (no padding) gives its row of the padded batch: the key mask at work."""
    z = golden('bert_text')
    sd = full_bert_sd(z)
    batch = encode64(z['ids'], z['mask'], sd)
    b = tok.batch(z.json('captions'))
    for i in range(len(b.row_off) - 1):
        r0, r1 = b.row_off[i], b.row_off[i + 1]
        alone = encode64(*padded(np.array([0, r1 - r0]), b.ids[r0:r1]), sd)
        assert np.abs(alone[0] - batch[i]).max() <= 1e-12


def hf_names(sd):
    return {'BertModel.' + k for k in sd}


def test_from_state_dict_takes_the_three_prefixes_and_the_legacy_names(golden, tok):
    z = golden('bert_text')
    sd = full_bert_sd(z)
    cfg = z.json('cfg')
    legacy = {k.replace('LayerNorm.weight', 'LayerNorm.gamma').replace('LayerNorm.bias', 'LayerNorm.beta'): v for k, v in sd.items()}
    extra = {'embeddings.position_ids': np.arange(512)[None], 'embeddings.token_type_ids': np.zeros((1, 512), np.int64)}
    head = {'cls.predictions.bias': np.zeros(cfg['vocab_size'], np.float32),
            'cls.predictions.transform.dense.weight': np.zeros((128, 128), np.float32)}
    sources = ({**sd, **extra}, {'bert.' + k: v for k, v in {**legacy, **extra}.items()} | head,
               {'BertModel.' + k: v for k, v in sd.items()}, legacy)
    for src in sources:
        enc = BT.BertTxtEncoder.from_state_dict(src, tok, device='cpu')
        assert (enc.width, enc.heads, enc.layers, enc.intermediate, enc.max_position, enc.vocab_size) == (128, 2, 2, 512, 512, 377)
        assert enc.precision == 'fp32' and enc.layer_norm_eps == 1e-12
        got = enc.state_dict()
        assert set(got) == hf_names(sd)
        for k in ('encoder.layer.1.attention.self.key.weight', 'encoder.layer.0.output.LayerNorm.bias', 'pooler.dense.bias'):
            assert torch.equal(got['BertModel.' + k], torch.from_numpy(sd[k]))
    assert {'BertModel.embeddings.word_embeddings.weight', 'BertModel.encoder.layer.1.attention.self.query.weight',
            'BertModel.pooler.dense.bias', 'BertModel.embeddings.LayerNorm.weight'} <= set(got)
    with pytest.raises(RuntimeError, match='Unexpected'):
        BT.BertTxtEncoder.from_state_dict({**sd, 'encoder.layer.0.attention.self.extra': np.zeros(3, np.float32)}, tok, device='cpu')
    with pytest.raises(RuntimeError, match='Missing'):
        BT.BertTxtEncoder.from_state_dict({k: v for k, v in sd.items() if k != 'pooler.dense.bias'}, tok, device='cpu')


def test_reference_checkpoint_loads_by_name(golden, tok):
    """A reference LAFF checkpoint keeps BertTxtEncoder's weights as txt_net.encoder.bert_encoder.BertModel.*: the encoder's own
    state dict, under that prefix, loads strictly."""
    z = golden('bert_text')
    enc = BT.BertTxtEncoder.from_state_dict(full_bert_sd(z), tok, device='cpu')
    holder = torch.nn.Module()
    holder.encoder = torch.nn.Module()
    holder.encoder.bert_encoder = BT.BertTxtEncoder(tok, z.json('cfg'), device='cpu')
    ckpt = {'encoder.bert_encoder.' + k: v for k, v in enc.state_dict().items()}
    holder.load_state_dict(ckpt, strict=True)
    assert torch.equal(holder.encoder.bert_encoder.BertModel.pooler.dense.weight, enc.BertModel.pooler.dense.weight)


@pytest.mark.parametrize('fmt', ['bin', 'safetensors'])
def test_from_pretrained_reads_a_local_directory(golden, tmp_path, fmt):
    z = golden('bert_text')
    sd = {k: torch.from_numpy(v) for k, v in full_bert_sd(z).items()}
    cfg = dict(z.json('cfg'), architectures=['BertModel'], model_type='bert')
    (tmp_path / 'config.json').write_text(json.dumps(cfg))
    (tmp_path / 'vocab.txt').write_text(open(VOCAB, encoding='utf-8').read(), encoding='utf-8')
    (tmp_path / 'tokenizer_config.json').write_text(json.dumps({'do_lower_case': False}))
    if fmt == 'bin':
        torch.save({'bert.' + k: v for k, v in sd.items()}, str(tmp_path / 'pytorch_model.bin'))
    else:
        st = pytest.importorskip('safetensors.torch')
        st.save_file(sd, str(tmp_path / 'model.safetensors'))
    enc = BT.BertTxtEncoder.from_pretrained(str(tmp_path), device='cpu')
    assert enc.tokenizer.do_lower_case is False and enc.tokenizer.max_length == 512
    assert torch.equal(enc.BertModel.encoder.layer[1].output.dense.weight, sd['encoder.layer.1.output.dense.weight'])
    with pytest.raises(FileNotFoundError):
        os.remove(str(tmp_path / ('pytorch_model.bin' if fmt == 'bin' else 'model.safetensors')))
        BT.BertTxtEncoder.from_pretrained(str(tmp_path), device='cpu')


def test_forward_returns_pre_extracted_features_without_encoding(golden, tok):
    enc = BT.BertTxtEncoder(tok, golden('bert_text').json('cfg'), device='cpu')
    feats = torch.ones(3, 128)
    assert enc({'caption': ['a', 'b', 'c'], 'bert_encoding': feats})['text_features'] is feats


def test_encoder_refuses_unsupported_configurations(golden, tok):
    base = golden('bert_text').json('cfg')
    for change, match in (({'hidden_act': 'relu'}, 'hidden_act'), ({'hidden_act': 'gelu_new'}, 'hidden_act'),
                          ({'position_embedding_type': 'relative_key'}, 'position_embedding_type'),
                          ({'num_attention_heads': 4}, 'head dim'), ({'hidden_size': 96, 'num_attention_heads': 1}, 'multiples of 64'),
                          ({'hidden_size': 1088, 'num_attention_heads': 17}, '1024'), ({'intermediate_size': 500}, 'intermediate_size'),
                          ({'max_position_embeddings': 513}, '512'), ({'is_decoder': True}, 'decoder'),
                          ({'add_cross_attention': True}, 'cross-attention'), ({'num_hidden_layers': 0}, 'layer')):
        with pytest.raises(NotImplementedError, match=match):
            BT.BertTxtEncoder(tok, dict(base, **change), device='cpu')
    with pytest.raises(NotImplementedError, match='precision'):
        BT.BertTxtEncoder(tok, base, precision='bf16', device='cpu')
    small = BT.BertTxtEncoder(tok, dict(base, vocab_size=100), device='cpu')
    with pytest.raises(ValueError, match='vocabulary'):
        small.batch(['a dog'])                                          # ids up to 376
    short = BT.BertTxtEncoder(tok, dict(base, max_position_embeddings=8), device='cpu')
    with pytest.raises(ValueError, match='positions'):
        short.batch(['the dog runs and jumps over the fence'])


def bert_model(width=128, heads=2, layers=2, inter=512, maxpos=512, eps=1e-12, blocks=True):
    from laff_amd import _lib
    fake = 4096                                                        # never dereferenced: every call below fails its checks first
    blk = (_lib.BertBlock * max(layers, 1))(*[_lib.BertBlock(*([fake] * 12)) for _ in range(max(layers, 1))])
    m = _lib.BertText(width, layers, heads, inter, maxpos, 377, eps, fake, fake, fake, fake, fake, blk if blocks else None, fake, fake)
    return m, blk


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.laff_bert_workspace_bytes(100, 10, 768, 3072, 0, C.byref(n)) == 0
    assert n.value == 100 * 768 * (4 + 4) + 100 * 3072 * 4 + 10 * 768 * 12       # big: max(12 W, 4 I) = 4 I bytes per row
    assert lib.laff_bert_workspace_bytes(100, 10, 768, 3072, 1, C.byref(n)) == 0
    assert n.value == 100 * 768 * (4 + 2 + 12) + 10 * 768 * 10                   # big: max(12 W, 2 I) = 12 W bytes per row
    assert lib.laff_bert_workspace_bytes(100, 10, 128, 2048, 1, C.byref(n)) == 0
    assert n.value == 100 * 128 * 6 + 100 * 2048 * 2 + 10 * 128 * 10               # big: 2 I > 12 W
    assert lib.laff_bert_workspace_bytes(100, 10, 768, 3072, 2, C.byref(n)) == -5 and b'precision' in lib.laff_last_error()
    assert lib.laff_bert_workspace_bytes(100, 10, 768, 3000, 0, C.byref(n)) == -5 and b'intermediate=3000' in lib.laff_last_error()
    assert lib.laff_bert_workspace_bytes(100, 10, 1088, 4096, 0, C.byref(n)) == -5 and b'width=1088' in lib.laff_last_error()
    assert lib.laff_bert_workspace_bytes(10, 11, 768, 3072, 0, C.byref(n)) == -1
    fake = C.c_void_p(4096)

    def enc(m=None, ro=(0, 3, 5), prec=0, ws_bytes=1 << 30, ldo=128, ids=fake, R=None):
        m = m if m is not None else bert_model()[0]
        roh = (C.c_int * len(ro))(*ro)
        return lib.laff_bert_encode(None, ids, fake, roh, len(ro) - 1, ro[-1] if R is None else R, C.byref(m), prec, fake, ldo, fake,
                                    ws_bytes)
    assert enc(m=bert_model(heads=4)[0]) == -5 and b'head dim' in lib.laff_last_error()
    assert enc(m=bert_model(width=1088, heads=17)[0]) == -5 and b'width=1088' in lib.laff_last_error()
    assert enc(m=bert_model(inter=500)[0]) == -5 and b'intermediate=500' in lib.laff_last_error()
    assert enc(m=bert_model(maxpos=513)[0]) == -5 and b'max_position=513' in lib.laff_last_error()
    assert enc(m=bert_model(layers=0)[0]) == -5 and b'layers=0' in lib.laff_last_error()
    assert enc(m=bert_model(eps=float('nan'))[0]) == -1 and b'layer_norm_eps' in lib.laff_last_error()
    assert enc(prec=7) == -1 and b'unknown precision' in lib.laff_last_error()
    assert enc(prec=3) == -5
    assert enc(ro=(1, 3, 5)) == -1 and b'row_off[0]' in lib.laff_last_error()
    assert enc(ro=(0, 3, 3)) == -1 and b'caption 1 has 0 rows' in lib.laff_last_error()
    assert enc(ro=(0, 513, 515)) == -1 and b'caption 0 has 513 rows' in lib.laff_last_error()
    assert enc(ro=(0, 3, 5), R=6) == -1 and b'row_off[N]=5 != R=6' in lib.laff_last_error()
    assert enc(ro=(0, 1 << 22, (1 << 22) + 1)) == -2 and b'4,194,304' in lib.laff_last_error()
    assert enc(ids=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(m=bert_model(blocks=False)[0]) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(ws_bytes=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert enc(ldo=64) == -2 and b'ldo' in lib.laff_last_error()
    assert enc() == -1 and b'null ctx' in lib.laff_last_error()        # valid arguments: only then the ctx
    assert enc(ro=(0,)) == 0                                            # the empty problem


def test_bert_entry_points_in_header_library_and_binding_at_the_header_abi():
    from laff_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert 'typedef struct laff_bert_text' in text and 'typedef struct laff_bert_block' in text
    assert C.sizeof(_lib.BertBlock) == 12 * 8 and C.sizeof(_lib.BertText) == 8 * 4 + 8 * 8


def test_bert_hip_kernels_have_no_spills_and_no_scratch(tmp_path):
    """Every bert_* kernel of bert.hip: 0 VGPR / SGPR spills, no scratch, MFMAs in the GEMMs and the attention only, no LDS in the
    attention (its footprint does not depend on the caption length)."""
    import subprocess
    import sys
    from laff_amd import build
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'bert.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'bert.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'bert_', quiet=True)
    # x2 precisions: 2 GEMM epilogues (erf-GELU, tanh), 3 row kernels (EMBED, ROW, CLS), 1 attention
    assert len(stats) == 12, sorted(stats)
    per_family = {f: sum(f in name for name in stats) for f in ('gemm_kernel', 'ln_kernel', 'attn_kernel')}
    assert per_family == {'gemm_kernel': 4, 'ln_kernel': 6, 'attn_kernel': 2}, per_family
    text = open(asm[0]).read()
    for name, st in stats.items():
        assert st['scratch'] == 0, (name, st)
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
        assert (st['mfma'] > 0) == ('gemm' in name or 'attn' in name), name
        if 'attn' in name:
            desc = text[text.index('.amdhsa_kernel ' + name):]
            assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', desc).group(1)) == 0, name
