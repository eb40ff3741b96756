"""The CLIP text encoder's host side, without a GPU: captions -> ids (clip.tokenize rules), the ragged layout, the float64
restatement against the reference's encode_text, the module's state-dict handling and refusals, the C entry points' argument checks
and the ISA of clip.hip's kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from clip_ref import encode_text64, full_text_sd
from conftest import GOLDEN, ROOT
from laff_amd import clip_text as CT

BPE = os.path.join(GOLDEN, 'clip_bpe_subset.txt.gz')


@pytest.fixture(scope='module')
def tok():
    return CT.ClipTokenizer(BPE)


def test_tokenizer_reproduces_the_reference_ids(golden, tok):
    z = golden('clip_text')
    caps, want = z.json('captions'), z['ids']
    assert len(caps) >= 40 and tok.vocab_size == 49408 and (tok.sot, tok.eot) == (49406, 49407)
    got = tok.tokenize(caps)
    assert got.shape == want.shape == (len(caps), 77)
    for c, g, w in zip(caps, got, want):
        assert g.tolist() == w.tolist(), c
    last = want[-1]                                               # the caption above 77 tokens: cut, no <|endoftext|> kept
    assert last[-1] != 0 and 49407 not in last.tolist() and int(last.argmax()) < 76
    assert want[0].tolist()[:3] == [49406, 49407, 0]              # ''


def test_stdlib_pattern_gives_the_same_ids_on_ascii_captions(golden, tok):
    z = golden('clip_text')
    plain = CT.ClipTokenizer(BPE, use_regex=False)
    ascii_caps = [c for c in z.json('captions') if c.isascii()]
    assert len(ascii_caps) >= 35
    assert np.array_equal(plain.tokenize(ascii_caps), tok.tokenize(ascii_caps))


def test_ragged_layout(golden, tok):
    z = golden('clip_text')
    caps, dense = z.json('captions'), z['ids']
    b = tok.batch(caps)
    p = dense.argmax(axis=1)                                     # torch / numpy argmax: the first occurrence
    assert b.ids.dtype == np.int32 and b.row_off.dtype == np.int32
    assert b.row_off[0] == 0 and np.array_equal(np.diff(b.row_off), p + 1)
    assert b.ids.size == b.row_off[-1] == int((p + 1).sum())
    for i in range(len(caps)):
        assert b.ids[b.row_off[i]:b.row_off[i + 1]].tolist() == dense[i, :p[i] + 1].tolist()
    eot_early = caps.index('Hello <|endoftext|> world')           # a literal <|endoftext|>: pooled at its first occurrence
    assert p[eot_early] == 2 and (dense[eot_early] == 49407).sum() == 2
    assert p[-1] < 76 and p[0] == 1
    assert (p + 1).sum() < 0.5 * dense.size                       # the ragged rows are well under the 77-position work


def test_float64_restatement_reproduces_the_reference(golden):
    z = golden('clip_text')
    got = encode_text64(z['ids'], full_text_sd(z))
    want = z['encode_text']
    assert got.shape == want.shape == (len(z.json('captions')), 64)
    assert np.abs(got - want).max() <= 1e-5


def test_float64_restatement_agrees_on_the_ragged_rows(golden):
    """Cutting every caption after its pooled row and padding with zeros changes nothing: the causal mask at work."""
    z = golden('clip_text')
    ids = z['ids'].copy()
    p = ids.argmax(axis=1)
    for i in range(len(ids)):
        ids[i, p[i] + 1:] = 0
    sd = full_text_sd(z)
    assert np.abs(encode_text64(ids, sd) - encode_text64(z['ids'], sd)).max() <= 1e-12


def test_from_state_dict_infers_the_dimensions(golden, tok):
    z = golden('clip_text')
    sd = full_text_sd(z)
    extra = {'visual.conv1.weight': np.zeros((64, 3, 32, 32), np.float32), 'logit_scale': np.float32(4.6),
             'input_resolution': np.int64(224), 'context_length': np.int64(77), 'vocab_size': np.int64(49408)}
    for src in ({**sd, **extra}, {'ClipModel.' + k: v for k, v in {**sd, **extra}.items()}):
        assert CT.ClipTxtEncoder.dims(src) == (128, 2, 2, 64, 77, 49408)
        enc = CT.ClipTxtEncoder.from_state_dict(src, tok, precision='fp32', device='cpu')
        assert (enc.width, enc.layers, enc.heads, enc.embed_dim, enc.context_length, enc.vocab_size) == (128, 2, 2, 64, 77, 49408)
        got = enc.state_dict()
        assert torch.equal(got['ClipModel.transformer.resblocks.1.mlp.c_fc.weight'],
                           torch.from_numpy(sd['transformer.resblocks.1.mlp.c_fc.weight']))
    names = set(enc.state_dict())
    assert {'ClipModel.token_embedding.weight', 'ClipModel.positional_embedding', 'ClipModel.ln_final.weight',
            'ClipModel.text_projection', 'ClipModel.transformer.resblocks.0.attn.in_proj_weight',
            'ClipModel.transformer.resblocks.0.attn.out_proj.bias', 'ClipModel.transformer.resblocks.0.ln_2.bias'} <= names
    assert names == {'ClipModel.' + k for k in sd}
    assert not any(isinstance(m, torch.nn.MultiheadAttention) for m in enc.modules())


def test_forward_returns_pre_extracted_features_without_encoding(tok):
    enc = CT.ClipTxtEncoder(tok, 64, 1, 1, 32, device='cpu')
    feats = torch.ones(3, 32)
    assert enc({'caption': ['a', 'b', 'c'], 'CLIP_encoding': feats})['text_features'] is feats


def test_encoder_refuses_unsupported_configurations(tok):
    with pytest.raises(NotImplementedError, match='head dim'):
        CT.ClipTxtEncoder(tok, 128, 1, 4, 64, device='cpu')       # head dim 32
    with pytest.raises(NotImplementedError, match='1024'):
        CT.ClipTxtEncoder(tok, 1088, 1, 17, 64, device='cpu')
    with pytest.raises(NotImplementedError, match='multiples of 64'):
        CT.ClipTxtEncoder(tok, 96, 1, 1, 64, device='cpu')
    with pytest.raises(NotImplementedError, match='77'):
        CT.ClipTxtEncoder(tok, 128, 1, 2, 64, context_length=78, device='cpu')
    with pytest.raises(NotImplementedError, match='precision'):
        CT.ClipTxtEncoder(tok, 128, 1, 2, 64, precision='bf16', device='cpu')
    enc = CT.ClipTxtEncoder(tok, 64, 1, 1, 32, vocab_size=1000, device='cpu')
    with pytest.raises(ValueError, match='vocabulary'):
        enc.batch(['a dog'])                                       # BPE ids above 1000


def clip_model(width=128, heads=2, layers=2, ctx=77, embed=64, blocks=True):
    from laff_amd import _lib
    fake = 4096                                                    # never dereferenced: every call below fails its checks first
    blk = (_lib.ClipBlock * max(layers, 1))(*[_lib.ClipBlock(*([fake] * 12)) for _ in range(max(layers, 1))])
    m = _lib.ClipText(width, layers, heads, embed, ctx, 49408, fake, fake, blk if blocks else None, fake, fake, fake)
    return m, blk


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.laff_clip_workspace_bytes(100, 10, 512, 1, C.byref(n)) == 0
    assert n.value == 100 * 512 * 4 + 100 * 512 * 2 + 100 * 512 * 12
    assert lib.laff_clip_workspace_bytes(100, 10, 512, 0, C.byref(n)) == 0 and n.value == 100 * 512 * (4 + 4 + 16)
    assert lib.laff_clip_workspace_bytes(100, 10, 512, 2, C.byref(n)) == -5 and b'precision' in lib.laff_last_error()
    assert lib.laff_clip_workspace_bytes(100, 10, 512, 9, C.byref(n)) == -1 and b'unknown precision' in lib.laff_last_error()
    assert lib.laff_clip_workspace_bytes(100, 10, 1088, 1, C.byref(n)) == -5 and b'width=1088' in lib.laff_last_error()
    assert lib.laff_clip_workspace_bytes(10, 11, 512, 1, C.byref(n)) == -1
    fake = C.c_void_p(4096)

    def enc(m=None, ro=(0, 3, 5), prec=1, ws_bytes=1 << 30, ldo=64, ids=fake, R=None):
        m = m if m is not None else clip_model()[0]
        N = len(ro) - 1
        roh = (C.c_int * len(ro))(*ro)
        return lib.laff_clip_encode(None, ids, fake, roh, N, ro[-1] if R is None else R, C.byref(m), prec, fake, ldo, fake, ws_bytes)
    assert enc(m=clip_model(width=128, heads=4)[0]) == -5 and b'head dim' in lib.laff_last_error()
    assert enc(m=clip_model(width=1088, heads=17)[0]) == -5 and b'width=1088' in lib.laff_last_error()
    assert enc(m=clip_model(ctx=78)[0]) == -5 and b'context_length=78' in lib.laff_last_error()
    assert enc(m=clip_model(layers=0)[0]) == -5 and b'layers=0' in lib.laff_last_error()
    assert enc(prec=7) == -1 and b'unknown precision' in lib.laff_last_error()
    assert enc(prec=3) == -5
    assert enc(ro=(1, 3, 5)) == -1 and b'row_off[0]' in lib.laff_last_error()
    assert enc(ro=(0, 3, 3)) == -1 and b'caption 1 has 0 rows' in lib.laff_last_error()
    assert enc(ro=(0, 78, 80)) == -1 and b'caption 0 has 78 rows' in lib.laff_last_error()
    assert enc(ro=(0, 3, 5), R=6) == -1 and b'row_off[N]=5 != R=6' in lib.laff_last_error()
    assert enc(ids=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(m=clip_model(blocks=False)[0]) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(ws_bytes=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert enc(ldo=32) == -2 and b'ldo' in lib.laff_last_error()
    assert enc() == -1 and b'null ctx' in lib.laff_last_error()   # valid arguments: only then the ctx
    assert enc(ro=(0,)) == 0                                        # the empty problem
    assert lib.laff_clip_pack_weight(None, fake, 4, 4, 0, 2, fake) == -5
    assert lib.laff_clip_pack_weight(None, None, 4, 4, 0, 1, fake) == -1
    assert lib.laff_clip_pack_weight(None, fake, 4, 4, 0, 1, fake) == -1 and b'null ctx' in lib.laff_last_error()


def test_clip_entry_points_in_header_library_and_binding_at_the_header_abi():
    """The CLIP structs are in the header and the binding (the entry points and the ABI version: test_cabi.py, ENTRY_POINTS)."""
    from laff_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert 'typedef struct laff_clip_text' in text and 'typedef struct laff_clip_block' in text
    assert C.sizeof(_lib.ClipBlock) == 12 * 8 and C.sizeof(_lib.ClipText) == 6 * 4 + 6 * 8


def test_clip_hip_kernels_have_no_spills_and_no_scratch(tmp_path):
    """Every clip_* kernel of clip.hip, the transformer core both CLIP encoders share: 0 VGPR / SGPR spills and no scratch (the
    GEMM's staging registers and accumulators stay in registers; a struct-typed vector there once sent them to scratch and LDS)."""
    import subprocess
    import sys
    from laff_amd import build
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'clip.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'clip.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'clip_', quiet=True)
    # 6 GEMMs, 10 LayerNorms (x2 precisions: ROW, EMBED, POOL, and from clip_image.hip the image's ROW with its fp32 rounding and its
    # PATCH embed LayerNorm), 2 attention, 2 packs (the image's padded pack merged into clip_pack_kernel)
    assert len(stats) == 20, sorted(stats)
    per_family = {f: sum(f in name for name in stats) for f in ('gemm_kernel', 'ln_kernel', 'attn_kernel', 'pack_kernel')}
    assert per_family == {'gemm_kernel': 6, 'ln_kernel': 10, 'attn_kernel': 2, 'pack_kernel': 2}, per_family
    text = open(asm[0]).read()
    for name, st in stats.items():
        assert st['scratch'] == 0, (name, st)
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
        assert (st['mfma'] > 0) == ('gemm' in name), name
