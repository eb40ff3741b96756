"""The CLIP image encoder's host side, without a GPU: the float64 restatement against the reference's encode_image, the module's
state-dict handling and refusals, the C entry points' argument checks, the binding and the ISA of clip_image.hip's kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from clip_image_ref import encode_image64, fixture_config
from conftest import ROOT
from laff_amd import clip_image as CI


def test_float64_restatement_reproduces_the_reference(golden):
    z = golden('clip_image')
    assert z.json('configs') == ['c0', 'c1']
    for name, L, E in (('c0', 17, 64), ('c1', 5, 32)):
        cfg, sd, pix = fixture_config(z, name)
        assert (cfg['res'] // cfg['patch']) ** 2 + 1 == L == sd['visual.positional_embedding'].shape[0]
        got, want = encode_image64(pix, sd), z[name + '/encode_image']
        assert got.shape == want.shape == (cfg['frames'], E)
        assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert fixture_config(z, 'c1')[1]['visual.conv1.weight'].shape == (64, 3, 14, 14)   # 3 p^2 = 588: the padded-K path


def _full_sd(z, name):
    """The fixture's visual tower plus text keys and scalars a real CLIP checkpoint carries (ignored by the image encoder)."""
    sd = dict(fixture_config(z, name)[1])
    sd.update({'text_projection': np.zeros((64, 32), np.float32), 'positional_embedding': np.zeros((77, 64), np.float32),
               'token_embedding.weight': np.zeros((10, 64), np.float32), 'logit_scale': np.float32(4.6),
               'transformer.resblocks.0.attn.in_proj_weight': np.zeros((192, 64), np.float32), 'input_resolution': np.int64(224)})
    return sd


def test_from_state_dict_takes_the_three_key_prefixes(golden):
    z = golden('clip_image')
    vis = fixture_config(z, 'c0')[1]
    sd = _full_sd(z, 'c0')
    for src in (sd, {'ClipModel.' + k: v for k, v in sd.items()}, {'clip_model.ClipModel.' + k: v for k, v in sd.items()}):
        assert CI.ClipImageEncoder.dims(src) == (128, 2, 2, 8, 32, 64)
        enc = CI.ClipImageEncoder.from_state_dict(src, precision='fp32', device='cpu')
        assert (enc.width, enc.layers, enc.heads, enc.patch_size, enc.input_resolution, enc.embed_dim, enc.tokens) == \
            (128, 2, 2, 8, 32, 64, 17)
        got = enc.state_dict()
        assert torch.equal(got['ClipModel.visual.transformer.resblocks.1.mlp.c_fc.weight'],
                           torch.from_numpy(vis['visual.transformer.resblocks.1.mlp.c_fc.weight']))
    assert set(enc.state_dict()) == {'ClipModel.' + k for k in vis}
    assert CI.ClipImageEncoder.dims(_full_sd(z, 'c1')) == (64, 1, 1, 14, 28, 32)
    assert not any(isinstance(m, torch.nn.MultiheadAttention) for m in enc.modules())


def test_encoder_refuses_unsupported_checkpoints_and_configurations():
    rn = {'visual.layer1.0.conv1.weight': np.zeros((64, 64, 1, 1), np.float32),
          'visual.attnpool.positional_embedding': np.zeros((50, 2048), np.float32), 'text_projection': np.zeros((512, 1024))}
    with pytest.raises(NotImplementedError, match='RN50'):
        CI.ClipImageEncoder.dims(rn)
    with pytest.raises(NotImplementedError, match='RN50'):
        CI.ClipImageEncoder.from_state_dict({'ClipModel.' + k: v for k, v in rn.items()}, device='cpu')
    with pytest.raises(NotImplementedError, match='1024'):
        CI.ClipImageEncoder(1280, 1, 20, 14, 224, 1024, device='cpu')           # ViT-H/14's width
    with pytest.raises(NotImplementedError, match='head dim'):
        CI.ClipImageEncoder(128, 1, 4, 8, 32, 64, device='cpu')
    with pytest.raises(NotImplementedError, match='577'):
        CI.ClipImageEncoder(1024, 1, 16, 14, 336, 768, device='cpu')            # ViT-L/14@336
    with pytest.raises(NotImplementedError, match='multiple'):
        CI.ClipImageEncoder(64, 1, 1, 14, 30, 32, device='cpu')
    with pytest.raises(NotImplementedError, match='precision'):
        CI.ClipImageEncoder(64, 1, 1, 14, 28, 32, precision='bf16', device='cpu')
    with pytest.raises(Exception, match='frame_agg_method'):
        CI.ClipImageEncoder(64, 1, 1, 14, 28, 32, device='cpu')(None, (torch.zeros(1, 3, 28, 28),), frame_agg_method='max')
    for dims in ((768, 12, 12, 32, 224, 512), (768, 12, 12, 16, 224, 512), (1024, 24, 16, 14, 224, 768)):
        enc = CI.ClipImageEncoder(*dims, device='cpu')                           # ViT-B/32, B/16, L/14 are accepted
        assert enc.tokens == (224 // dims[3]) ** 2 + 1


def vit_model(width=128, heads=2, layers=2, res=32, patch=8, embed=64, blocks=True):
    from laff_amd import _lib
    fake = 4096                                                    # never dereferenced: every call below fails its checks first
    blk = (_lib.ClipBlock * max(layers, 1))(*[_lib.ClipBlock(*([fake] * 12)) for _ in range(max(layers, 1))])
    m = _lib.ClipVisual(width, layers, heads, embed, res, patch, fake, fake, fake, fake, fake, blk if blocks else None, fake, fake, fake)
    return m, blk


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    k = C.c_int()
    assert lib.laff_clip_image_kpad(14, 1, C.byref(k)) == 0 and k.value == 640
    assert lib.laff_clip_image_kpad(14, 0, C.byref(k)) == 0 and k.value == 608
    assert lib.laff_clip_image_kpad(32, 1, C.byref(k)) == 0 and k.value == 3072
    assert lib.laff_clip_image_kpad(8, 2, C.byref(k)) == -5
    n = C.c_size_t()
    assert lib.laff_clip_image_workspace_bytes(64, 768, 224, 32, 1, C.byref(n)) == 0
    R, np_ = 64 * 50, 64 * 49
    assert n.value >= R * 768 * (4 + 2 + 12) + 64 * 768 * 6 and n.value >= np_ * (3072 * 2 + 768 * 4)
    assert lib.laff_clip_image_workspace_bytes(64, 1088, 224, 32, 1, C.byref(n)) == -5 and b'width=1088' in lib.laff_last_error()
    assert lib.laff_clip_image_workspace_bytes(64, 1024, 336, 14, 1, C.byref(n)) == -5 and b'577 tokens' in lib.laff_last_error()
    assert lib.laff_clip_image_workspace_bytes(64, 768, 225, 32, 1, C.byref(n)) == -5 and b'multiple' in lib.laff_last_error()
    assert lib.laff_clip_image_workspace_bytes(-1, 768, 224, 32, 1, C.byref(n)) == -1
    assert lib.laff_clip_image_workspace_bytes(4, 768, 224, 32, 9, C.byref(n)) == -1 and b'unknown precision' in lib.laff_last_error()
    fake = C.c_void_p(4096)

    def enc(m=None, fo=(0, 3, 5), prec=1, ws_bytes=1 << 40, ldo=64, ldm=64, pix=fake, F=None, mean=fake):
        m = m if m is not None else vit_model()[0]
        V = len(fo) - 1
        foh = (C.c_int * len(fo))(*fo)
        return lib.laff_clip_image_encode(None, pix, fo[-1] if F is None else F, fake, foh, V, C.byref(m), prec, fake, ldo, mean, ldm,
                                          fake, ws_bytes)
    assert enc(m=vit_model(width=128, heads=4)[0]) == -5 and b'head dim' in lib.laff_last_error()
    assert enc(m=vit_model(width=1088, heads=17)[0]) == -5 and b'width=1088' in lib.laff_last_error()
    assert enc(m=vit_model(res=336, patch=14, width=1024, heads=16)[0]) == -5 and b'577 tokens' in lib.laff_last_error()
    assert enc(m=vit_model(res=30)[0]) == -5 and b'multiple of the patch size' in lib.laff_last_error()
    assert enc(m=vit_model(layers=0)[0]) == -5 and b'layers=0' in lib.laff_last_error()
    assert enc(prec=7) == -1 and b'unknown precision' in lib.laff_last_error()
    assert enc(prec=3) == -5
    assert enc(fo=(1, 3, 5)) == -1 and b'frame_off[0]' in lib.laff_last_error()
    assert enc(fo=(0, 3, 3)) == -1 and b'video 1 has 0 frames' in lib.laff_last_error()
    assert enc(fo=(0, 3, 5), F=6) == -1 and b'frame_off[V]=5 != F=6' in lib.laff_last_error()
    assert enc(pix=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(mean=None) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(m=vit_model(blocks=False)[0]) == -1 and b'null argument' in lib.laff_last_error()
    assert enc(ws_bytes=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert enc(ldo=32) == -2 and b'ldo' in lib.laff_last_error()
    assert enc(ldm=32) == -2 and b'ldm' in lib.laff_last_error()
    assert enc(fo=(0, 20000, 21291), m=vit_model(res=224, patch=16, width=768, heads=12)[0]) == -2 and b'token rows' in lib.laff_last_error()
    assert enc() == -1 and b'null ctx' in lib.laff_last_error()    # valid arguments: only then the ctx
    assert enc(fo=(0,), F=0) == 0                                    # the empty problem
    assert enc(fo=(0,), F=4) == -1 and b'null ctx' in lib.laff_last_error()   # frames without means (V = 0) are valid
    assert lib.laff_clip_pack_weight_padded(None, fake, 4, 588, 640, 2, fake) == -5
    assert lib.laff_clip_pack_weight_padded(None, fake, 4, 588, 587, 1, fake) == -2
    assert lib.laff_clip_pack_weight_padded(None, None, 4, 588, 640, 1, fake) == -1
    assert lib.laff_clip_pack_weight_padded(None, fake, 4, 588, 640, 1, fake) == -1 and b'null ctx' in lib.laff_last_error()


def test_image_entry_points_in_header_library_and_binding_at_the_header_abi():
    from laff_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert 'typedef struct laff_clip_visual' in text
    assert C.sizeof(_lib.ClipVisual) == 6 * 4 + 9 * 8


def test_clip_image_hip_kernels_have_no_spills_and_no_scratch(tmp_path):
    """Every vit_* kernel of clip_image.hip (the image-specific ones; the shared core is audited with clip.hip): 0 VGPR / SGPR
    spills and no scratch; MFMA exactly in the fp16 attention."""
    import subprocess
    import sys
    from laff_amd import build
    assert 'clip_image.hip' in build.SOURCES
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'debug'))
    import isa_audit
    src = os.path.join(build.CSRC, 'clip_image.hip')
    r = subprocess.run([build.hipcc()] + build.FLAGS + ['-save-temps=obj', '-c', src, '-o', str(tmp_path / 'clip_image.o')],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    asm = [str(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith('gfx950.s')]
    assert len(asm) == 1
    stats = isa_audit.audit(asm[0], 'vit_', quiet=True)
    # patch x2, fp16 attention x4 (key-tile classes), fp32 attention, mean (the LayerNorms and the pack moved to clip.hip's
    # clip_ln_kernel / clip_pack_kernel, audited by test_clip_host.py)
    assert len(stats) == 8, sorted(stats)
    assert not [name for name in stats if 'ln_kernel' in name or 'pack_kernel' in name], sorted(stats)
    text = open(asm[0]).read()
    for name, st in stats.items():
        assert st['scratch'] == 0, (name, st)
        meta = text[text.index('.name:           ' + name):]
        assert int(re.search(r'\.vgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.sgpr_spill_count: (\d+)', meta).group(1)) == 0, name
        assert int(re.search(r'\.private_segment_fixed_size: (\d+)', meta).group(1)) == 0, name
        assert (st['mfma'] > 0) == ('attn_f16' in name), name
