#!/usr/bin/env python3
"""Golden vectors for the CLIP image encoder (tests/golden/clip_image.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden), builds the
reference's own clip.model.CLIP (its ViT branch: VisualTransformer) on CPU at two small visual configs with seeded parameters and
runs encode_image in fp32:
  c0: resolution 32, patch 8, width 128, 2 layers, embed 64 (L = 17 tokens, patch K = 192)
  c1: resolution 28, patch 14, width 64, 1 layer, embed 32 (L = 5, patch K = 588: the zero-padded K of ViT-L/14)
It writes arrays and JSON strings only, per config c:
  c/cfg (json), c/q/<name> int8 + c/e/<name> int8: every visual parameter as q * 2**e, |q| <= QMAX (per-tensor exponent),
  c/pix_q int8 + c/pix_e: the frames [F, 3, R, R] on the same kind of grid, c/encode_image [F, embed] fp32.
The parameters (at CLIP's init scales; LayerNorm affines and biases moved away from 1 / 0) and the frames are rounded to the grid
BEFORE the reference runs, so the stored values are exactly the ones encode_image saw.

    python tools/gen_golden_clip_image.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

QMAX = 31                                   # |q| of the stored grid: 6 bits of each drawn value
CONFIGS = {'c0': dict(res=32, patch=8, width=128, layers=2, embed=64, frames=6),
           'c1': dict(res=28, patch=14, width=64, layers=1, embed=32, frames=4)}


def to_grid(t):
    e = int(np.ceil(np.log2(float(t.abs().max()) / QMAX)))
    q = torch.clamp(torch.round(t / 2.0 ** e), -QMAX, QMAX)
    return q * 2.0 ** e, q.numpy().astype(np.int8), np.int8(e)


def main():
    from model.clip import model as cm
    arrays = {}
    for ci, (name, c) in enumerate(sorted(CONFIGS.items())):
        g = G.rng(9100 + ci)
        torch.manual_seed(9100 + ci)
        # CLIP(embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
        #      transformer_width, transformer_heads, transformer_layers): an int vision_layers takes the ViT branch
        clip = cm.CLIP(c['embed'], c['res'], c['layers'], c['width'], c['patch'], 8, 64, 64, 1, 1).eval()
        assert isinstance(clip.visual, cm.VisualTransformer)
        with torch.no_grad():
            for n, p in clip.visual.named_parameters():
                if n.endswith('bias'):
                    p.copy_(torch.from_numpy(G.f32(g.normal(0, 0.05, p.shape))))
                elif ('.ln_' in '.' + n or n.startswith('ln_')) and n.endswith('weight'):
                    p.copy_(torch.from_numpy(G.f32(1 + g.normal(0, 0.1, p.shape))))
            for n, p in clip.visual.named_parameters():
                v, q, e = to_grid(p)
                p.copy_(v)
                arrays['%s/q/visual.%s' % (name, n)] = q
                arrays['%s/e/visual.%s' % (name, n)] = e
            pix = torch.from_numpy(G.f32(g.normal(0, 1, (c['frames'], 3, c['res'], c['res']))))
            pix, pq, pe = to_grid(pix)
            out = clip.encode_image(pix).numpy().astype(np.float32)
        arrays[name + '/pix_q'] = pq
        arrays[name + '/pix_e'] = pe
        arrays[name + '/encode_image'] = out
        arrays[name + '/cfg'] = np.array(json.dumps(c))
    arrays['configs'] = np.array(json.dumps(sorted(CONFIGS)))
    G.save('clip_image', **arrays)


if __name__ == '__main__':
    main()
