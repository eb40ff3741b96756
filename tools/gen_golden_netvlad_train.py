#!/usr/bin/env python3
"""Golden vectors for the NetVLAD backward (tests/golden/netvlad_train.npz), from the REAL reference.

Runs only in the build container: it reuses gen_golden.import_reference() (the stub recipe, by importing gen_golden) and runs the
reference's own NetVLAD module (model/Attention.py:862-913) forward and backward under CPU autograd, once in float64 and once in
float32 from the same float32 values of the parameters, the rows and d_out.  The module level is all the reference can give: its
full model with NetVLAD on does not construct (see MultiScaleTxtEncoder's docstring).  Arrays only.

    python tools/gen_golden_netvlad_train.py
"""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402  (imports the reference with its stubs)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (K, D, rows per caption; 0: a caption of all-zero rows, here 2 of them)
CASES = [(5, 20, (1, 3, 17, 0, 8, 9)), (8, 20, (9, 1, 0, 16, 2)), (5, 300, (4, 0, 1, 11)), (8, 300, (2, 17, 0, 5))]
ZERO_ROWS = 2


def run(dtype, K, D, rows, fc1, cent, dout):
    with contextlib.redirect_stdout(io.StringIO()):
        nv = G.ref_att.NetVLAD(D, K)
    nv.to(dtype)
    with torch.no_grad():
        nv.fc1.weight.copy_(torch.from_numpy(fc1))
        nv.centeroids.copy_(torch.from_numpy(cent))
    with torch.enable_grad():
        out = nv([torch.from_numpy(x).to(dtype) for x in rows])
        out.backward(torch.from_numpy(dout).to(dtype))
    return out.detach().numpy(), nv.fc1.weight.grad.numpy(), nv.centeroids.grad.numpy()


def main():
    g = G.rng(2828)
    arrays = {}
    for c, (K, D, lens) in enumerate(CASES):
        rows = [G.f32(g.normal(0, 1, (m, D))) if m else np.zeros((ZERO_ROWS, D), np.float32) for m in lens]
        fc1 = G.f32(g.normal(0, 1.0 / np.sqrt(D), (K, D)))
        cent = G.f32(g.normal(0, 1.0 / np.sqrt(D), (K, D)))
        dout = G.f32(g.normal(0, 1, (len(lens), K * D)))
        p = 'c%d/' % c
        arrays.update({p + 'rows': np.concatenate(rows), p + 'lens': np.array([len(x) for x in rows], np.int32),
                       p + 'zero': np.array([m == 0 for m in lens]), p + 'fc1': fc1, p + 'cent': cent, p + 'dout': dout})
        for tag, dtype in (('f64', torch.float64), ('f32', torch.float32)):
            out, dfc1, dcent = run(dtype, K, D, rows, fc1, cent, dout)
            assert out.dtype == (np.float64 if tag == 'f64' else np.float32)
            arrays.update({p + tag + '/out': out, p + tag + '/fc1.weight': dfc1, p + tag + '/centeroids': dcent})
    G.save('netvlad_train', **arrays)


if __name__ == '__main__':
    main()
