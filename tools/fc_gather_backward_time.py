"""Times laff_fc_gather_backward against the only route there was before it -- densify the counts and run laff_fc_backward -- and against a
hipMemsetAsync of dW's bytes, the floor of a kernel that has to write them.

    python tools/fc_gather_backward_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back calls
after a warm-up, the median of 5 such windows.  Per shape (N, Dk, D), a batch of N captions of about 10 words whose ids follow a 1 / rank
law, tanh, dW + db, one JSON line:
    kernel_ms            laff_fc_gather_backward through the C entry point with every buffer made beforehand
    op_ms                the same through ops.fc_gather_backward, which allocates the outputs per call
    dense_ms             laff_fc_backward (dW + db) on the densified input, the densification not counted
    densify_dense_ms     the same with x.to_dense() in front of every call
    memset_ms            hipMemsetAsync of the 4 D Dk bytes of dW
    weight_t_ms          fc1.weight.t().contiguous(), which TransformNet.weight_t() re-forms after every optimizer step
    csr_transpose_ms     ops.csr_transpose of the device CSR, what a step pays without BoWTxtEncoder(with_csc=True)
    hbm_fraction         4 D Dk bytes over kernel_ms, as a fraction of HBM_PEAK
Before anything is timed the new call and the densified route are held to the element-by-element bound of
tests/test_gpu_fc_gather_backward.py, (N + 4) 2^-24 |dA|^T |X| (and sum |dA| for db), against the float64 formulas evaluated on the
device.  A miss ends the run with exit status 1 and no timing line for that shape.
"""
import ctypes
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 10000, 2048), (128, 7811, 4096)]
HBM_PEAK = 8.0e12
U = 2.0 ** -24
TV = 64


def child(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    hip = ctypes.CDLL('libamdhip64.so')
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    for N, Dk, D in SHAPES:
        rng = np.random.default_rng(N + Dk + D)
        rows = [np.unique((Dk ** rng.random(10)).astype(np.int64) - 1) for _ in range(N)]
        crow = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
        col = np.concatenate(rows).astype(np.int32)
        host = torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.ones(len(col)), size=(N, Dk))
        x_csr = host.to(dev)
        colptr, rws, vals = (t.to(dev) for t in ops.csr_transpose(host))
        ptr = colptr.cpu().numpy()
        empty = sum(1 for v0 in range(0, Dk, TV) if ptr[min(v0 + TV, Dk)] == ptr[v0])
        g = torch.Generator(device='cuda').manual_seed(N + Dk + D)
        a = torch.tanh(3.0 * torch.randn(N, D, device=dev, generator=g))
        dA = torch.randn(N, D, device=dev, generator=g)
        w = torch.randn(D, Dk, device=dev, generator=g)
        x = x_csr.to_dense()
        dw, db = torch.empty(D, Dk, device=dev), torch.empty(D, device=dev)
        dw2, db2 = torch.empty(D, Dk, device=dev), torch.empty(D, device=dev)
        lib, ctx = ops._context(dev)
        raw = lambda: ops.check(lib.laff_fc_gather_backward(ctx, ops._ptr(colptr), ops._ptr(rws), ops._ptr(vals), rws.numel(), N, Dk, D,    # noqa: E731
                                                            ops.ACT['tanh'], ops._ptr(a), D, ops._ptr(dA), D, ops._ptr(dw), Dk, ops._ptr(db)))
        dense = lambda: ops.fc_backward(x, w, a, dA, 'tanh', want_dx=False, out=(None, dw2, db2))      # noqa: E731
        raw()
        dense()
        dz = dA.double() * (1.0 - a.double() ** 2)
        ref = {'dw': dz.T @ x.double(), 'db': dz.sum(0)}
        bound = {'dw': (N + 4) * U * (dA.double().abs().T @ x.double()), 'db': (N + 4) * U * dA.double().abs().sum(0)}
        del dz
        used = {}
        for route, outs in (('gather', {'dw': dw, 'db': db}), ('dense', {'dw': dw2, 'db': db2})):
            for k, t in outs.items():
                err = (t.double() - ref[k]).abs()
                ok = bool((err <= bound[k]).all())
                used[route + '_' + k] = float((err / bound[k].clamp_min(1e-300)).max())
                if not ok:
                    print('%s of the %s route at %s leaves its bound: nothing is timed' % (k, route, (N, Dk, D)), file=sys.stderr)
                    return 1
        del ref, bound
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nbytes = 4 * D * Dk

        def memset():
            if hip.hipMemsetAsync(dw.data_ptr(), 0, nbytes, stream):
                raise RuntimeError('hipMemsetAsync failed')
        kernel_ms = median_ms(raw, iters)
        res = {'shape': [N, Dk, D], 'nnz': int(rws.numel()), 'empty_tiles': '%d of %d' % (empty, (Dk + TV - 1) // TV),
               'kernel_ms': round(kernel_ms, 4),
               'op_ms': round(median_ms(lambda: ops.fc_gather_backward((colptr, rws, vals), N, Dk, a, dA, 'tanh'), iters), 4),
               'dense_ms': round(median_ms(dense, iters), 4),
               'densify_dense_ms': round(median_ms(lambda: ops.fc_backward(x_csr.to_dense(), w, a, dA, 'tanh', want_dx=False,
                                                                          out=(None, dw2, db2)), iters), 4),
               'memset_ms': round(median_ms(memset, iters), 4),
               'weight_t_ms': round(median_ms(lambda: w.t().contiguous(), iters), 4),
               'csr_transpose_ms': round(median_ms(lambda: ops.csr_transpose(x_csr), iters), 4),
               'dw_bytes': nbytes, 'hbm_fraction': round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK, 3),
               'largest_used_fraction_of_bound': {k: round(v, 4) for k, v in used.items()}}
        print(json.dumps(res), flush=True)
        del x, w, dw, dw2
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
