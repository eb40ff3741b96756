"""Times laff_fc_backward against torch's own autograd of act(F.linear(x, W, b)) on the same device, backward only -- what a user who
wants the gradients of a TransformNet projection has without the kernel.

    python tools/fc_backward_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back calls
after a warm-up, the median of 5 such windows.  Per shape (N, Dk, D) and per set of outputs (dW + db, the training call; and dX as well)
one JSON line:
    kernel_ms      laff_fc_backward through the C entry point with every buffer made beforehand
    op_ms          the same through ops.fc_backward, which allocates the outputs and the workspace per call
    torch_bwd_ms   torch.autograd.grad of tanh(F.linear(x, W, b)) with respect to W and b (and x); its forward is kept
    ratio          torch_bwd_ms / kernel_ms
    hbm_fraction   the mandatory bytes -- read dA, A, X, and W for dX; write the outputs -- over kernel_ms, as a fraction of HBM_PEAK
Before anything is timed both results are compared: the float64 formulas are evaluated on the device and the kernel has to stay within
the element-by-element bound of tests/test_gpu_fc_backward.py, (K + 4) 2^-24 sum |dA| |operand|; the two fp32 results may then differ by
twice that.  A miss ends the run with exit status 1 and no timing line for that shape.
"""
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 512, 4096), (128, 2048, 4096), (8192, 512, 512)]
HBM_PEAK = 8.0e12
U = 2.0 ** -24


def child(iters):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    for N, Dk, D in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(N + Dk + D)
        x = torch.randn(N, Dk, device=dev, generator=g)
        w = (torch.randn(D, Dk, device=dev, generator=g) / Dk ** 0.5).requires_grad_(True)
        b = (0.1 * torch.randn(D, device=dev, generator=g)).requires_grad_(True)
        dA = torch.randn(N, D, device=dev, generator=g)
        xt = x.clone().requires_grad_(True)
        A = torch.tanh(F.linear(xt, w, b))
        a, wd = A.detach(), w.detach()
        lib, ctx = ops._context(dev)
        chunks, nbytes, chunks_dx, _ = ops.fc_backward_plan(N, Dk, D)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        dx, dw, db = torch.empty(N, Dk, device=dev), torch.empty(D, Dk, device=dev), torch.empty(D, device=dev)
        # the float64 formulas and the bounds, on the device
        dz = dA.double() * (1.0 - a.double() ** 2)
        ref = {'dx': dz @ wd.double(), 'dw': dz.T @ x.double(), 'db': dz.sum(0)}
        bound = {'dx': (D + 4) * U * (dA.double().abs() @ wd.double().abs()), 'dw': (N + 4) * U * (dA.double().abs().T @ x.double().abs()),
                 'db': (N + 4) * U * dA.double().abs().sum(0)}
        del dz
        for with_dx in (False, True):
            raw = lambda: ops.check(lib.laff_fc_backward(ctx, ops._ptr(x), N, Dk, Dk, ops._ptr(wd), Dk, D, ops.ACT['tanh'], ops._ptr(a), D,
                                                         ops._ptr(dA), D, ops._ptr(dx) if with_dx else None, Dk, ops._ptr(dw), Dk,
                                                         ops._ptr(db), ops._ptr(ws), nbytes))      # noqa: E731
            leaves = [w, b] + ([xt] if with_dx else [])
            raw()
            theirs = dict(zip(('dw', 'db', 'dx'), torch.autograd.grad(A, leaves, dA, retain_graph=True)))
            used = {}
            for k, t in theirs.items():
                mine = {'dx': dx, 'dw': dw, 'db': db}[k]
                used[k] = float(((mine.double() - ref[k]).abs() / bound[k]).max())
                apart = float(((mine.double() - t.double()).abs() / bound[k]).max())
                if not (used[k] <= 1.0 and apart <= 2.0):
                    print('%s at %s: laff_fc_backward uses %.3g of its bound and lies %.3g bounds from torch autograd: nothing is timed'
                          % (k, (N, Dk, D), used[k], apart), file=sys.stderr)
                    return 1
            kernel_ms = median_ms(raw, iters)
            op_ms = median_ms(lambda: ops.fc_backward(x, wd, a, dA, 'tanh', want_dx=with_dx), iters)
            torch_bwd_ms = median_ms(lambda: torch.autograd.grad(A, leaves, dA, retain_graph=True), iters)
            mandatory = 4 * (2 * N * D + N * Dk + D * Dk + D + (D * Dk + N * Dk if with_dx else 0))
            print(json.dumps({'shape': [N, Dk, D], 'outputs': 'dW+db+dX' if with_dx else 'dW+db', 'chunks': chunks, 'chunks_dx': chunks_dx if with_dx else None,
                              'kernel_ms': round(kernel_ms, 4), 'op_ms': round(op_ms, 4), 'torch_bwd_ms': round(torch_bwd_ms, 4),
                              'ratio': round(torch_bwd_ms / kernel_ms, 2), 'mandatory_bytes': mandatory,
                              'hbm_fraction': round(mandatory / (kernel_ms * 1e-3) / HBM_PEAK, 3),
                              'largest_used_fraction_of_bound': {k: round(v, 4) for k, v in used.items()}}), flush=True)
        del A, ref, bound
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
