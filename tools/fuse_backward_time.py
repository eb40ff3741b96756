"""Times laff_fuse_backward against torch's own autograd of the same block built from torch ops on the same device -- what a user who
wants gradients through the fusion has without the kernel.

    python tools/fuse_backward_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back calls
after a warm-up, the median of 5 such windows.  Per shape (N, L, H, d) one JSON line:
    kernel_ms      laff_fuse_backward (dx, dw, db; both launches), planes and gradients as the slices of stacked (N, L, H d) tensors,
                   called through the C entry point with every buffer made beforehand
    op_ms          the same through ops.fuse_backward, which allocates dw, db and the workspace per call (host-bound for short launches)
    torch_bwd_ms   torch.autograd.grad of the block's output with respect to the planes, w and b (backward only; its forward is kept)
    torch_fwd_ms   the block's forward in torch ops, for scale
    ratio          torch_bwd_ms / kernel_ms
    hbm_fraction   (2 L + 1) N H d 4 bytes, the launch's mandatory traffic, over kernel_ms, as a fraction of HBM_PEAK (8 TB/s)
Before torch is timed, dx and dw of the kernel are compared with torch's; a difference above AGREE of the largest entry ends the run with
exit status 1 and no timing line for that shape.
"""
import ctypes as C
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8192, 4, 8, 512), (8192, 4, 1, 512)]
HBM_PEAK = 8.0e12
AGREE = 1e-5          # both sides are fp32 with errors near 1e-6 of the largest entry (tests/test_gpu_fuse_backward.py); ten times that


def _torch_block(x, w, b, gw, L):
    """Multi_head_MyApply_Attention(with_ave=True, mul=True) on x (N, L, H, d) in torch ops, as the reference writes it."""
    s = x.sum(1)
    c = x * (s / L)[:, None]
    a = (c * w[None, None]).sum(3).add(b[None, None]).softmax(1)                 # (N, L, H)
    g = (a[..., None] * x).sum(1) + gw[None, :, None] * s
    return g / (g.pow(2).sum(2, keepdim=True).sqrt() + 1e-14)


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    flags = ops.attention_flags(with_ave=True, mul=True)
    for N, L, H, d in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(N + L + H + d)
        x = 0.5 * torch.randn(N, L, H * d, device=dev, generator=g)
        w = torch.randn(H, d, device=dev, generator=g) / d ** 0.5
        b = 0.1 * torch.randn(H, device=dev, generator=g)
        gw = torch.ones(H, device=dev)
        dE = torch.randn(N, H, d, device=dev, generator=g)
        planes = [x[:, l, :] for l in range(L)]
        dxs = torch.empty_like(x)
        out = [dxs[:, l, :] for l in range(L)]
        # the C entry point itself with every buffer made beforehand: the op's host work per call (allocations, argument arrays) is as long
        # as the H = 1 launch and would be what the events see
        lib, ctx = ops._context(dev)
        nbytes = ops._size_query('laff_fuse_backward_workspace_bytes', L, N, H, d, flags)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        dw, db = torch.empty(H, d, device=dev), torch.empty(H, device=dev)
        xp, dp = (C.c_void_p * L)(*[t.data_ptr() for t in planes]), (C.c_void_p * L)(*[t.data_ptr() for t in out])
        ld = (C.c_int * L)(*[L * H * d] * L)
        raw = lambda: ops.check(lib.laff_fuse_backward(ctx, xp, ld, L, N, H, d, ops._ptr(w), ops._ptr(b), ops._ptr(gw), flags, ops._ptr(dE),
                                                       H * d, dp, ld, ops._ptr(dw), ops._ptr(db), ops._ptr(ws), nbytes))      # noqa: E731
        kernel_ms = median_ms(raw, iters)
        op_ms = median_ms(lambda: ops.fuse_backward(planes, H, d, w, b, gw, flags, dE, out=out), iters)
        # the same numbers from both sides, before any is trusted
        raw()
        xt, wt, bt = x.view(N, L, H, d).clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        E = _torch_block(xt, wt, bt, gw, L)
        gx, gwt, _ = torch.autograd.grad(E, [xt, wt, bt], dE, retain_graph=True)
        agree = max(float((gx.reshape(N, L, H * d) - dxs).abs().max() / gx.abs().max()), float((gwt - dw).abs().max() / gwt.abs().max()))
        if not agree <= AGREE:
            print('laff_fuse_backward and torch autograd differ by %.3g (relative to the largest entry) at %s: nothing is timed'
                  % (agree, (N, L, H, d)), file=sys.stderr)
            return 1
        torch_bwd_ms = median_ms(lambda: torch.autograd.grad(E, [xt, wt, bt], dE, retain_graph=True), max(iters // 4, 2))
        with torch.no_grad():
            torch_fwd_ms = median_ms(lambda: _torch_block(xt, wt, bt, gw, L), max(iters // 4, 2))
        nbytes = (2 * L + 1) * N * H * d * 4
        print(json.dumps({'shape': [N, L, H, d], 'kernel_ms': round(kernel_ms, 4), 'torch_bwd_ms': round(torch_bwd_ms, 4),
                          'torch_fwd_ms': round(torch_fwd_ms, 4), 'op_ms': round(op_ms, 4), 'ratio': round(torch_bwd_ms / kernel_ms, 2),
                          'mandatory_bytes': nbytes, 'hbm_fraction': round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK, 3),
                          'max_rel_difference_to_torch': agree}), flush=True)
        del E, gx, gwt, xt
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
