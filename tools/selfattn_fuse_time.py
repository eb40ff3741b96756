"""Times laff_selfattn_fuse and laff_selfattn_fuse_backward (output type 'mean') against a torch restatement of the block on the same
device, and at the inference shape against laff_fuse on the same planes, the HBM-bound yardstick.

    python tools/selfattn_fuse_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back calls
after a warm-up, the median of 5 such windows.  Per shape (N, L, H, d) one JSON line:
    fwd_ms, bwd_ms       the two entry points, called through the C ABI with every buffer made beforehand (backward: dx of every plane,
                         dgamma and dbeta; both launches); planes and gradients are the slices of stacked (N, L, H d) tensors
    torch_fwd_ms         the block in torch ops, forward
    torch_bwd_ms         torch.autograd.grad of it with respect to the planes, gamma and beta (backward only; its forward is kept)
    laff_fuse_ms         laff_fuse (with_ave, mul) on the same planes: reads the same L planes once, writes one row per (n, h)
    fwd_hbm_fraction     (L + 1) N H d 4 bytes over fwd_ms, as a fraction of HBM_PEAK (8 TB/s); bwd: (2 L + 1) N H d 4 bytes
Before torch is timed the kernel's E, dx and dgamma are compared with torch's; a difference above AGREE of the largest entry ends the
run with exit status 1 and no timing line for that shape.  There is no pass / fail threshold on the times.
"""
import ctypes as C
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [('LAFF training', 128, 4, 8, 512), ('C4 inference', 40000, 4, 8, 512)]
HBM_PEAK = 8.0e12
AGREE = 1e-5          # both sides are fp32 with errors near 1e-6 of the largest entry (tests/test_gpu_selfattn_fuse.py); ten times that


def _torch_block(x, gamma, beta, H, d):
    """Multi_head_MyApply_selfAttention(output_type='mean') on x (N, L, H, d) in torch ops."""
    import torch
    t = x.permute(0, 2, 1, 3)
    A = torch.softmax((d // H) ** -0.5 * t @ t.transpose(2, 3), dim=3)
    o = torch.nn.functional.layer_norm(A @ t + t, (d,), gamma, beta, 1e-5)
    return o.mean(2)


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import _lib, ops
    dev = torch.device('cuda')
    K = _lib.K
    for name, N, L, H, d in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(N + L + H + d)
        x = torch.randn(N, L, H * d, device=dev, generator=g)
        gamma, beta = 0.5 + torch.rand(d, device=dev, generator=g), 0.3 * torch.randn(d, device=dev, generator=g)
        dE = torch.randn(N, H, d, device=dev, generator=g)
        planes = [x[:, l, :] for l in range(L)]
        E, dxs = torch.empty(N, H, d, device=dev), torch.empty_like(x)
        dg, db = torch.empty(d, device=dev), torch.empty(d, device=dev)
        lib, ctx = ops._context(dev)
        nbytes = ops.selfattn_fuse_backward_plan(N, H, d)[0]
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        xp = (C.c_void_p * L)(*[t.data_ptr() for t in planes])
        dp = (C.c_void_p * L)(*[dxs[:, l, :].data_ptr() for l in range(L)])
        ld = (C.c_int * L)(*[L * H * d] * L)
        mode = (K['LAFF_SA_PREPEND_NONE'], K['LAFF_SA_POOL_MEAN'], 0, 0)
        fwd = lambda: ops.check(lib.laff_selfattn_fuse(ctx, xp, ld, L, N, H, d, ops._ptr(gamma), ops._ptr(beta), *mode, ops._ptr(E), H * d,  # noqa: E731
                                                       None, 0, 0))
        bwd = lambda: ops.check(lib.laff_selfattn_fuse_backward(ctx, xp, ld, L, N, H, d, ops._ptr(gamma), ops._ptr(beta), *mode,  # noqa: E731
                                                                ops._ptr(dE), H * d, None, 0, 0, dp, ld, ops._ptr(dg), ops._ptr(db),
                                                                ops._ptr(ws), nbytes))
        fwd_ms, bwd_ms = median_ms(fwd, iters), median_ms(bwd, iters)
        w, b, gw = torch.randn(H, d, device=dev, generator=g) / d ** 0.5, torch.zeros(H, device=dev), torch.ones(H, device=dev)
        Ef = torch.empty(N, H, d, device=dev)
        tuples = [(t, False, None, None) for t in planes]
        fuse_ms = median_ms(lambda: ops.fuse(tuples, H, d, w, b, gw, ops.attention_flags(with_ave=True, mul=True), out=Ef), iters)
        # the same numbers from both sides, before any is trusted
        fwd()
        bwd()
        xt, gt, bt = x.view(N, L, H, d).clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        Et = _torch_block(xt, gt, bt, H, d)
        gx, gg, _ = torch.autograd.grad(Et, [xt, gt, bt], dE, retain_graph=True)
        agree = max(float((Et - E).abs().max() / Et.abs().max()), float((gx.reshape(N, L, H * d) - dxs).abs().max() / gx.abs().max()),
                    float((gg - dg).abs().max() / gg.abs().max()))
        if not agree <= AGREE:
            print('laff_selfattn_fuse and torch differ by %.3g (relative to the largest entry) at %s: nothing is timed'
                  % (agree, (N, L, H, d)), file=sys.stderr)
            return 1
        k = max(iters // 4, 2)
        torch_bwd_ms = median_ms(lambda: torch.autograd.grad(Et, [xt, gt, bt], dE, retain_graph=True), k)
        with torch.no_grad():
            torch_fwd_ms = median_ms(lambda: _torch_block(xt, gt, bt, H, d), k)
        unit = N * H * d * 4
        print(json.dumps({'shape': [N, L, H, d], 'name': name, 'fwd_ms': round(fwd_ms, 4), 'bwd_ms': round(bwd_ms, 4),
                          'fwd_plus_bwd_ms': round(fwd_ms + bwd_ms, 4), 'torch_fwd_ms': round(torch_fwd_ms, 4),
                          'torch_bwd_ms': round(torch_bwd_ms, 4), 'torch_fwd_plus_bwd_ms': round(torch_fwd_ms + torch_bwd_ms, 4),
                          'laff_fuse_ms': round(fuse_ms, 4), 'fwd_hbm_fraction': round((L + 1) * unit / (fwd_ms * 1e-3) / HBM_PEAK, 3),
                          'bwd_hbm_fraction': round((2 * L + 1) * unit / (bwd_ms * 1e-3) / HBM_PEAK, 3),
                          'max_rel_difference_to_torch': agree}), flush=True)
        del Et, gx, gg, xt
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
