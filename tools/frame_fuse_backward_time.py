"""Times laff_frame_fuse_backward against torch's own autograd of the same block built from torch ops on the same device -- what a user
who wants gradients through the frame attention has without the kernel.

    python tools/frame_fuse_backward_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Per (B, Fmax, d), mul setting and feature count
(with_ave on, lens uniform in [1, Fmax]) the tool FIRST holds both sides to float64 -- the same block in float64 torch on the device --
with the error measure and the bound of tests/test_gpu_frame_fuse_backward.py: max |x - float64| / max |float64| of dframes and of dw
within max(4 e32, 1.5e-6) for the kernel, e32 being the error of float32 CPU autograd of the block on the first feature, and within twice
that for torch's float32 backward on the device.  A shape that misses either ends the run with exit status 1 and is not timed.
Times are HIP events around K back-to-back calls after a warm-up, the median of 5 such windows.  One JSON line per case:
    kernel_ms      laff_frame_fuse_backward (dframes, dw, db; both launches) through the C entry point, every buffer made beforehand
    op_ms          the same through ops.frame_fuse_backward, which allocates the outputs and the workspace per call
    torch_bwd_ms   torch.autograd.grad of the block's output with respect to the frames, w and b, once per feature (backward only)
    torch_fwd_ms   the block's forward in torch ops, for scale
    ratio          torch_bwd_ms / kernel_ms (below 1: torch wins, and `torch_wins` says so)
    mandatory_bytes  sum over the videos of (2 len d + d) 4: the frames read once, their gradient written once, dV read
    hbm_fraction   mandatory_bytes over kernel_ms, as a fraction of HBM_PEAK (8 TB/s)
"""
import ctypes as C
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 50, 512), (128, 200, 1024), (3000, 32, 512)]
COUNTS = (1, 4)
HBM_PEAK = 8.0e12
TOL_UNIT = 1.5e-6


def _torch_block(x, keep, w, b, gw, mul):
    """Attention_1(with_ave=True, mul) over the frames of every video, x (B, Fmax, d), keep (B, Fmax, 1) the mask of the real frames."""
    xm = x * keep
    s = xm.sum(1)
    ws = w[None] * s / x.shape[1] if mul else w[None]
    a = ((xm * ws[:, None]).sum(2) + b).softmax(1)
    g = (a[..., None] * xm).sum(1) + gw * s
    return g / (g.pow(2).sum(1, keepdim=True).sqrt() + 1e-14)


def _grads(x, keep, w, b, gw, dV, mul, dtype, device):
    import torch
    xt = x.to(device=device, dtype=dtype).requires_grad_(True)
    wt = w.to(device=device, dtype=dtype).requires_grad_(True)
    bt = b.to(device=device, dtype=dtype).requires_grad_(True)
    V = _torch_block(xt, keep.to(device=device, dtype=dtype), wt, bt, gw.to(device=device, dtype=dtype), mul)
    gx, gw_, _ = torch.autograd.grad(V, [xt, wt, bt], dV.to(device=device, dtype=dtype))
    return gx, gw_


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    status = 0
    for (B, Fmax, d), mul in [(s, m) for s in SHAPES for m in (False, True)]:
        flags = ops.attention_flags(with_ave=True, mul=mul)
        g = torch.Generator(device='cuda').manual_seed(B + Fmax + d + mul)
        n = max(COUNTS)
        xs = [0.5 * torch.randn(B, Fmax, d, device=dev, generator=g) for _ in range(n)]
        ws = [torch.randn(d, device=dev, generator=g) / d ** 0.5 for _ in range(n)]
        bs = [0.1 * torch.randn(1, device=dev, generator=g) for _ in range(n)]
        gws = [torch.ones(1, device=dev) for _ in range(n)]
        dVs = [torch.randn(B, d, device=dev, generator=g) for _ in range(n)]
        lens = torch.randint(1, Fmax + 1, (B,), device=dev, generator=g).to(torch.int32)
        keep = (torch.arange(Fmax, device=dev)[None, :] < lens[:, None])[:, :, None]
        dfs = [torch.empty_like(x) for x in xs]
        dws, dbs = [torch.empty(d, device=dev) for _ in range(n)], [torch.empty(1, device=dev) for _ in range(n)]
        lib, ctx = ops._context(dev)

        def tab(ts, k):
            return (C.c_void_p * k)(*[t.data_ptr() for t in ts[:k]])

        def raw_call(k):
            nbytes = ops.frame_fuse_backward_plan(k, B, Fmax, d)[0]
            wsp = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            t = [tab(v, k) for v in (xs, ws, bs, gws, dVs, dfs, dws, dbs)]
            return lambda: ops.check(lib.laff_frame_fuse_backward(ctx, k, t[0], ops._ptr(lens), B, Fmax, d, t[1], t[2], t[3], flags, t[4], d,
                                                                  t[5], t[6], t[7], ops._ptr(wsp), nbytes)), wsp
        # both sides against float64 before anything is timed
        raw, wsp = raw_call(n)
        raw()
        torch.cuda.synchronize()
        x0 = [t.cpu() for t in (xs[0], keep, ws[0], bs[0], gws[0], dVs[0])]
        r64 = _grads(xs[0], keep, ws[0], bs[0], gws[0], dVs[0], mul, torch.float64, dev)
        c32 = _grads(*x0, mul, torch.float32, 'cpu')
        e32 = (_rel(c32[0], r64[0].cpu()), _rel(c32[1], r64[1].cpu()))
        bound = (max(4.0 * e32[0], TOL_UNIT), max(4.0 * e32[1], TOL_UNIT))
        del c32, x0
        e_k, e_t = [0.0, 0.0], [0.0, 0.0]
        for i in range(n):
            if i:
                r64 = _grads(xs[i], keep, ws[i], bs[i], gws[i], dVs[i], mul, torch.float64, dev)
            t32 = _grads(xs[i], keep, ws[i], bs[i], gws[i], dVs[i], mul, torch.float32, dev)
            for j, (got, tor) in enumerate(((dfs[i], t32[0]), (dws[i], t32[1]))):
                e_k[j], e_t[j] = max(e_k[j], _rel(got, r64[j])), max(e_t[j], _rel(tor, r64[j]))
            del t32
        del r64
        ok = all(e_k[j] <= bound[j] and e_t[j] <= 2.0 * bound[j] for j in (0, 1)) and not any(float(t.abs().max()) for t in dbs)
        if not ok:
            print('not timed at %s mul=%d: against float64 the kernel is at dx %.3g dw %.3g (bounds %.3g, %.3g), torch at dx %.3g dw %.3g '
                  '(bounds twice those)' % ((B, Fmax, d), mul, e_k[0], e_k[1], bound[0], bound[1], e_t[0], e_t[1]), file=sys.stderr)
            status = 1
            continue
        mandatory = int((2 * lens.sum().item() * d + B * d) * 4)
        for k in COUNTS:
            raw, wsp = raw_call(k)
            kernel_ms = median_ms(raw, iters)
            op_ms = median_ms(lambda: ops.frame_fuse_backward(xs[:k], lens, list(zip(ws, bs, gws))[:k], flags, dVs[:k]), iters)
            leaves = [(xs[i].clone().requires_grad_(True), ws[i].clone().requires_grad_(True), bs[i].clone().requires_grad_(True))
                      for i in range(k)]
            Vs = [_torch_block(x, keep, w, b, gws[i], mul) for i, (x, w, b) in enumerate(leaves)]

            def torch_bwd():
                for i in range(k):
                    torch.autograd.grad(Vs[i], list(leaves[i]), dVs[i], retain_graph=True)
            torch_bwd_ms = median_ms(torch_bwd, max(iters // 4, 2))
            with torch.no_grad():
                torch_fwd_ms = median_ms(lambda: [_torch_block(x, keep, w, b, gws[i], mul) for i, (x, w, b) in enumerate(leaves)],
                                          max(iters // 4, 2))
            print(json.dumps({'shape': [B, Fmax, d], 'mul': bool(mul), 'count': k, 'kernel_ms': round(kernel_ms, 4),
                              'op_ms': round(op_ms, 4), 'torch_bwd_ms': round(torch_bwd_ms, 4), 'torch_fwd_ms': round(torch_fwd_ms, 4),
                              'ratio': round(torch_bwd_ms / kernel_ms, 2), 'torch_wins': bool(torch_bwd_ms < kernel_ms),
                              'mandatory_bytes': k * mandatory,
                              'hbm_fraction': round(k * mandatory / (kernel_ms * 1e-3) / HBM_PEAK, 3),
                              'err_kernel_dx_dw': [float('%.3g' % e) for e in e_k], 'err_torch_dx_dw': [float('%.3g' % e) for e in e_t],
                              'bound_dx_dw': [float('%.3g' % e) for e in bound]}), flush=True)
            del Vs, leaves
    return status


if __name__ == '__main__':
    sys.exit(run_child(child, 20, default_timeout=400))
