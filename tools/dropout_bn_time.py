"""Times laff_dropout_bn_train and its backward against torch's own F.dropout + BatchNorm1d (training mode) on the same device -- the
route a TransformNet takes without device_norm.

    python tools/dropout_bn_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back calls
after a warm-up, the median of 5 such windows.  Per shape (N, D) and per stage (p = 0.2 + BatchNorm, BatchNorm only, dropout only) one
JSON line:
    fwd_ms / bwd_ms              the C entry points with every buffer made beforehand
    op_fwd_ms / op_bwd_ms        the same through ops.dropout_bn_train(_backward), which allocate outputs and workspace per call
    torch_fwd_ms / torch_bwd_ms  bn(F.dropout(a, p)) and torch.autograd.grad of it with respect to a, weight and bias (forward kept)
    ratio_fwd / ratio_bwd        torch over kernel
    launches                     per call and direction: this library's from the plan, torch's counted by torch.profiler (None when the
                                 profiler reports no device kernels)
    hbm_fraction_fwd / _bwd      the mandatory bytes -- forward: read A, write Y; backward: read dY (and A with a BatchNorm stage), write
                                 dA -- over the kernel time, as a fraction of HBM_PEAK
Before anything is timed the kernel is held to the rule of tests/test_gpu_dropout_bn.py: per tensor, max |device - float64| / max |float64|
<= max(4 e32, 1.5e-6), float64 being tests/dropout_bn_ref.py on the same fp32 inputs with the mask recomputed on the host, e32 the same
error of float32 CPU torch with that mask.  A miss ends the run with exit status 1 and no timing line for that row.
"""
import json
import os
import sys

from train_time import median_ms, run_child, torch_launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 512), (128, 2048), (128, 4096), (8192, 512)]
STAGES = [('dropout0.2+bn', 0.2, True), ('bn', 0.0, True), ('dropout0.2', 0.2, False)]
HBM_PEAK = 8.0e12
TOL_UNIT = 1.5e-6
SEED = 0x0123456789abcdef
EPS, MOMENTUM = 1e-5, 0.1


def child(iters):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import dropout_bn_ref as R
    from laff_amd import ops
    dev = torch.device('cuda')
    for N, D in SHAPES:
        g = torch.Generator().manual_seed(N + D)
        a_h, dy_h = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
        gamma_h, beta_h = torch.randn(D, generator=g), torch.randn(D, generator=g)
        a, dy, gamma, beta = a_h.to(dev), dy_h.to(dev), gamma_h.to(dev), beta_h.to(dev)
        seed = torch.tensor([SEED], dtype=torch.int64, device=dev)
        lib, ctx = ops._context(dev)
        for name, p, bn in STAGES:
            chunks, nbytes, launches, _ = ops.dropout_bn_train_plan(N, D, bn)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            y, da = torch.empty(N, D, device=dev), torch.empty(N, D, device=dev)
            sm, si, dg, db = (torch.empty(D, device=dev) for _ in range(4))
            rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
            P = ops._ptr
            sd = P(seed) if p else None
            if bn:
                fwd = lambda: ops.check(lib.laff_dropout_bn_train(ctx, P(a), N, D, D, p, sd, P(gamma), P(beta), P(rm), P(rv), MOMENTUM, EPS, P(y), D,
                                                                  P(sm), P(si), P(ws), nbytes))       # noqa: E731
                bwd = lambda: ops.check(lib.laff_dropout_bn_train_backward(ctx, P(dy), D, P(a), N, D, D, p, sd, P(gamma), P(sm), P(si), P(da), D,
                                                                           P(dg), P(db), P(ws), nbytes))      # noqa: E731
            else:
                fwd = lambda: ops.check(lib.laff_dropout_bn_train(ctx, P(a), N, D, D, p, sd, None, None, None, None, MOMENTUM, EPS, P(y), D,
                                                                  None, None, None, 0))       # noqa: E731
                bwd = lambda: ops.check(lib.laff_dropout_bn_train_backward(ctx, P(dy), D, P(a), N, D, D, p, sd, None, None, None, P(da), D,
                                                                           None, None, None, 0))      # noqa: E731
            # ---- the rule, before anything is timed ----
            fwd()
            bwd()
            torch.cuda.synchronize()
            keep = R.keep_mask(SEED, N, D, p)
            f = R.forward(a_h, keep, p, gamma_h if bn else None, beta_h, np.zeros(D), np.ones(D), MOMENTUM, EPS)
            r = R.backward(dy_h, a_h, keep, p, gamma_h if bn else None, sm.cpu() if bn else None, si.cpu() if bn else None)
            ref = dict(y=f['y'], da=r[0])
            got = dict(y=y, da=da)
            at = a_h.clone().requires_grad_(True)
            u32 = at * torch.from_numpy(keep) * float(R.scale32(p)) if p else at * 1.0
            if bn:
                ref.update(dgamma=r[1], dbeta=r[2], save_mean=f['mean'], save_invstd=f['invstd'], running_mean=f['running_mean'],
                           running_var=f['running_var'])
                got.update(dgamma=dg, dbeta=db, save_mean=sm, save_invstd=si, running_mean=rm, running_var=rv)
                norm = torch.nn.BatchNorm1d(D, eps=EPS, momentum=MOMENTUM).train()
                with torch.no_grad():
                    norm.weight.copy_(gamma_h)
                    norm.bias.copy_(beta_h)
                _, mean_t, invstd_t = torch.native_batch_norm(u32.detach(), gamma_h, beta_h, torch.zeros(D), torch.ones(D), True, MOMENTUM, EPS)
                y32 = norm(u32)
                y32.backward(dy_h)
                cpu32 = dict(y=y32, da=at.grad, dgamma=norm.weight.grad, dbeta=norm.bias.grad, running_mean=norm.running_mean,
                             running_var=norm.running_var, save_mean=mean_t, save_invstd=invstd_t)
            else:
                u32.backward(dy_h)
                cpu32 = dict(y=u32, da=at.grad)
            used = {}
            for k in ref:
                bound = max(4.0 * (R.rel_err(cpu32[k], ref[k]) if k in cpu32 else 0.0), TOL_UNIT)
                used[k] = R.rel_err(got[k], ref[k]) / bound
                if not used[k] <= 1.0:
                    print('%s at %s %s: %.3g of its bound: nothing is timed' % (k, (N, D), name, used[k]), file=sys.stderr)
                    return 1
            # ---- torch's own route on the device ----
            norm = torch.nn.BatchNorm1d(D, eps=EPS, momentum=MOMENTUM).to(dev).train() if bn else None
            ag = a.clone().requires_grad_(True)

            def t_fwd():
                z = F.dropout(ag, p, training=True) if p else ag
                return norm(z) if bn else z
            yt = t_fwd()
            leaves = [ag] + ([norm.weight, norm.bias] if bn else [])
            t_bwd = lambda: torch.autograd.grad(yt, leaves, dy, retain_graph=True)       # noqa: E731
            row = {'shape': [N, D], 'stage': name, 'chunks': chunks,
                   'launches': {'fwd': launches, 'bwd': launches, 'torch_fwd': torch_launches(t_fwd), 'torch_bwd': torch_launches(t_bwd)}}
            times = {'fwd_ms': median_ms(fwd, iters), 'bwd_ms': median_ms(bwd, iters),
                     'op_fwd_ms': median_ms(lambda: ops.dropout_bn_train(a, p, seed if p else None, gamma if bn else None, beta, rm, rv,
                                                                         MOMENTUM, EPS), iters),
                     'op_bwd_ms': median_ms(lambda: ops.dropout_bn_train_backward(dy, a, p, seed if p else None, gamma if bn else None, sm, si,
                                                                                  True, bn, bn), iters),
                     'torch_fwd_ms': median_ms(t_fwd, iters), 'torch_bwd_ms': median_ms(t_bwd, iters)}
            bytes_fwd, bytes_bwd = 4 * 2 * N * D, 4 * (3 if bn else 2) * N * D
            row.update({k: round(v, 4) for k, v in times.items()})
            row.update({'ratio_fwd': round(times['torch_fwd_ms'] / times['fwd_ms'], 2), 'ratio_bwd': round(times['torch_bwd_ms'] / times['bwd_ms'], 2),
                        'mandatory_bytes': [bytes_fwd, bytes_bwd],
                        'hbm_fraction_fwd': round(bytes_fwd / (times['fwd_ms'] * 1e-3) / HBM_PEAK, 4),
                        'hbm_fraction_bwd': round(bytes_bwd / (times['bwd_ms'] * 1e-3) / HBM_PEAK, 4),
                        'largest_used_fraction_of_bound': {k: round(v, 4) for k, v in used.items()}})
            print(json.dumps(row), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 200))
