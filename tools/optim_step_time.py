"""Times the fused optimizer step (laff_amd.optim with grad_clip = 2: one norm launch set and one update launch set, DESIGN.md section
4.21) against torch.nn.utils.clip_grad_norm_ followed by torch.optim's own step on the same device, in the same run.

    python tools/optim_step_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Per parameter set and optimizer one JSON line:
    fused_ms / fused_wall_ms         optim.Adam / optim.RMSprop(grad_clip=2).step(): device time by HIP events around K back-to-back
                                     steps after a warm-up, the median of 5 such windows; host wall time per step of the same windows
    torch_foreach_ms / _wall_ms      clip_grad_norm_(params, 2) + torch.optim.*.step() in its default (foreach) form
    torch_fused_ms / _wall_ms        the same with fused=True, where this build of torch constructs it (else null)
    launches                         of the fused step, from laff_optim_plan: it must be 2 for a one-group set that fits the table
    hbm_fraction                     the mandatory bytes -- 28 B an element for Adam (read p, g, m, v; write p, m, v), 20 B for RMSprop,
                                     plus 4 B for the norm pass -- over fused_ms, as a fraction of HBM_PEAK
Before anything is timed one step of each is compared from equal state: the float64 formulas are evaluated on the device and the fused
step's parameters have to stay within the whole-step bound of tests/test_gpu_optim.py (test_state_dict_moves_to_torch_on_the_device);
the two fp32 results may then differ by four of them.  A miss ends the run with exit status 1 and no timing line for that set.
"""
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
U = 2.0 ** -24


def laff_set(dk):
    """8 x {fc1.weight (4096, dk), fc1.bias, BatchNorm weight and bias} plus the 2 x 8 attention heads' Linear(512, 1)."""
    shapes = []
    for _ in range(8):
        shapes += [(4096, dk), (4096,), (4096,), (4096,)]
    for _ in range(16):
        shapes += [(1, 512), (1,)]
    return shapes


SETS = [('LAFF Dk=512', laff_set(512)), ('LAFF Dk=2048', laff_set(2048)), ('small 8 x (512, 512)', [s for _ in range(8) for s in ((512, 512), (512,))])]


def _gate(kind, params, grads, make_mine, make_torch):
    """One step of each from equal state against float64 on the device; returns (fraction of the bound used, bounds apart) or None."""
    import torch
    p0 = [p.detach().clone() for p in params]
    mine, theirs = [torch.nn.Parameter(p.clone()) for p in p0], [torch.nn.Parameter(p.clone()) for p in p0]
    for plist in (mine, theirs):
        for p, g in zip(plist, grads):
            p.grad = g.clone()
    make_mine(mine).step()
    torch.nn.utils.clip_grad_norm_(theirs, 2.0)
    make_torch(theirs).step()
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads))
    c = torch.clamp(2.0 / (total + 1e-6), max=1.0)
    used = apart = 0.0
    for p, a, b, g in zip(p0, [t.detach() for t in mine], [t.detach() for t in theirs], grads):
        p64, gh = p.double(), c * g.double()
        G = gh.abs()
        if kind == 'adam':                                # step 1 from zero moments, lr 1e-3, betas (0.9, 0.999), eps 1e-4
            m, v = 0.1 * gh, 0.001 * gh * gh
            ss, bc2 = 1e-3 / 0.1, 0.001
            den = v.sqrt() / bc2 ** 0.5 + 1e-4
            ref = p64 - ss * (m / den)
            bm, bv = 10 * U * 0.1 * G, 14 * U * 0.001 * G * G
            dden = torch.where(v > 0, bv / (2.0 * v.sqrt().clamp_min(1e-300) * bc2 ** 0.5), torch.zeros_like(v))
            bound = U * ref.abs() + 13 * U * ss * m.abs() / den + ss * bm / den + ss * m.abs() / den ** 2 * dden
        else:                                             # lr 1e-2, alpha 0.99, eps 1e-8
            s = 0.01 * gh * gh
            den = s.sqrt() + 1e-8
            ref = p64 - 1e-2 * (gh / den)
            bs = 14 * U * 0.01 * G * G
            dden = torch.where(s > 0, bs / (2.0 * s.sqrt().clamp_min(1e-300)), torch.zeros_like(s))
            bound = U * ref.abs() + 13 * U * 1e-2 * G / den + 1e-2 * G / den ** 2 * dden
        ok = bound > 0
        if not bool(((a.double() - ref)[~ok] == 0).all()):
            return None
        used = max(used, float(((a.double() - ref).abs()[ok] / bound[ok]).max()))
        apart = max(apart, float(((a.double() - b.double()).abs()[ok] / bound[ok]).max()))
    return used, apart


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops, optim
    dev = torch.device('cuda')
    rc = 0
    for label, shapes in SETS:
        g = torch.Generator(device='cuda').manual_seed(len(shapes))
        params = [torch.randn(s, device=dev, generator=g) * 0.05 for s in shapes]
        grads = [torch.randn(s, device=dev, generator=g) * 1e-2 for s in shapes]
        n = sum(p.numel() for p in params)
        plan = ops.optim_plan([p.numel() for p in params])
        launches = plan[2] + plan[4]
        assert len(shapes) > plan[1] or launches == 2, (label, plan)           # a one-group set that fits the table: 2 launches
        for kind, cls, kw, bytes_per in (('adam', 'Adam', dict(lr=1e-3, eps=1e-4), 28), ('rmsprop', 'RMSprop', dict(lr=1e-2), 20)):
            gate = _gate(kind, params, grads, lambda ps: getattr(optim, cls)(ps, grad_clip=2.0, **kw), lambda ps: getattr(torch.optim, cls)(ps, **kw))
            if gate is None or not (gate[0] <= 1.0 and gate[1] <= 4.0):
                print('%s %s: the fused step uses %s of its bound / lies that many bounds from torch: nothing is timed' % (label, kind, gate),
                      file=sys.stderr)
                rc = 1
                continue
            row = {'set': label, 'optimizer': kind, 'tensors': len(shapes), 'elements': n, 'launches': launches}

            def run(make, clip):
                ps = [torch.nn.Parameter(p.clone()) for p in params]
                for p, gr in zip(ps, grads):
                    p.grad = gr.clone()
                opt = make(ps)

                def step():
                    if clip:
                        torch.nn.utils.clip_grad_norm_(ps, 2.0)
                    opt.step()
                return median_ms(step, iters, wall=True)
            row['fused_ms'], row['fused_wall_ms'] = run(lambda ps: getattr(optim, cls)(ps, grad_clip=2.0, **kw), False)
            row['torch_foreach_ms'], row['torch_foreach_wall_ms'] = run(lambda ps: getattr(torch.optim, cls)(ps, **kw), True)
            try:
                row['torch_fused_ms'], row['torch_fused_wall_ms'] = run(lambda ps: getattr(torch.optim, cls)(ps, fused=True, **kw), True)
            except (TypeError, RuntimeError, ValueError):                      # this build of torch has no fused form of it
                row['torch_fused_ms'] = row['torch_fused_wall_ms'] = None
            mandatory = (bytes_per + 4) * n
            row['mandatory_bytes'] = mandatory
            row['hbm_fraction'] = round(mandatory / (row['fused_ms'] * 1e-3) / HBM_PEAK, 3)
            row['gate_used_fraction_of_bound'], row['gate_bounds_from_torch'] = round(gate[0], 3), round(gate[1], 3)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    return rc


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
