"""Times the no-transform feature's training-mode BatchNorm, forward plus backward under autograd, on its two routes (DESIGN.md section
4.26): _TileBnFn (laff_tile_bn_train, the tiled input never formed) against what the library offered before it -- x.repeat(1, H), then
_DropoutBnFn with p = 0 (laff_dropout_bn_train and its backward), torch summing dX over the heads in repeat's own backward.

    python tools/tile_bn_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back
forward + backward pairs after a warm-up, five such windows per route.  Per shape (N, C, H) and per kind of input (a pre-extracted
feature: no dX; a trained one: with dX) one JSON line:
    tile_ms / repeat_ms        the median window of each route
    tile_spread / repeat_spread  [min, max] of the five windows
    ratio                      repeat_ms over tile_ms
    no_slower                  tile_ms <= repeat_ms + (the larger of the two routes' max - min)
Before anything is timed both routes' y, dgamma and dbeta have to be equal bit for bit; a difference ends the run with exit status 1.
"""
import json
import os
import sys

from train_time import run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 512, 8), (256, 512, 8), (512, 512, 8)]
EPS, MOMENTUM = 1e-5, 0.1


def windows_ms(fn, iters):
    """Device time per call of fn by HIP events around `iters` back-to-back calls after a warm-up of 3: five such windows, sorted."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / iters)
    return sorted(out)


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd.model.autograd import _DropoutBnFn, _TileBnFn
    dev = torch.device('cuda')
    for N, C, H in SHAPES:
        g = torch.Generator().manual_seed(N + C + H)
        x0 = torch.randn(N, C, generator=g).to(dev)
        dy = torch.randn(N, H * C, generator=g).to(dev)
        gamma = torch.randn(H * C, generator=g).to(dev).requires_grad_(True)
        beta = torch.randn(H * C, generator=g).to(dev).requires_grad_(True)
        rm, rv = torch.zeros(H * C, device=dev), torch.ones(H * C, device=dev)
        for with_dx in (False, True):
            x = x0.clone().requires_grad_(with_dx)
            leaves = ([x] if with_dx else []) + [gamma, beta]

            def tile():
                y = _TileBnFn.apply(x, H, gamma, beta, rm, rv, MOMENTUM, EPS)
                return y, torch.autograd.grad(y, leaves, dy)

            def repeat():
                y = _DropoutBnFn.apply(x.repeat(1, H), gamma, beta, rm, rv, None, MOMENTUM, EPS)
                return y, torch.autograd.grad(y, leaves, dy)
            (yt, gt), (yr, gr) = tile(), repeat()
            torch.cuda.synchronize()
            if not (torch.equal(yt, yr) and torch.equal(gt[-2], gr[-2]) and torch.equal(gt[-1], gr[-1])):
                print('the routes differ at %s: nothing is timed' % ((N, C, H),), file=sys.stderr)
                return 1
            t, r = windows_ms(tile, iters), windows_ms(repeat, iters)
            spread = max(t[-1] - t[0], r[-1] - r[0])
            print(json.dumps({'shape': [N, C, H], 'dx': with_dx, 'tile_ms': round(t[2], 4), 'repeat_ms': round(r[2], 4),
                              'tile_spread': [round(t[0], 4), round(t[-1], 4)], 'repeat_spread': [round(r[0], 4), round(r[-1], 4)],
                              'ratio': round(r[2] / t[2], 2), 'no_slower': bool(t[2] <= r[2] + spread),
                              'dx_max_abs_diff': float((gt[0] - gr[0]).abs().max()) if with_dx else None}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 200))
