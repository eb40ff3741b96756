"""What the training-path timing tools (tools/*_backward_time.py, tools/optim_step_time.py) share: the timed window, the count of
torch's launches and the parent / child process scaffold."""
import argparse
import os
import subprocess
import sys
import time


def median_ms(fn, iters, wall=False):
    """Device time of fn by HIP events around `iters` back-to-back calls after a warm-up of 3, the median of 5 such windows; with
    `wall` the pair (device, host wall time per call of the same windows)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - w0) * 1e3 / iters)
        dev.append(t0.elapsed_time(t1) / iters)
    return (sorted(dev)[2], sorted(host)[2]) if wall else sorted(dev)[2]


def torch_launches(fn):
    """Device kernels of one call of fn, counted by torch.profiler; None when it sees none."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower())
        return n or None
    except Exception:
        return None


def run_child(child, default_iters, default_timeout=240):
    """The tool's main(): `--child` runs child(iters) here; otherwise the tool starts itself once more with --child, in a process
    that is ended after --timeout seconds, and returns its exit status."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--timeout', type=int, default=default_timeout)
    ap.add_argument('--iters', type=int, default=default_iters)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.iters)
    r = subprocess.run([sys.executable, os.path.abspath(sys.argv[0]), '--child', '--iters', str(a.iters)], timeout=a.timeout)
    return r.returncode
