"""Times one training step of the NetVLAD caption encoder -- forward + backward of NetVLADTxtEncoder(differentiable=True) on a prepared
batch -- against two restatements of the reference's module in torch on the same device:

    loop      the reference's own formulation: a Python loop over the captions (normalize, Linear, softmax, the expanded residual),
              then the two normalisations, under autograd
    padded    the same mathematics fully vectorised over a zero-padded [N, M_max, D] batch with a row mask (bmm for the pooling)

    python tools/netvlad_backward_time.py [--timeout SECONDS] [--iters K]

The reference's training size: N = 128 captions of 5..25 rows, K = 32 clusters, D = 500, a table of 11,286 rows.  The measurement runs
once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back steps after a warm-up, the
median of 5 such windows, with the host's wall time per step of the same windows beside them (the step is bound by launches).  One JSON
line:
    ours_ms / ours_wall_ms        encode_batch(...) then .backward(dout): 2 launches forward, 3 backward
    ours_fwd_ms                   the saving forward alone
    ours_graph_ms                 the five launches replayed from a captured HIP graph: the step without the host side of its calls
    loop_ms, padded_ms (+ wall)   the torch steps; *_launches: device kernels of one step as torch's profiler counts them (null where the
                                  profiler is not available)
    ratio_padded                  padded_ms / ours_ms
Before anything is timed the kernels are held to the rule of tests/test_gpu_netvlad_backward.py against float64: for the output and both
gradients, max |device - f64| / max |f64| <= max(4 x the float32 CPU graph's error, 1.5e-6).  A miss ends the run with exit status 1 and
no timing line.
"""
import json
import os
import sys

from train_time import median_ms, run_child, torch_launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, D, V = 128, 32, 500, 11286
TOL_UNIT = 1.5e-6


def child(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import netvlad_bwd_ref as B
    from laff_amd import txt2vec as T
    F = torch.nn.functional
    g = np.random.default_rng(0)
    table = g.normal(0, 1, (V, D)).astype(np.float32)
    w2v = T.W2Vec(['w%d' % i for i in range(V)], table)
    caps = [' '.join('w%d' % i for i in g.choice(V, int(L), replace=False)) for L in g.integers(5, 26, N)]
    torch.manual_seed(1)
    enc = T.NetVLADTxtEncoder(w2v, num_clusters=K, device='cuda', differentiable=True).train()
    b = enc.to_device(*w2v.ragged(caps))
    dout = torch.randn(N, K * D, device='cuda')
    params = [enc.netvlad.fc1.weight, enc.netvlad.centeroids]

    def ours():
        for p in params:
            p.grad = None
        enc.encode_batch(*b).backward(dout)
    # the accuracy rule first
    ours()
    out = enc.encode_batch(*b).detach().cpu().numpy()
    rows = [table[ids] for ids, _ in (w2v.raw_ids(c) for c in caps)]
    fc1, cent = (p.detach().cpu().numpy() for p in params)
    o64, f64, c64 = B.netvlad_backward(rows, fc1, cent, dout.cpu().numpy())
    ref = {'out': o64, 'fc1.weight': f64, 'centeroids': c64}
    f32 = B.torch_module_grads(rows, fc1, cent, dout.cpu().numpy(), torch.float32)
    got = {'out': out, 'fc1.weight': params[0].grad.cpu().numpy(), 'centeroids': params[1].grad.cpu().numpy()}
    used = {k: B.rel_err(got[k], ref[k]) / max(4.0 * B.rel_err(f32[k], ref[k]), TOL_UNIT) for k in ref}
    if not max(used.values()) <= 1.0:
        print('the kernels miss the accuracy rule, fractions of the bound %s: nothing is timed' % used, file=sys.stderr)
        return 1
    line = {'N': N, 'K': K, 'D': D, 'rows': int(b[0].numel()), 'largest_used_fraction_of_bound': round(max(used.values()), 3)}
    line['ours_ms'], line['ours_wall_ms'] = (round(x, 4) for x in median_ms(ours, iters, wall=True))
    line['ours_fwd_ms'] = round(median_ms(lambda: enc.encode_batch(*b), iters), 4)
    line['ours_launches'] = torch_launches(ours)
    # the same five launches replayed from a captured graph: the device's share of the step, without the host side of the calls
    from laff_amd import ops
    R = int(b[0].numel())
    args = (enc.t2v_w2v.device_table('cuda'),) + tuple(b) + tuple(p.detach() for p in params)
    bufs = dict(out=torch.empty(N, K * D, device='cuda'), d_fc1=torch.empty(K, D, device='cuda'), d_cent=torch.empty(K, D, device='cuda'),
                reserve=torch.empty(ops.netvlad_train_reserve_bytes(N, R, K), dtype=torch.uint8, device='cuda'),
                ws=torch.empty(ops.netvlad_backward_workspace_bytes(N, R, K, D), dtype=torch.uint8, device='cuda'))

    def step():
        o, r = ops.netvlad_encode_train(*args, out=bufs['out'], reserve=bufs['reserve'])
        ops.netvlad_backward(dout, o, r, *args, d_fc1=bufs['d_fc1'], d_centroids=bufs['d_cent'], workspace=bufs['ws'])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    line['ours_graph_ms'] = round(median_ms(graph.replay, iters), 4)
    assert torch.equal(bufs['d_fc1'], params[0].grad) and torch.equal(bufs['d_cent'], params[1].grad)

    # the two torch restatements on the device, from the same parameter values
    W = params[0].detach().clone().requires_grad_(True)
    C = params[1].detach().clone().requires_grad_(True)
    xs = [torch.from_numpy(r).cuda() for r in rows]
    lens = torch.tensor([len(r) for r in rows], device='cuda')
    Mx = int(lens.max())
    X = torch.zeros(N, Mx, D, device='cuda')
    for i, x in enumerate(xs):
        X[i, :len(x)] = x
    mask = (torch.arange(Mx, device='cuda')[None, :] < lens[:, None]).float()[:, :, None]

    def finish(vlad):
        vlad = F.normalize(vlad, p=2, dim=2)
        return F.normalize(vlad.view(vlad.size(0), -1), p=2, dim=1)

    def loop():
        W.grad = C.grad = None
        vlad = []
        for x in xs:
            x = F.normalize(x, p=2, dim=-1)
            a = F.softmax(F.linear(x, W), dim=-1)
            residual = x.expand(K, -1, -1).permute(1, 0, 2) - C.expand(x.shape[0], -1, -1)
            vlad.append((residual * a.unsqueeze(-1)).sum(dim=0))
        finish(torch.stack(vlad, 0)).backward(dout)

    def padded():
        W.grad = C.grad = None
        xh = F.normalize(X, p=2, dim=-1)
        a = F.softmax(F.linear(xh, W), dim=-1) * mask
        finish(torch.bmm(a.transpose(1, 2), xh) - a.sum(1)[:, :, None] * C).backward(dout)
    for name, fn in (('loop', loop), ('padded', padded)):
        fn()
        torch.cuda.synchronize()
        line['%s_max_rel_diff_vs_ours' % name] = max(B.rel_err(W.grad.cpu().numpy(), got['fc1.weight']),
                                                     B.rel_err(C.grad.cpu().numpy(), got['centeroids']))
        line[name + '_ms'], line[name + '_wall_ms'] = (round(x, 4) for x in median_ms(fn, iters if name == 'padded' else max(1, iters // 5),
                                                                                      wall=True))
        line[name + '_launches'] = torch_launches(fn)
    line['ratio_padded'] = round(line['padded_ms'] / line['ours_ms'], 2)
    print(json.dumps(line), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20))
