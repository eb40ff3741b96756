"""Times one training step of the GRU caption encoder -- forward + backward of GruTxtEncoder(differentiable=True) on a prepared batch --
against the same step through torch on the same device: nn.Embedding, pack_padded_sequence, nn.GRU (MIOpen), pad_packed_sequence and
the mean pooling, forward + backward.

    python tools/gru_backward_time.py [--timeout SECONDS] [--iters K]

N = 128 captions (the reference's training batch is of that order), H = 1024, we_dim = 500, V = 11,286, seeded MSR-VTT-like lengths
(mean ~11 tokens with <start> / <end>, at most 40).  The measurement runs once, in a child process that is ended after --timeout
seconds.  Times are HIP events around K back-to-back steps after a warm-up, the median of 5 such windows.  One JSON line per net
(gru_mean, bigru_mean):
    ours_ms        encode_batch(...) then .backward(dout): gather, GI GEMM, pack, T saving steps; T backward steps, the weight GEMMs, d_we
    ours_fwd_ms    the training forward alone
    torch_ms       the torch step; where MIOpen refuses the shape the line carries "torch_refused" with its message instead
    ratio          torch_ms / ours_ms
Before anything is timed the kernel is held to the rule of tests/test_gpu_gru_backward.py against a float64 CPU nn.GRU under autograd:
for the output and every gradient tensor, max |device - f64| / max |f64| <= max(4 x the float32 CPU graph's error, 1.5e-6).  A miss
ends the run with exit status 1 and no timing line.
"""
import json
import os
import sys

from train_time import median_ms, run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, WE, V = 128, 1024, 500, 11286
TOL_UNIT = 1.5e-6


def child(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import gru_bwd_ref as R
    from laff_amd import txt2vec as T
    voc = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + ['w%d' % i for i in range(V - 4)]:
        voc.add(w)
    g = np.random.default_rng(0)
    lens = np.clip(g.poisson(9, N), 1, 38)
    lens[0] = 38
    caps = [' '.join('w%d' % i for i in g.integers(0, V - 4, L)) for L in lens]
    for net in ('gru_mean', 'bigru_mean'):
        bi = net.startswith('bigru')
        torch.manual_seed(1)
        enc = T.GruTxtEncoder(T.IdxVec(voc), WE, H, bidirectional=bi, pooling='mean', device='cuda', differentiable=True).train()
        hb = enc.t2v_idx.batch(caps)
        b = enc.to_device(hb)
        dout = torch.randn(N, 2 * H if bi else H, device='cuda')
        params = list(enc.parameters())

        def ours():
            for p in params:
                p.grad = None
            enc.encode_batch(b).backward(dout)
        # the accuracy rule first
        ours()
        out = enc.encode_batch(b).detach().cpu().numpy()
        ids = [enc.t2v_idx.encoding(c) for c in caps]
        sd = {k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}
        o64, ref = R.autograd_grads(ids, sd, 'mean', bi, dout.cpu().numpy())
        o32, f32 = R.autograd_grads(ids, sd, 'mean', bi, dout.cpu().numpy(), dtype=torch.float32)
        got = {k: p.grad.cpu().numpy() for k, p in enc.named_parameters()}
        used = {'out': R.rel_err(out, o64) / max(4.0 * R.rel_err(o32, o64), TOL_UNIT)}
        for k in ref:
            used[k] = R.rel_err(got[k], ref[k]) / max(4.0 * R.rel_err(f32[k], ref[k]), TOL_UNIT)
        if not max(used.values()) <= 1.0:
            print('%s: the kernel misses the accuracy rule, fractions of the bound %s: nothing is timed' % (net, used), file=sys.stderr)
            return 1
        line = {'net': net, 'N': N, 'H': H, 'we_dim': WE, 'V': V, 'tokens': int(sum(hb.batch_sizes)), 'T': len(hb.batch_sizes),
                'largest_used_fraction_of_bound': round(max(used.values()), 3)}
        line['ours_ms'] = round(median_ms(ours, iters), 4)
        line['ours_fwd_ms'] = round(median_ms(lambda: enc.encode_batch(b), iters), 4)
        # the same step through torch on the device
        try:
            we = torch.nn.Embedding(V, WE).cuda()
            rnn = torch.nn.GRU(WE, H, 1, batch_first=True, bidirectional=bi).cuda()
            we.load_state_dict({'weight': enc.we.weight.detach()})
            rnn.load_state_dict({k[4:]: v for k, v in enc.state_dict().items() if k.startswith('rnn.')})
            order = np.argsort(-lens, kind='stable')
            tok = torch.zeros(N, int(hb.lengths.max()), dtype=torch.long)
            for j, i in enumerate(order):
                tok[j, :len(ids[i])] = torch.as_tensor(ids[i])
            tok = tok.cuda()
            slen = torch.as_tensor(hb.lengths.astype(np.int64))
            ln = slen.cuda().float()[:, None]
            inv = torch.as_tensor(np.argsort(order)).cuda()
            tparams = list(we.parameters()) + list(rnn.parameters())

            def theirs():
                for p in tparams:
                    p.grad = None
                packed = torch.nn.utils.rnn.pack_padded_sequence(we(tok), slen, batch_first=True)
                y, _ = torch.nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], batch_first=True)
                ((y.sum(1) / ln)[inv]).backward(dout)
            theirs()
            torch.cuda.synchronize()
            line['max_abs_diff_dW_hh_vs_torch'] = float((rnn.weight_hh_l0.grad - enc.rnn.weight_hh_l0.grad).abs().max())
            line['torch_ms'] = round(median_ms(theirs, iters), 4)
            line['ratio'] = round(line['torch_ms'] / line['ours_ms'], 2)
        except RuntimeError as e:                       # MIOpen refuses some batch shapes outright
            line['torch_refused'] = str(e).splitlines()[0][:200]
        print(json.dumps(line), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 10))
