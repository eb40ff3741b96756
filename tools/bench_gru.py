#!/usr/bin/env python3
"""Times the GRU caption encoder (txt2vec.GruTxtEncoder, laff_gru_encode) against the reference-shaped path on the device.

For each case (N captions, seeded MSR-VTT-like lengths: mean ~11 tokens with <start>/<end>, max 40; H = 1024, we_dim = 500,
V = 11,286) three things are timed with device events around work that ends in a synchronise:
  encoder    GruTxtEncoder.forward from caption strings (tokenising on the host included)
  ref_path   the reference's GruTxtEncoder.forward shape (model/model.py:340-387): tokenise, embedding, pack_padded_sequence,
             nn.GRU on the device, pad_packed_sequence and the per-row mean loop
  nn_gru     bare nn.GRU on the already packed, already embedded input
and encoder_device: the device half of the encoder alone (laff_gru_encode on a prepared batch).
FLOPs are counted as 6 H^2 per token per direction (the recurrent GEMM; the input half is the P table lookup).

    python tools/bench_gru.py [--cases 1,64,1000,40000] [--nets gru_mean,bigru_mean] [--reps 5] [--out FILE.json]
    python tools/bench_gru.py --encoder-only ...     # only the encoder's device half (for a rocprofv3 --kernel-trace run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from laff_amd import txt2vec as T  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

V, WE, H = 11286, 500, 1024
PEAK_F32 = 157.3e12


def vocab():
    v = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + ['w%d' % i for i in range(V - 4)]:
        v.add(w)
    return v


def captions(n, seed):
    """Token counts without <start>/<end>: 1 + Poisson(8), capped at 38 (so lengths 3..40, mean ~11)."""
    g = np.random.default_rng(seed)
    lens = np.minimum(1 + g.poisson(8.0, n), 38)
    return [' '.join('w%d' % i for i in g.integers(0, V - 4, L)) for L in lens]


def timed(fn, reps):
    """Mean ms per call: device events around `reps` calls followed by a synchronise."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def ref_path(enc, rnn, caps, bi):
    """model/model.py:340-387 on the device (pooling 'mean')."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    idx = [enc.t2v_idx.encoding(c) for c in caps]
    lengths = [len(v) for v in idx]
    x = torch.zeros(len(caps), max(lengths), dtype=torch.long, device='cuda')
    for i, v in enumerate(idx):
        x[i, :lengths[i]] = torch.from_numpy(v)
    x = enc.we(x)
    out, _ = rnn(pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False))
    padded = pad_packed_sequence(out, batch_first=True)
    res = x.new_zeros((len(caps), padded[0].shape[-1]))
    for i, ln in enumerate(lengths):
        res[i] = torch.mean(padded[0][i][:ln], dim=0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1,64,1000,40000')
    ap.add_argument('--nets', default='gru_mean,bigru_mean')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--encoder-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_gru.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    voc = vocab()
    rows = []
    for net in a.nets.split(','):
        bi = net.startswith('bigru')
        torch.manual_seed(0)
        enc = T.GruTxtEncoder(T.IdxVec(voc), WE, H, bidirectional=bi, pooling='mean', device='cuda')
        rnn = None
        if not a.encoder_only:
            rnn = torch.nn.GRU(WE, H, 1, batch_first=True, bidirectional=bi).cuda()
            rnn.load_state_dict({k[4:]: v for k, v in enc.state_dict().items() if k.startswith('rnn.')})
        for n in [int(x) for x in a.cases.split(',')]:
            caps = captions(n, n)
            b = enc.to_device(enc.t2v_idx.batch(caps))
            tokens = int(b.lengths.sum())
            flop = 6.0 * H * H * tokens * (2 if bi else 1)
            reps = max(1, a.reps if n < 10000 else a.reps // 2)
            r = {'net': net, 'N': n, 'tokens': tokens, 'T_max': len(b.batch_sizes), 'gflop': flop / 1e9}
            r['encoder_device_ms'] = timed(lambda: enc.encode_batch(b), reps)
            r['encoder_device_tflops'] = flop / (r['encoder_device_ms'] * 1e-3) / 1e12
            if not a.encoder_only:
                r['encoder_ms'] = timed(lambda: enc({'caption': caps}), reps)
                ours = enc({'caption': caps})['text_features']
                ref_reps = 1 if n >= 10000 else reps
                # nn.GRU (MIOpen) refuses a 40,000-row batch (miopenStatusBadParm, 'Lengths must be > 0'): above 1,000 captions the
                # reference-shaped path runs in 1,000-caption batches, as a loader would feed it (ref_batch)
                chunk = n if n <= 1000 else 1000
                parts = [caps[i:i + chunk] for i in range(0, n, chunk)]
                ref = torch.cat([ref_path(enc, rnn, p_, bi) for p_ in parts])
                r['ref_batch'] = chunk
                r['max_abs_diff_vs_nn_gru'] = float((ref - ours).abs().max())
                r['ref_path_ms'] = timed(lambda: [ref_path(enc, rnn, p_, bi) for p_ in parts], ref_reps)
                from torch.nn.utils.rnn import pack_padded_sequence
                packs = []
                for p_ in parts:
                    lengths = [len(enc.t2v_idx.encoding(c)) for c in p_]
                    x = torch.zeros(len(p_), max(lengths), dtype=torch.long, device='cuda')
                    for i, c in enumerate(p_):
                        x[i, :lengths[i]] = torch.from_numpy(enc.t2v_idx.encoding(c))
                    packs.append(pack_padded_sequence(enc.we(x), lengths, batch_first=True, enforce_sorted=False))
                r['nn_gru_ms'] = timed(lambda: [rnn(pk) for pk in packs], reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'H': H, 'we_dim': WE, 'V': V, 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device']}))


if __name__ == '__main__':
    main()
