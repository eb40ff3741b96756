#!/usr/bin/env python3
"""Times the NetVLAD text encoder (txt2vec.NetVLADTxtEncoder, laff_netvlad_encode) against torch restatements on the device.

For each case (N captions of 1 + Poisson(8) words, capped at 30, over a V = 100,000-word table of width D = 500, K = 32 clusters, with
a few stop and unknown words: about 6-9 distinct known words per caption) these are timed with device events around work that ends
in a synchronise:
  encoder_device  laff_netvlad_encode alone on a prepared batch (ids, offsets and zero-row counts already on the device)
  encoder         NetVLADTxtEncoder.forward from caption strings (tokenising and the host-to-device copies included)
  ref_loop        the reference's shape (model/model.py:538-549 over model/Attention.py:885-918): per caption, its rows gathered
                  on the device, F.normalize, fc1, softmax, the M x K x D residual, its sum; then stack and the two normalisations
  padded          a batched eager-torch restatement: rows padded to the longest caption with a mask, the same arithmetic as einsums
and fc_after: the K*D -> 2048 TransformNet projection that follows in the text tower (ops.fc_act_bn), as context.
write_tbps is the output's bytes (N K D 4) over encoder_device; the write roof is about 6.3 TB/s (float4 copy).

    python tools/bench_netvlad.py [--cases 1,64,4096,40000] [--reps 10] [--out FILE.json]
    python tools/bench_netvlad.py --encoder-only ...     # only the device call (for a rocprofv3 --kernel-trace run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from laff_amd import txt2vec as T  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

V, D, K, D_OUT = 100000, 500, 32, 2048


def captions(n, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(1 + g.poisson(8.0, n), 30)
    caps = []
    for L in lens:
        ws = ['w%d' % i for i in g.integers(0, V, L)]
        if L > 4:
            ws[1], ws[3] = 'the', 'notaword'
        caps.append(' '.join(ws))
    return caps


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


def ref_loop(table, rows, fc1, cent):
    """Per caption as the reference runs it, its rows gathered from the device table."""
    vlad = []
    for ids, n in rows:
        x = table[torch.as_tensor(ids, device='cuda', dtype=torch.long)] if ids else table.new_zeros((n, D))
        x = F.normalize(x, p=2, dim=-1)
        a = F.softmax(x @ fc1.t(), dim=-1)
        res = x.expand(K, -1, -1).permute(1, 0, 2) - cent.expand(x.shape[0], -1, -1)
        res = res * a.unsqueeze(-1)
        vlad.append(res.sum(dim=0))
    v = F.normalize(torch.stack(vlad, 0), p=2, dim=2)
    return F.normalize(v.view(v.shape[0], -1), p=2, dim=1)


def padded(table, idx, mask, fc1, cent):
    """Batched: idx [N, L] rows (0 where masked), mask [N, L] (1 = a row; zero rows of an unknown-only caption are rows of 0)."""
    x = F.normalize(table[idx] * (mask > 0).unsqueeze(-1), p=2, dim=-1)
    a = F.softmax(x @ fc1.t(), dim=-1) * mask.unsqueeze(-1)
    u = torch.einsum('nlk,nld->nkd', a, x) - a.sum(1).unsqueeze(-1) * cent
    v = F.normalize(u, p=2, dim=2)
    return F.normalize(v.reshape(v.shape[0], -1), p=2, dim=1)


def padded_batch(rows):
    L = max(1, max(len(ids) if ids else n for ids, n in rows))
    idx = np.zeros((len(rows), L), np.int64)
    mask = np.zeros((len(rows), L), np.float32)
    for i, (ids, n) in enumerate(rows):
        idx[i, :len(ids)] = ids
        mask[i, :len(ids) if ids else n] = 1.0
    return torch.from_numpy(idx).cuda(), torch.from_numpy(mask).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1,64,4096,40000')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--encoder-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_netvlad.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    from laff_amd import ops
    g = np.random.default_rng(0)
    w2v = T.W2Vec(['w%d' % i for i in range(V)], g.normal(0, 1, (V, D)).astype(np.float32), stopwords=('the',))
    torch.manual_seed(0)
    enc = T.NetVLADTxtEncoder(w2v, num_clusters=K, device='cuda')
    table = w2v.device_table('cuda')
    fc1, cent = enc.netvlad.fc1.weight.detach(), enc.netvlad.centeroids.detach()
    W_fc = torch.randn(D_OUT, K * D, device='cuda') / np.sqrt(K * D)
    b_fc = torch.zeros(D_OUT, device='cuda')
    rows_out = []
    for n in [int(x) for x in a.cases.split(',')]:
        caps = captions(n, n)
        ragged = w2v.ragged(caps)
        b = enc.to_device(*ragged)
        ws = torch.empty(max(16, ops.netvlad_workspace_bytes(len(ragged[0]), K)), dtype=torch.uint8, device='cuda')
        out = torch.empty((n, K * D), device='cuda')
        reps = a.reps if n < 10000 else max(1, a.reps // 2)
        r = {'N': n, 'K': K, 'D': D, 'rows': int(len(ragged[0])), 'rows_per_caption': len(ragged[0]) / n,
             'out_gb': n * K * D * 4 / 1e9}
        r['encoder_device_ms'] = timed(lambda: enc.encode_batch(*b, out=out, workspace=ws), reps)
        r['write_tbps'] = n * K * D * 4 / (r['encoder_device_ms'] * 1e-3) / 1e12
        if not a.encoder_only:
            r['encoder_ms'] = timed(lambda: enc({'caption': caps}), reps)
            rows = [w2v.raw_ids(c) for c in caps]
            ref_reps = 1 if n >= 4096 else reps
            r['ref_loop_ms'] = timed(lambda: ref_loop(table, rows, fc1, cent), ref_reps)
            ours = enc.encode_batch(*b)
            r['max_abs_diff_vs_ref_loop'] = float((ref_loop(table, rows, fc1, cent) - ours).abs().max())
            idx, mask = padded_batch(rows)
            chunk = n if n <= 4096 else 4096       # the padded M x K x D intermediate of 40,000 captions would not fit
            parts = [(idx[i:i + chunk], mask[i:i + chunk]) for i in range(0, n, chunk)]
            r['padded_batch'] = chunk
            r['padded_ms'] = timed(lambda: [padded(table, i_, m_, fc1, cent) for i_, m_ in parts], reps)
            r['max_abs_diff_vs_padded'] = float((torch.cat([padded(table, i_, m_, fc1, cent) for i_, m_ in parts]) - ours).abs().max())
            r['fc_after_ms'] = timed(lambda: ops.fc_act_bn(out, W_fc, b_fc), reps)
        print(json.dumps(r), flush=True)
        rows_out.append(r)
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'V': V, 'D': D, 'K': K, 'rows': rows_out}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device']}))


if __name__ == '__main__':
    main()
