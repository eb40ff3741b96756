#!/usr/bin/env python3
"""Times the BERT text encoder (bert_text.BertTxtEncoder, laff_bert_encode) against the reference-shaped path on the device.

bert-base-uncased shape (width 768, 12 heads, 12 layers, intermediate 3072, vocab 30,522; BertConfig's std-0.02 init).  For each
case (N captions, seeded MSR-VTT-like: 1 + Poisson(8) words, at most 40, from a small word list, tokenised with the fixture
vocabulary) three things are timed with device events around work that ends in a synchronise:
  device     the encode call on a prepared ragged batch (ids / row_off already on the device, workspace allocated), per precision
  encoder    BertTxtEncoder.forward from caption strings (tokenising on the host and the row-budget chunking included), fp32
  ref_path   the reference's shape on the device in fp32: every caption of a batch padded to the batch's longest with the dense key
             mask, all rows of every layer (transformers' BertModel when importable, else tests/bert_ref.RefBert), in batches of
             --ref-batch captions as a dataloader feeds the reference, on prepared ids
FLOPs are those of the ragged rows: 2 (4 W^2 + 2 W I) per row and layer, 4 W L^2 per caption and layer for the attention (the
last layer computes the CLS rows only: counted as the reference's work, so the device's TF/s are effective ones), 2 W^2 per
caption for the pooler; TF/s against 2.5 PF (fp16) and 157 TF (fp32).

    python tools/bench_bert.py [--cases 1,64,1000,40000] [--reps 5] [--out FILE.json]
    python tools/bench_bert.py --device-only --precision fp32 --cases 40000   # one precision's device call (a rocprofv3 run)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from laff_amd import bert_text as BT  # noqa: E402
from laff_amd.build import source_hash  # noqa: E402

W, LAYERS, HEADS, INTER, VOCAB = 768, 12, 12, 3072, 30522
PEAK = {'fp16': 2.5e15, 'fp32': 157.3e12}
WORDS = ('a man woman person dog cat is are playing plays guitar piano on the stage in park kitchen street car red blue two '
         'people dancing singing cooking food video of news talking about game football basketball someone how to make water '
         'slow motion child baby').split()
CONFIG = {'hidden_size': W, 'num_attention_heads': HEADS, 'num_hidden_layers': LAYERS, 'intermediate_size': INTER,
          'max_position_embeddings': 512, 'vocab_size': VOCAB, 'type_vocab_size': 2, 'layer_norm_eps': 1e-12}


def captions(n, seed):
    g = np.random.default_rng(seed)
    lens = np.minimum(1 + g.poisson(8.0, n), 40)
    return [' '.join(g.choice(WORDS, L)) for L in lens]


def model_sd(seed=0):
    torch.manual_seed(seed)
    return {k: v.detach() for k, v in BT._BertModel(W, LAYERS, INTER, 512, VOCAB, 2).state_dict().items()}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def flops(row_off):
    L = np.diff(row_off).astype(np.float64)
    return LAYERS * (2.0 * (4 * W * W + 2 * W * INTER) * L.sum() + 4.0 * W * (L * L).sum()) + 2.0 * W * W * len(L)


def ref_model(sd):
    """transformers' BertModel (fp32, eager attention) when importable, else the torch restatement: (callable(ids, mask), name)."""
    try:
        import transformers
    except ImportError:
        from bert_ref import RefBert
        return RefBert(sd, torch.float32), 'bert_ref.RefBert'
    cfg = transformers.BertConfig(**CONFIG, hidden_act='gelu')
    try:
        cfg._attn_implementation = 'eager'
    except AttributeError:
        pass
    m = transformers.BertModel(cfg).eval().cuda()
    missing = [k for k in m.load_state_dict(sd, strict=False).missing_keys if not k.endswith('_ids')]
    assert not missing, missing

    def run(ids, mask):
        return m(input_ids=ids, attention_mask=mask, token_type_ids=torch.zeros_like(ids))['pooler_output']
    return run, 'transformers %s BertModel' % transformers.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='1,64,1000,40000')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ref-batch', type=int, default=1000)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--precision', default=None, help='--device-only: the one precision to run')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_bert.py measures on the GPU; there is no CPU fallback'
    torch.set_grad_enabled(False)
    tok = BT.BertTokenizer(os.path.join(ROOT, 'tests', 'golden', 'bert_vocab.txt'))
    sd = model_sd()
    precs = (a.precision,) if a.precision else ('fp32', 'fp16')
    encs = {p: BT.BertTxtEncoder.from_state_dict(sd, tok, precision=p, config=CONFIG) for p in precs}
    ref, ref_name = (None, None) if a.device_only else ref_model(sd)
    rows = []
    for n in [int(x) for x in a.cases.split(',')]:
        caps = captions(n, n)
        enc0 = encs[precs[0]]
        hb = enc0.batch(caps)
        b = enc0.to_device(hb)
        R = int(hb.row_off[-1])
        f = flops(hb.row_off)
        reps = max(1, a.reps if n < 10000 else a.reps // 2)
        r = {'N': n, 'rows': R, 'mean_len': R / n, 'max_len': int(np.diff(hb.row_off).max()), 'gflop_ragged': f / 1e9}
        for p, enc in encs.items():
            ws = torch.empty(enc.workspace_bytes(b), dtype=torch.uint8, device='cuda')
            out = torch.empty((n, W), device='cuda')
            ms = timed(lambda: enc.encode_batch(b, out=out, workspace=ws), reps)
            r['device_%s_ms' % p] = ms
            r['device_%s_tflops' % p] = f / (ms * 1e-3) / 1e12
            r['device_%s_peak_frac' % p] = f / (ms * 1e-3) / PEAK[p]
            del ws
        if not a.device_only:
            r['encoder_fp32_ms'] = timed(lambda: encs['fp32']({'caption': caps}), reps)
            from bert_ref import padded
            ids, mask = padded(hb.row_off, hb.ids)
            batches = []
            for s in range(0, n, a.ref_batch):
                m_ = mask[s:s + a.ref_batch]
                L = int(m_.sum(axis=1).max())
                batches.append((torch.from_numpy(ids[s:s + a.ref_batch, :L]).cuda(), torch.from_numpy(m_[:, :L]).cuda()))
            r['ref_path_ms'] = timed(lambda: [ref(i_, m_) for i_, m_ in batches], 1 if n >= 10000 else reps)
            theirs = torch.cat([ref(i_, m_) for i_, m_ in batches]).double()
            for p in precs:
                ours = encs[p].encode_batch(b).double()
                r['max_rel_diff_%s_vs_ref_path' % p] = float(((ours - theirs).norm(dim=1) / theirs.norm(dim=1)).max())
                r['speedup_device_%s_vs_ref' % p] = r['ref_path_ms'] / r['device_%s_ms' % p]
            r['speedup_encoder_vs_ref'] = r['ref_path_ms'] / r['encoder_fp32_ms']
        print(json.dumps(r), flush=True)
        rows.append(r)
    res = {'src_hash': source_hash(), 'device': torch.cuda.get_device_name(0), 'width': W, 'layers': LAYERS, 'heads': HEADS,
           'intermediate': INTER, 'ref_path': ref_name, 'rows': rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps({'src_hash': res['src_hash'], 'device': res['device'], 'ref_path': ref_name}))


if __name__ == '__main__':
    main()
