"""A float64 torch restatement of the reference's BertTxtEncoder.forward (model/model.py:437-466: transformers' BertModel,
pooler_output), run the way the reference runs it: captions padded to the batch's longest with the dense key mask.  So it checks the
ragged layout of laff_bert_encode as well.  The checker of tests/test_bert_host.py and tests/test_gpu_bert.py; runs on the CPU for
the fixture and on the device (float64) at full size.  RefBert is the same computation in fp32 / fp16: the reference-shaped torch
path that tools/bench_bert.py times and tests/test_gpu_bert.py reports beside the device's fp16 error."""
import math

import numpy as np
import torch


def full_bert_sd(z):
    """The fixture's BertModel state dict (stored as int8 q * 2**e, the exact values the reference ran on), bare names."""
    e = z.sub('e/')
    return {k: (q.astype(np.float32) * np.float32(2.0 ** int(e[k]))) for k, q in z.sub('q/').items()}


def padded(row_off, ids):
    """A ragged batch (row_off [N+1], ids [R]) -> (ids [N, Lmax] padded with 0, mask [N, Lmax]) as the reference's tokenizer pads."""
    row_off, ids = np.asarray(row_off), np.asarray(ids)
    lens = np.diff(row_off)
    L = int(lens.max()) if lens.size else 1
    out, mask = np.zeros((len(lens), L), np.int64), np.zeros((len(lens), L), np.int64)
    for i, n in enumerate(lens):
        out[i, :n] = ids[row_off[i]:row_off[i + 1]]
        mask[i, :n] = 1
    return out, mask


def _tensors(sd, dtype, device):
    return {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v)).to(device=device, dtype=dtype)
            for k, v in sd.items()}


def _ln(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _layers(t):
    return len(set(k.split('.')[2] for k in t if k.startswith('encoder.layer.')))


def _forward(t, ids, mask, eps, ln):
    """BertModel(input_ids, attention_mask, token_type_ids = 0)['pooler_output'] on padded ids [n, L] with the key mask."""
    W = t['embeddings.word_embeddings.weight'].shape[1]
    H = W // 64
    n, L = ids.shape
    x = t['embeddings.word_embeddings.weight'][ids] + t['embeddings.token_type_embeddings.weight'][0]
    x = ln(x + t['embeddings.position_embeddings.weight'][:L], t['embeddings.LayerNorm.weight'], t['embeddings.LayerNorm.bias'], eps)
    bias = torch.zeros((n, 1, 1, L), dtype=x.dtype, device=x.device).masked_fill(mask[:, None, None, :] == 0, float('-inf'))
    for i in range(_layers(t)):
        p = 'encoder.layer.%d.' % i

        def lin(v, name):
            return v @ t[p + name + '.weight'].T + t[p + name + '.bias']
        q, k, v = (lin(x, 'attention.self.' + s).reshape(n, L, H, 64).transpose(1, 2) for s in ('query', 'key', 'value'))
        att = torch.softmax(q @ k.transpose(-1, -2) / 8.0 + bias, dim=-1)
        a = (att @ v).transpose(1, 2).reshape(n, L, W)
        x = ln(x + lin(a, 'attention.output.dense'), t[p + 'attention.output.LayerNorm.weight'], t[p + 'attention.output.LayerNorm.bias'],
               eps)
        hdn = lin(x, 'intermediate.dense')
        hdn = 0.5 * hdn * (1.0 + torch.erf(hdn / math.sqrt(2.0)))
        x = ln(x + lin(hdn, 'output.dense'), t[p + 'output.LayerNorm.weight'], t[p + 'output.LayerNorm.bias'], eps)
    return torch.tanh(x[:, 0] @ t['pooler.dense.weight'].T + t['pooler.dense.bias'])


def encode64(ids, mask, sd, eps=1e-12, device='cpu', chunk=64):
    """ids / mask [N, L] (padded, as the reference's tokenizer returns them), sd: the bare BertModel state dict -> (N, hidden) float64
    numpy.  Chunks of `chunk` captions, each padded to its longest (the mask makes any padding exact)."""
    t = _tensors(sd, torch.float64, device)
    ids, mask = np.asarray(ids), np.asarray(mask)
    outs = []
    for s in range(0, len(ids), chunk):
        m = mask[s:s + chunk]
        L = max(int(m.sum(axis=1).max()), 1)
        i_ = torch.as_tensor(ids[s:s + chunk, :L], dtype=torch.long, device=device)
        m_ = torch.as_tensor(m[:, :L], dtype=torch.long, device=device)
        outs.append(_forward(t, i_, m_, eps, _ln).cpu().numpy())
    return np.concatenate(outs) if outs else np.zeros((0, sd['pooler.dense.bias'].shape[0]))


class RefBert(object):
    """The reference's shape on the device in torch: every caption of a batch padded to the longest, the dense key mask, all rows of
    every layer, in `dtype` (torch.float32: what the reference runs; torch.float16: .half() of the same), torch's LayerNorm."""

    def __init__(self, sd, dtype=torch.float32, device='cuda', eps=1e-12):
        self.t, self.eps = _tensors(sd, dtype, device), eps

    def _ln(self, x, w, b, eps):
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps)

    @torch.no_grad()
    def __call__(self, ids, mask):
        return _forward(self.t, ids, mask, self.eps, self._ln)
