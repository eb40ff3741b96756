"""Retrieval post-processing of the reference's model/ReRank.py on the device: `re_ranking` (k-reciprocal encoding, Zhong et al.,
CVPR 2017; ReRank.py:19-104) and `re_ranking_tkb_simple` (ReRank.py:107-159), same names and signatures.

Inputs are fp32 SIMILARITY matrices (despite the parameter names, as in the reference): numpy arrays or device tensors; the result is
of the same kind.  There is no CPU path: a numpy input is copied to the device and only the [Q, G] result comes back.
`Concept_re_ranking` / `process_query` (nltk, concept files) are out of scope.
"""
import numpy as np
import torch

from .. import loss as _loss
from .. import ops

#: bytes of re-ranking workspace one launch set may take: more problems than fit are run in chunks
WORKSPACE_BUDGET = 1 << 30


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _blocks(q_g_dist, q_q_dist, g_g_dist):
    """the three blocks as fp32 device tensors + whether the caller gave numpy"""
    host = not isinstance(q_g_dist, torch.Tensor)
    out = []
    for name, a in (('q_g_dist', q_g_dist), ('q_q_dist', q_q_dist), ('g_g_dist', g_g_dist)):
        if isinstance(a, torch.Tensor) != (not host):
            raise TypeError('re-ranking inputs must be all numpy arrays or all device tensors')
        if host:
            a = np.ascontiguousarray(a, dtype=np.float32)
        elif a.dtype != torch.float32 or not a.is_cuda:
            raise TypeError('%s must be an fp32 device tensor: laff_amd has no CPU path' % name)
        if a.ndim != 2:
            raise ValueError('%s must be 2-D, got shape %s' % (name, tuple(a.shape)))
        out.append(a)
    Q, G = out[0].shape
    if tuple(out[1].shape) != (Q, Q) or tuple(out[2].shape) != (G, G):
        raise ValueError('re-ranking blocks must be q_g [Q, G], q_q [Q, Q], g_g [G, G]; got %s, %s, %s'
                         % tuple(tuple(a.shape) for a in out))
    return out, host


def re_ranking_batched(problems, k1=20, k2=6, lambda_value=0.3, budget_bytes=None):
    """`re_ranking` of many independent problems, each (q_g [Q, G], q_q [Q, Q], g_g [G, G]) fp32 device tensors of its own size:
    as many problems per launch set as fit `budget_bytes` of workspace (WORKSPACE_BUDGET).  Returns the list of [Q, G] results; a
    problem's result does not depend on how it was batched."""
    budget = WORKSPACE_BUDGET if budget_bytes is None else int(budget_bytes)
    sizes = [tuple(p[0].shape) for p in problems]
    need = [ops.rerank_workspace_bytes([s], k1, k2) for s in sizes]          # raises on sizes / k1 / k2 outside the limits
    outs, lo = [], 0
    while lo < len(problems):
        hi, total = lo + 1, need[lo]
        while hi < len(problems) and total + need[hi] <= budget:
            total += need[hi]
            hi += 1
        outs.extend(ops.rerank_run(problems[lo:hi], k1, k2, lambda_value))
        lo = hi
    return outs


def re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3):
    """k-reciprocal re-ranking of Q queries against G gallery items (ReRank.py:19-104): the [Q, G] fp32 blend of the Jaccard
    distance of the k-reciprocal encodings and the normalised original distance, smaller = closer.  fp32 throughout; the step-by-step
    definition is in include/laff_hip.h (laff_rerank_run).  Supported: k1 <= 32, k2 <= min(8, k1 + 1), k1 + 1 <= Q + G <= 4096;
    anything else raises.  Near-ties among the k1 + 2 nearest neighbours of an item resolve to the lower index."""
    (qg, qq, gg), host = _blocks(q_g_dist, q_q_dist, g_g_dist)
    ops.rerank_workspace_bytes([tuple(qg.shape)], k1, k2)                    # the limits, before anything moves to the device
    if host:
        dev = _device()
        qg, qq, gg = (torch.from_numpy(a).to(dev) for a in (qg, qq, gg))
    out = ops.rerank_run([(qg.contiguous(), qq.contiguous(), gg.contiguous())], k1, k2, lambda_value)[0]
    return out.cpu().numpy() if host else out


def tkb_counts(g_g_dist, k1=20):
    """count[v] = 1 + the number of rows of g_g whose k1 best columns hold v (int32 device tensor) -- the dictionary of
    ReRank.py:121-132."""
    G = g_g_dist.shape[0]
    nn, _ = ops.topk_rows(g_g_dist, k1)
    empty = torch.empty((0, 1), dtype=torch.int32, device=g_g_dist.device)
    return ops.rerank_tkb(nn, empty, G)[1]


def re_ranking_tkb_simple(q_g_dist, q_q_dist, g_g_dist, topK=3000, k1=20):
    """ReRank.py:107-159: log(count + 1) on the topK best columns of every q_g row and 0 elsewhere, rows L2-normalised, where
    count[v] = 1 + the number of gallery rows that have v among their k1 most similar.  One top-K pass per matrix, one histogram pass,
    one scatter; q_q_dist is unused, as in the reference.  Needs 1 <= k1 <= G."""
    (qg, _, gg), host = _blocks(q_g_dist, q_q_dist, g_g_dist)
    Q, G = qg.shape
    k1, K = int(k1), min(int(topK), G)
    if not 1 <= k1 <= G or K < 1:
        raise ValueError('re_ranking_tkb_simple: need 1 <= k1 <= G and topK >= 1 (k1=%d topK=%d G=%d)' % (k1, topK, G))
    if host:
        dev = _device()
        qg, gg = torch.from_numpy(qg).to(dev), torch.from_numpy(gg).to(dev)
    nn, _ = ops.topk_rows(gg.contiguous(), k1)
    cand, _ = ops.topk_rows(qg.contiguous(), K)
    out, _ = ops.rerank_tkb(nn, cand, G)
    out = _loss.l2norm(out)
    return out.cpu().numpy() if host else out
