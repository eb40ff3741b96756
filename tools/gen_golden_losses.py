#!/usr/bin/env python
"""Golden vectors for the dual-softmax and score-matrix margin criteria, from the REAL reference.

Runs only in the build container: it imports loss.py from /root/reference (read-only; the module needs nothing but torch and
numpy, so it is imported directly) and writes DATA only:

    tests/golden/dsl_loss.npz        loss.DualSoftmaxLoss (loss.py:291-310), forward + autograd
    tests/golden/margin_scores.npz   loss.MarginRankingLossWithScore (loss.py:138-200), forward + autograd

Every case holds its seeded inputs, the reference's fp32 loss and gradients, and e_ref: how far those fp32 results lie from the
float64 restatement of tests/loss_ref.py on the same inputs -- [loss (relative to max(1, |loss|)), gradients (absolute, element-wise
maximum)].  A test that compares something else with the restatement takes its bound from there.

    python tools/gen_golden_losses.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
REF = '/root/reference'
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import loss_ref  # noqa: E402

sys.path.insert(0, REF)
import loss as ref_loss  # noqa: E402  (the reference's loss.py)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def save(name, **arrays):
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def rel(a, b):
    return abs(float(a) - float(b)) / max(1.0, abs(float(b)))


def correlated(g, B, H, d):
    """Matched pairs share a latent, so the diagonal of the score matrix dominates as it does in training."""
    z = f32(g.normal(0, 1, (B, 16)))
    P = f32(g.normal(0, 1, (16, H * d)))
    s = f32(z @ P + 1.5 * g.normal(0, 1, (B, H * d))).reshape(B, H, d)
    im = f32(z @ P + 1.5 * g.normal(0, 1, (B, H * d))).reshape(B, H, d)
    return s, im


def gen_dsl():
    g = np.random.default_rng(2911)
    arrays, cases = {}, []
    shapes = [((B, d), temp) for (B, d) in ((1, 8), (2, 5), (3, 7), (17, 36)) for temp in (1000, 0.05)] + [((5, 3, 12), 1000)]
    crit = ref_loss.DualSoftmaxLoss()
    for ci, (shape, temp) in enumerate(shapes):
        k = 'c%d' % ci
        B, H, d = (shape[0], 1, shape[1]) if len(shape) == 2 else shape
        s_np, im_np = correlated(g, B, H, d)
        s = torch.tensor(s_np.reshape(shape), requires_grad=True)
        im = torch.tensor(im_np.reshape(shape), requires_grad=True)
        if len(shape) == 2:
            total = crit(s, im, temp)
        else:
            total = 0
            for h in range(H):                                   # model/model.py:2037-2039
                total = total + crit(s[:, h, :], im[:, h, :], temp)
        total.backward()
        l64, ds64, di64 = loss_ref.dsl(s.detach().numpy(), im.detach().numpy(), temp)
        arrays[k + '/s'] = s.detach().numpy()
        arrays[k + '/im'] = im.detach().numpy()
        arrays[k + '/loss'] = np.float32(total.item())
        arrays[k + '/d_s'] = s.grad.numpy()
        arrays[k + '/d_im'] = im.grad.numpy()
        arrays[k + '/e_ref'] = np.array([rel(total.item(), l64),
                                         max(np.abs(s.grad.numpy() - ds64).max(), np.abs(im.grad.numpy() - di64).max())])
        cases.append(dict(key=k, shape=list(shape), temp=temp))
        print(k, shape, temp, 'loss %.6g' % total.item(), 'e_ref', arrays[k + '/e_ref'])
    arrays['cases'] = np.array(json.dumps(cases))
    save('dsl_loss', **arrays)


def gen_margin_scores():
    g = np.random.default_rng(2912)
    arrays, cases = {}, []
    combos = [(False, 'sum'), (False, 'mean'), (True, 'sum'), (True, 'mean')]
    dirs = ['i2t', 't2i', 'bidir']
    ci = 0
    for bi, B in enumerate((1, 2, 9)):
        for qi, (maxv, style) in enumerate(combos):
            direction = dirs[(qi + bi) % 3]
            margin = 0.2
            for _ in range(100):                                 # every decision well clear of flipping between fp32 and float64
                sc = f32(0.6 * np.eye(B) + g.uniform(-0.5, 0.5, (B, B)))
                if loss_ref.margin_scores_slack(sc, margin, maxv, direction) >= 1e-4:
                    break
            else:
                raise RuntimeError('no draw with every decision 1e-4 clear')
            k = 'c%d' % ci
            ci += 1
            score = torch.tensor(sc, requires_grad=True)
            crit = ref_loss.MarginRankingLossWithScore(margin=margin, max_violation=maxv, cost_style=style, direction=direction)
            total = crit(score)
            total.backward()
            l64, d64 = loss_ref.margin_scores(sc, margin, maxv, style, direction)
            arrays[k + '/score'] = sc
            arrays[k + '/loss'] = np.float32(total.item())
            arrays[k + '/d_score'] = score.grad.numpy() if score.grad is not None else np.zeros_like(sc)
            arrays[k + '/e_ref'] = np.array([rel(total.item(), l64), np.abs(arrays[k + '/d_score'] - d64).max()])
            cases.append(dict(key=k, B=B, margin=margin, max_violation=maxv, cost_style=style, direction=direction))
            print(k, B, maxv, style, direction, 'loss %.6g' % total.item(), 'e_ref', arrays[k + '/e_ref'])
    arrays['cases'] = np.array(json.dumps(cases))
    save('margin_scores', **arrays)


if __name__ == '__main__':
    torch.manual_seed(0)
    gen_dsl()
    gen_margin_scores()
