"""Times laff_fc_concat_backward (ops.fc_concat_backward) against the per-segment route it groups -- one
ops.fc_backward per dense segment and one ops.fc_gather_backward per CSR segment on the column windows, as
model.autograd._FcConcatFn.backward issues them -- and then one whole 'W2VVPP' training step against the same model restated with torch
modules.  Nominal W2VV++ sizes at batch 128:
    text    bigru 2,048 (dense, with dX: the GRU trains through it) + bag of words 7,811 (CSR, about 10 words a caption) + word2vec 500
            -> 2,048
    video   2,048 + 2,048 -> 2,048, no dX

    python tools/concat_backward_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Both routes are first held to the
element-by-element bounds of tests/fc_bwd_ref.py against float64 on the concatenated input; a miss ends the run with exit status 1 and
nothing is timed.  Times are HIP events around K back-to-back calls after a warm-up, five such windows per row, next to the host wall
time of the same windows (tools/train_step_time.py's windows); one JSON line per row with ms (the median window), spread [min, max],
host_ms and the library launches of one call by entry point.  The comparison partner of the grouped call is the per-segment route,
timed in the same process."""
import json
import os
import sys

from train_step_time import Counter, windows
from train_time import run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 128, 2048
TOWERS = {'text': ((2048, 'd', True), (7811, 'c', False), (500, 'd', False)), 'video': ((2048, 'd', False), (2048, 'd', False))}
VID = {'resnext': 2048, 'ircsn': 2048}
TXT = {'rnn': 2048, 'bow': 7811, 'w2v': 500}


def bag_of_words(n, dk, g, words=10):
    import numpy as np
    import torch
    rows = [np.sort(g.choice(dk, size=words, replace=False)) for _ in range(n)]
    crow = torch.arange(0, words * n + 1, words, dtype=torch.int32)
    col = torch.from_numpy(np.concatenate(rows).astype(np.int32))
    return torch.sparse_csr_tensor(crow, col, torch.ones(words * n), size=(n, dk))


def tower_problem(segs, dev):
    import numpy as np
    import torch
    from laff_amd import ops
    g = np.random.default_rng(5)
    gen = torch.Generator().manual_seed(5)
    dense, device_segs = [], []
    for w, kind, _ in segs:
        if kind == 'c':
            csr = bag_of_words(N, w, g)
            dense.append(csr.to_dense())
            device_segs.append(tuple(t.to(dev) for t in ops.csr_transpose(csr)))
        else:
            dense.append(torch.randn(N, w, generator=gen))
            device_segs.append(dense[-1].to(dev))
    K = sum(w for w, _, _ in segs)
    W = torch.randn(D, K, generator=gen) / K ** 0.5
    a = torch.tanh(torch.randn(N, D, generator=gen))
    da = torch.randn(N, D, generator=gen)
    return dict(segs=segs, dense=dense, dev=device_segs, W=W, a=a, da=da, K=K, want_dx=[dx for _, _, dx in segs])


def routes(p, dev):
    """(the grouped call, the per-segment route) as closures writing (dxs, dw, db) into their own buffers."""
    import torch
    from laff_amd import ops
    W, a, da = p['W'].to(dev), p['a'].to(dev), p['da'].to(dev)
    cols = [sum(w for w, _, _ in p['segs'][:j]) for j in range(len(p['segs']))]

    def buffers():
        return ([torch.empty(N, w, device=dev) if dx else None for w, _, dx in p['segs']], torch.empty(D, p['K'], device=dev),
                torch.empty(D, device=dev))
    out_g, out_s = buffers(), buffers()

    def grouped():
        ops.fc_concat_backward(p['dev'], W, a, da, 'tanh', want_dx=p['want_dx'], out=out_g)

    def per_segment():
        dxs, dw, db = out_s
        for j, ((w, kind, dx), x) in enumerate(zip(p['segs'], p['dev'])):
            window, first = dw[:, cols[j]:cols[j] + w], db if j == 0 else None
            if kind == 'c':
                ops.fc_gather_backward(x, N, w, a, da, 'tanh', want_dw=True, want_db=first is not None, out=(window, first))
            else:
                ops.fc_backward(x, W[:, cols[j]:cols[j] + w], a, da, 'tanh', want_dx=dx, want_dw=True, want_db=first is not None,
                                out=(dxs[j], window, first))
    return (grouped, out_g), (per_segment, out_s)


def within_bounds(p, out, label):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import fc_bwd_ref as R
    x = torch.cat(p['dense'], 1)
    rdx, rdw, rdb = R.backward(x, p['W'], p['a'], p['da'], 'tanh')
    bdx, bdw, bdb = R.bounds(x, p['W'], p['da'])
    dxs, dw, db = out
    torch.cuda.synchronize()
    ok = bool(np.all(np.abs(dw.cpu().double().numpy() - rdw) <= bdw)) and bool(np.all(np.abs(db.cpu().double().numpy() - rdb) <= bdb))
    col = 0
    for (w, _, _), dx in zip(p['segs'], dxs):
        if dx is not None:
            ok = ok and bool(np.all(np.abs(dx.cpu().double().numpy() - rdx[:, col:col + w]) <= bdx[:, col:col + w]))
        col += w
    if not ok:
        print('%s misses the float64 bound: nothing is timed' % label, file=sys.stderr)
    return ok


class TorchW2VVPP:
    """The same model from torch modules (Linear on the concatenated input, Tanh, Dropout, BatchNorm1d; the margin loss with
    max_violation, clip_grad_norm_, torch.optim.RMSprop), parameters copied from the library's model."""

    def __init__(self, model, cfg, dropout):
        import torch
        from torch import nn
        self.torch, self.cfg = torch, cfg
        self.nets = {}
        for side, t in (('vis', model.vis_net), ('txt', model.txt_net.transformer)):
            lin = nn.Linear(t.fc1.in_features, t.fc1.out_features)
            lin.load_state_dict(t.fc1.state_dict())
            bn = nn.BatchNorm1d(t.out_features)
            bn.load_state_dict(t.bn1.state_dict())
            self.nets[side] = nn.Sequential(lin, nn.Tanh(), *([nn.Dropout(dropout)] if dropout else []), bn).to(t.fc1.weight.device).train()
        self.params = [p for n in self.nets.values() for p in n.parameters()]
        self.opt = torch.optim.RMSprop(self.params, lr=cfg.lr)

    def loss(self, vis, txt):
        torch, F = self.torch, self.torch.nn.functional
        v, t = self.nets['vis'](torch.cat(vis, 1)), self.nets['txt'](torch.cat(txt, 1))
        s = F.normalize(v, dim=1) @ F.normalize(t, dim=1).T
        eye = torch.eye(s.shape[0], dtype=torch.bool, device=s.device)
        return (self.cfg.margin + s - s.diag()[None, :]).clamp(min=0).masked_fill(eye, 0).max(0)[0].sum()

    def step(self, vis, txt):
        self.opt.zero_grad()
        loss = self.loss(vis, txt)
        loss.backward()
        self.torch.nn.utils.clip_grad_norm_(self.params, self.cfg.grad_clip)
        self.opt.step()
        return loss


def build(dropout, dev):
    import torch
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    cfg = make_config(VID, TXT, D, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat', batch_norm=True, dropout=dropout)
    torch.manual_seed(1)
    return get_model('W2VVPP', dev, cfg).train(), cfg


def child(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    rows = []
    for name, segs in TOWERS.items():
        p = tower_problem(segs, dev)
        (grouped, out_g), (per_segment, out_s) = routes(p, dev)
        for label, fn, out in (('fc_concat_backward', grouped, out_g), ('per_segment', per_segment, out_s)):
            ops.profiler = counter = Counter()
            fn()
            ops.profiler = None
            if not within_bounds(p, out, '%s %s' % (name, label)):
                return 1
            rows.append(('%s %s' % (name, label), fn, {'calls': counter.names}))
    # one whole 'W2VVPP' step: the two routes compute the same loss (dropout off) before anything is timed
    g = torch.Generator().manual_seed(7)
    vis = {k: torch.randn(N, d, generator=g).to(dev) for k, d in VID.items()}
    bow = bag_of_words(N, TXT['bow'], np.random.default_rng(9))
    bow_dev = bow.to(dev)
    bow_dev.laff_csc = tuple(t.to(dev) for t in ops.csr_transpose(bow))
    txt = {'rnn_encoding': torch.randn(N, TXT['rnn'], generator=g).to(dev), 'bow_encoding': bow_dev,
           'w2v_encoding': torch.randn(N, TXT['w2v'], generator=g).to(dev)}
    txt_dense = [txt['rnn_encoding'], bow.to_dense().to(dev), txt['w2v_encoding']]

    def data():
        return {'vis_feats': dict(vis), 'captions': dict(txt, caption=[''] * N), 'vis_frame_feat_dict': {}}
    model, cfg = build(0, dev)
    ref = TorchW2VVPP(model, cfg, 0)
    model.enable_training()
    ours = float(model.cal_foward(data())[0].detach())
    theirs = float(ref.loss(list(vis.values()), txt_dense).detach())
    if not abs(ours - theirs) <= 1e-4 * abs(theirs):
        print('the routes differ: loss %.9g against %.9g: nothing is timed' % (ours, theirs), file=sys.stderr)
        return 1
    model, cfg = build(0.2, dev)
    ref = TorchW2VVPP(model, cfg, 0.2)
    model.enable_training()
    ops.profiler = counter = Counter()
    model(data())
    ops.profiler = None
    rows.append(('W2VVPP step laff_amd', lambda: model(data()), {'launches': sum(counter.names.values()), 'calls': counter.names}))
    rows.append(('W2VVPP step torch', lambda: ref.step(list(vis.values()), txt_dense), {}))
    timed = [(name, windows(fn, iters), extra) for name, fn, extra in rows]
    timed += [(name + ' again', windows(fn, iters), {}) for name, fn, _ in rows[:4]]           # the spread of a repeat in the same process
    for name, (ms, host), extra in timed:
        print(json.dumps(dict({'row': name, 'N': N, 'D': D, 'ms': round(ms[2], 4), 'spread': [round(ms[0], 4), round(ms[-1], 4)],
                               'host_ms': round(host, 4)}, **extra)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 50))
