"""Times the whole training step of the 'LAFF' model, enable_training() + model(train_data), at the LAFF shape:
batch 128, D 4096, H 8, four video and four text features, one of them a no-transform feature on each side, dropout 0.2, BatchNorm,
margin ranking loss with max_violation, RMSprop with grad_clip 2.

    python tools/train_step_time.py [--timeout SECONDS] [--iters K]

The measurement runs once, in a child process that is ended after --timeout seconds.  Times are HIP events around K back-to-back steps
after a warm-up, five such windows per route, next to the host wall time of the same windows.  One JSON line per row:
    laff_amd                 this library's step, device_norm=True; 'launches' counts the library's launches of one step by entry point
    torch                    the same model restated with torch modules on the same GPU (Linear, Tanh, Dropout, BatchNorm1d, a softmax
                             attention per head, the per-head margin loss, clip_grad_norm_, torch.optim.RMSprop)
    laff_amd_all_fc          a configuration without no-transform features (every feature through an fc), device_norm=True, and
    laff_amd_all_fc_torch_norm   the same with device_norm=False (torch's dropout and BatchNorm1d): the no-transform feature trains
                             with device_norm only, so the pair is timed where the configuration allows both
Per row: ms (the median window), spread [min, max], host_ms (wall time per step of the median window).
Before anything is timed the first step's loss of the library and of the torch restatement, from the same parameters and inputs with
dropout off, have to agree within 1e-4 relative; a difference ends the run with exit status 1.
"""
import json
import os
import sys
import time

from train_time import run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, H = 128, 4096, 8
VID = {'clip_ft': 512, 'x3d': 2048, 'ircsn': 2048, 'timesformer': 768}
TXT = {'rnn': 2048, 'bow': 8192, 'w2v': 500, 'CLIP': 512}
KEYS = {'rnn_encoder': 'rnn_encoding', 'bow_encoder': 'bow_encoding', 'w2v_encoder': 'w2v_encoding', 'CLIP_encoder': 'CLIP_encoding'}


def windows(fn, iters):
    """(sorted device ms per call of five windows of `iters` calls after a warm-up of 3, host wall ms per call of the median window)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append((t0.elapsed_time(t1) / iters, (time.perf_counter() - w0) * 1e3 / iters))
    out.sort()
    return [d for d, _ in out], out[2][1]


class Counter:
    """ops.profiler: counts the library's launches by entry point."""

    def __init__(self):
        self.names = {}

    def begin(self, name):
        self.names[name] = self.names.get(name, 0) + 1

    def end(self, name):
        pass


def build(no_transform, dropout, dev):
    import torch
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    cfg = make_config(VID, TXT, D, H, 'LAFF', vis_no_transform=['clip_ft'] if no_transform else [],
                      txt_no_transform=['CLIP_encoder'] if no_transform else [], batch_norm=True, with_ave=True, dropout=dropout)
    cfg.clip_opt = dict(cfg.clip_opt, transform_dropout=0.0 if no_transform else dropout)     # (a tiled layer takes no dropout)
    torch.manual_seed(1)
    return get_model('LAFF', dev, cfg).train(), cfg


class TorchLaff:
    """The same model from torch modules, parameters copied from the library's model."""

    def __init__(self, model, cfg, dropout):
        import torch
        from torch import nn
        self.torch, self.cfg = torch, cfg
        self.sides = {}
        for side, tower, names, attn in (('vis', model.vis_net.VisMutiTransformNet, list(VID), model.vis_net.attention_layer),
                                         ('txt', model.txt_net.transform_layer, [n + '_transform' for n in model.txt_net.encoder_name_list],
                                          model.txt_net.attention_layer)):
            layers = []
            for name in names:
                t = getattr(tower, name)
                seq = []
                if t.fc1 is not None:
                    lin = nn.Linear(t.fc1.in_features, t.fc1.out_features)
                    lin.load_state_dict(t.fc1.state_dict())
                    seq += [lin, nn.Tanh()]
                    if dropout:
                        seq.append(nn.Dropout(dropout))
                bn = nn.BatchNorm1d(t.out_features)
                bn.load_state_dict(t.bn1.state_dict())
                layers.append((t.fc1 is None, nn.Sequential(*seq, bn).to(model_device(model)).train()))
            heads = [(nn.Linear(D // H, 1).to(model_device(model)), a.global_emb_weight_net.weight.item()) for a in attn.attention_layer]
            for (lin, _), a in zip(heads, attn.attention_layer):
                lin.load_state_dict(a.embedding_common[0].state_dict())
            self.sides[side] = (layers, heads)
        self.params = [p for layers, heads in self.sides.values() for _, m in layers for p in m.parameters()] + \
                      [p for _, heads in self.sides.values() for lin, _ in heads for p in lin.parameters()]
        self.opt = torch.optim.RMSprop(self.params, lr=cfg.lr)

    def tower(self, side, feats):
        torch = self.torch
        layers, heads = self.sides[side]
        planes = torch.stack([m(x.repeat(1, H) if tile else x) for (tile, m), x in zip(layers, feats)], 1)       # (N, L, D)
        X = planes.view(planes.shape[0], planes.shape[1], H, D // H)
        out = []
        for h, (lin, gw) in enumerate(heads):
            x = X[:, :, h]
            a = torch.softmax(lin(x), dim=1)
            g = (a * x).sum(1) + gw * x.sum(1)                  # Attention_1 adds gw * mean to each of the L terms
            out.append(g / (g.pow(2).sum(1, keepdim=True).sqrt() + 1e-14))
        return torch.stack(out, 1)

    def loss(self, vis, txt):
        torch, cfg = self.torch, self.cfg
        t, v = self.tower('txt', txt), self.tower('vis', vis)
        total = 0.0
        eye = torch.eye(t.shape[0], dtype=torch.bool, device=t.device)
        for h in range(H):
            s = torch.nn.functional.normalize(v[:, h], dim=1) @ torch.nn.functional.normalize(t[:, h], dim=1).T
            cost = (cfg.margin + s - s.diag()[None, :]).clamp(min=0).masked_fill(eye, 0)
            total = total + cost.max(0)[0].sum()
        return total

    def step(self, vis, txt):
        self.opt.zero_grad()
        loss = self.loss(vis, txt)
        loss.backward()
        self.torch.nn.utils.clip_grad_norm_(self.params, self.cfg.grad_clip)
        self.opt.step()
        return loss


def model_device(model):
    return next(model.parameters()).device


def child(iters):
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import ops
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(7)
    vis = {k: torch.randn(N, d, generator=g).to(dev) for k, d in VID.items()}
    txt = {k: torch.randn(N, TXT[k.split('_')[0]], generator=g).to(dev) for k in KEYS}

    def data():
        cap = {'caption': [''] * N}
        cap.update({KEYS[k]: v for k, v in txt.items()})
        return {'vis_feats': dict(vis), 'captions': cap, 'vis_frame_feat_dict': {}}

    # the two routes compute the same loss (dropout off) before anything is timed
    model, cfg = build(True, 0, dev)
    ref = TorchLaff(model, cfg, 0)
    model.enable_training()
    ours = float(model.cal_foward(data())[0].detach())
    theirs = float(ref.loss(list(vis.values()), [txt[k] for k in model.txt_net.encoder_name_list]).detach())
    if not abs(ours - theirs) <= 1e-4 * abs(theirs):
        print('the routes differ: loss %.9g against %.9g: nothing is timed' % (ours, theirs), file=sys.stderr)
        return 1
    rows = []
    model, cfg = build(True, 0.2, dev)
    ref = TorchLaff(model, cfg, 0.2)
    model.enable_training()
    ops.profiler = counter = Counter()
    model(data())
    ops.profiler = None
    rows.append(('laff_amd', lambda: model(data()), {'launches': sum(counter.names.values()), 'by_entry_point': counter.names}))
    order = list(model.txt_net.encoder_name_list)
    rows.append(('torch', lambda: ref.step(list(vis.values()), [txt[k] for k in order]), {}))
    fc_on = build(False, 0.2, dev)[0].enable_training(device_norm=True)
    fc_off = build(False, 0.2, dev)[0].enable_training(device_norm=False)
    rows.append(('laff_amd_all_fc', lambda: fc_on(data()), {}))
    rows.append(('laff_amd_all_fc_torch_norm', lambda: fc_off(data()), {}))
    timed = [(name, windows(fn, iters), extra) for name, fn, extra in rows]
    timed += [(name + '_again', windows(fn, iters), {}) for name, fn, _ in rows[:2]]            # the spread of a repeat in the same process
    for name, (ms, host), extra in timed:
        print(json.dumps(dict({'row': name, 'shape': {'N': N, 'D': D, 'H': H, 'vid': VID, 'txt': TXT}, 'ms': round(ms[2], 4),
                               'spread': [round(ms[0], 4), round(ms[-1], 4)], 'host_ms': round(host, 4)}, **extra)), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 50))
