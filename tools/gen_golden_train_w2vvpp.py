#!/usr/bin/env python3
"""tests/golden/train_step_w2vvpp.<case>[.<n>].npz: two training steps of the REAL reference's W2VV++ concat towers (the stub recipe
of tools/gen_golden.py, the step recipe of tools/gen_golden_train.py, the towers' config of tools/gen_golden_w2vvpp.py), in float32 and,
from the same initial state, in float64 (`model.double()`).

    python tools/gen_golden_train_w2vvpp.py

Reference symbols exercised (file:line relative to the reference tree): model/model.py:279-308 VisTransformNet, :552-726
MultiScaleTxtEncoder / MultiScaleTxtNet, :791-836 W2VVPP.__init__ (criterion, Adam / RMSprop with torch's default eps), :840-865
compute_loss on 2-D embeddings, :867-887 cal_foward, :964-1001 forward, :2501-2519 get_model; loss.py:68-135 MarginRankingLoss.

Arrays, name lists and scalars only.  Video features {resnext 96, x3d 48, ircsn 40}, pre-extracted text features {bow 30, w2v 50,
CLIP 64}, both towers to D = 64, B = 12, BatchNorm on, dropout 0 (the masks cannot be shared with the reference), lr 1e-4, grad_clip 2:
    i    'W2VVPP', rmsprop, max_violation=True, direction 't2i'
    ii   'w2vpp_mutivis_attention' with both attentions 'concat', adam, max_violation=False, direction 'bidir' -- the case that pins
         Adam's eps to torch's default 1e-8
Each case takes two steps on fresh input dicts, step 2 on other inputs.  Per step and per run: the embeddings and the loss, the raw
(unclipped) gradients of cal_foward + backward on a deep copy, their global norm, and after the step the state_dict (BatchNorm
statistics included) and the optimizer's state (RMSprop: square_avg; Adam: exp_avg, exp_avg_sq) and step.  The float64 run is stored as
arrays; of the float32 run the fixture keeps the loss and, per tensor, e32 = max |f32 - f64| / max |f64|, which is what the tests'
tolerance rule reads.

A seed is accepted when, before both steps, train_ref.hinge_slack of the float64 embeddings and the case's own slack (under
max_violation every top-2 gap as well) stay at least train_ref.HINGE_CLEAR from flipping and the float32 run takes the same
decisions; the search stops after 40 seeds.  The float64 restatement of the tests (tests/concat_tower_ref.py, tests/optim_ref.py) has
to reproduce the float64 run to 1e-12 before anything is written.
"""
import copy
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import gen_golden as G  # noqa: E402  (imports the reference)
import gen_golden_train as T  # noqa: E402
import gen_golden_w2vvpp as WV  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import concat_tower_ref  # noqa: E402
import optim_ref  # noqa: E402
import train_ref  # noqa: E402

mm = G.mm
VID_DIMS, TXT_DIMS = WV.VID_DIMS, WV.TXT_DIMS
D, N = 64, 12
CASES = {
    'i': dict(model='W2VVPP', optimizer='rmsprop', max_violation=True, direction='t2i'),
    'ii': dict(model='w2vpp_mutivis_attention', optimizer='adam', max_violation=False, direction='bidir'),
}
STATE_KEYS = {'rmsprop': ('square_avg',), 'adam': ('exp_avg', 'exp_avg_sq')}


def make_cfg(spec):
    cfg = WV.concat_cfg(D, True)
    cfg.dropout = 0
    cfg.optimizer = spec['optimizer']
    cfg.max_violation = spec['max_violation']
    cfg.direction = spec['direction']
    assert (cfg.loss, cfg.lr, cfg.grad_clip, cfg.margin, cfg.negative, cfg.activation) == ('mrl', 1e-4, 2, 0.2, False, 'tanh')
    return cfg


def make_inputs(g):
    vis = {k: G.f32(g.normal(0, 1, (N, d))) for k, d in VID_DIMS.items()}
    txt = {'bow_feature': G.f32((g.uniform(0, 1, (N, TXT_DIMS['bow'])) < 0.15).astype(np.float32)),
           'w2v_feature': G.f32(g.normal(0, 1, (N, TXT_DIMS['w2v']))), 'CLIP_encoding': G.f32(g.normal(0, 1, (N, TXT_DIMS['CLIP'])))}
    return vis, txt


def run(model, inputs, dtype, cfg):
    """Two steps of `model` (already of `dtype`); everything recorded as float64 numpy arrays / Python scalars."""
    out = []
    for step in (0, 1):
        rec = {}
        probe = copy.deepcopy(model)              # the embeddings, on a copy (a forward moves the running statistics)
        data = T.train_data(inputs[step], dtype)
        txt_emb = probe.txt_net(data['captions'])
        vis_emb = probe.vis_net(data['vis_feats'], txt_emb=txt_emb, vis_frame_feat_dict_input=None)
        assert txt_emb.dim() == vis_emb.dim() == 2
        rec['txt_emb'], rec['vis_emb'] = txt_emb.detach().double().numpy(), vis_emb.detach().double().numpy()
        rec['slack'], rec['decisions'] = T.decisions(txt_emb[:, None], vis_emb[:, None], cfg)
        rec['slack'] = min(rec['slack'], train_ref.hinge_slack(txt_emb, vis_emb, cfg.margin))
        probe = copy.deepcopy(model)              # the raw gradients, on another copy
        loss, _ = probe.cal_foward(T.train_data(inputs[step], dtype))
        loss.backward()
        rec['loss'] = float(loss.detach().double())
        grads = {k: p.grad for k, p in T.param_model(probe).items()}
        assert all(gr is not None for gr in grads.values())
        rec['grad'] = {k: gr.detach().double().numpy() for k, gr in grads.items()}
        rec['total_norm'] = float(np.sqrt(sum(float((gr ** 2).sum()) for gr in rec['grad'].values())))
        items = model(T.train_data(inputs[step], dtype))   # the step itself
        assert abs(float(items['triplet_loss'].detach().double()) - rec['loss']) <= 1e-6 * abs(rec['loss'])
        rec['sd'] = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in T.sd_of(model).items()}
        names = {id(p): k for k, p in model.named_parameters()}
        rec['state'], rec['opt_step'] = {}, {}
        for p, st in model.optimizer.state.items():
            k = names[id(p)]
            for sk in STATE_KEYS[cfg.optimizer]:
                rec['state'][sk + '/' + k] = st[sk].detach().double().clone().numpy()
            rec['opt_step'][k] = float(st['step'])
        out.append(rec)
    return out


def check_restatement(arrays, meta, r64):
    """tests/concat_tower_ref.py and tests/optim_ref.py reproduce the reference's float64 run to 1e-12."""
    for s in (1, 2):
        graph = concat_tower_ref.step_graph_of(arrays, meta, s)
        rec = r64[s - 1]
        assert T.rel(graph['txt_emb'].detach().numpy(), rec['txt_emb']) <= 1e-12 and T.rel(graph['vis_emb'].detach().numpy(), rec['vis_emb']) <= 1e-12
        assert abs(float(graph['loss'].detach()) - rec['loss']) <= 1e-12 * abs(rec['loss'])
        for k, v in rec['grad'].items():
            assert T.rel(graph['grads'][k].numpy(), v) <= 1e-12, k
        names = sorted(rec['grad'])
        before = concat_tower_ref.tower_ref.sub(arrays, 'sd0/') if s == 1 else r64[s - 2]['sd']
        grads = [rec['grad'][k] for k in names]
        c = optim_ref.clip_coef(optim_ref.total_norm(grads), meta['grad_clip'])
        params = [before[k] for k in names]
        zeros = [np.zeros_like(g) for g in grads]
        if meta['optimizer'] == 'rmsprop':
            sq = zeros if s == 1 else [r64[s - 2]['state']['square_avg/' + k] for k in names]
            p2, s2 = optim_ref.rmsprop(params, grads, sq, meta['lr'], meta['alpha'], meta['eps'], 0.0, c)
            new = {'square_avg': s2}
        else:
            m, v = (zeros, zeros) if s == 1 else ([r64[s - 2]['state'][n + '/' + k] for k in names] for n in ('exp_avg', 'exp_avg_sq'))
            p2, m2, v2 = optim_ref.adam(params, grads, m, v, meta['lr'], 0.9, 0.999, meta['eps'], 0.0, s, c)
            new = {'exp_avg': m2, 'exp_avg_sq': v2}
        for i, k in enumerate(names):
            assert T.rel(p2[i], rec['sd'][k]) <= 1e-12, k
            for sk, vals in new.items():
                assert T.rel(vals[i], rec['state'][sk + '/' + k]) <= 1e-12, (sk, k)


def build_case(key, spec, first_seed, tries=40):
    cfg = make_cfg(spec)
    for seed in range(first_seed, first_seed + tries):
        g = G.rng(seed)
        torch.manual_seed(seed)
        model = mm.get_model(spec['model'], torch.device('cpu'), cfg)
        assert type(model.vis_net).__name__ == 'VisTransformNet' and type(model.txt_net).__name__ == 'MultiScaleTxtNet'
        WV.plug(model)
        G.randomize_model(model, g)
        model.train()
        inputs = [make_inputs(g), make_inputs(g)]
        sd0 = {k: v.numpy().copy() for k, v in T.sd_of(model).items()}
        r64 = run(copy.deepcopy(model).double(), inputs, torch.float64, cfg)
        r32 = run(copy.deepcopy(model), inputs, torch.float32, cfg)
        slack = min(r['slack'] for r in r64)
        same = all(np.array_equal(a['decisions'], b['decisions']) for a, b in zip(r32, r64))
        print('case %s seed %d: slack %.2e, float32 takes the same decisions: %s' % (key, seed, slack, same))
        if slack >= train_ref.HINGE_CLEAR and same:
            break
    else:
        raise SystemExit('case %s: no seed in %d tries keeps every decision %g clear' % (key, tries, train_ref.HINGE_CLEAR))
    arrays = {'sd0/' + k: v for k, v in sd0.items()}
    group = model.optimizer.param_groups[0]
    meta = {'key': key, 'seed': seed, 'slack': slack, 'model': spec['model'], 'vid_dims': VID_DIMS, 'txt_dims': TXT_DIMS, 'D': D, 'N': N,
            'batch_norm': True, 'max_violation': cfg.max_violation, 'direction': cfg.direction, 'margin': cfg.margin, 'loss': cfg.loss,
            'optimizer': cfg.optimizer, 'lr': cfg.lr, 'grad_clip': cfg.grad_clip, 'alpha': group.get('alpha'), 'eps': group['eps'],
            'betas': list(group.get('betas', ())), 'dropout': 0, 'encoder_name_list': list(model.txt_net.encoder.encoder_name_list),
            'steps': []}
    for s, (a, b) in enumerate(zip(r32, r64)):
        pre = 's%d/' % (s + 1)
        for k, v in inputs[s][0].items():
            arrays[pre + 'in/vis/' + k] = v
        for k, v in inputs[s][1].items():
            arrays[pre + 'in/txt/' + k] = v
        arrays[pre + 'txt_emb'], arrays[pre + 'vis_emb'] = b['txt_emb'], b['vis_emb']
        e = {'txt_emb': T.rel(a['txt_emb'], b['txt_emb']), 'vis_emb': T.rel(a['vis_emb'], b['vis_emb']),
             'loss': abs(a['loss'] - b['loss']) / abs(b['loss']), 'total_norm': abs(a['total_norm'] - b['total_norm']) / b['total_norm']}
        for k, v in b['grad'].items():
            arrays[pre + 'grad/' + k] = v
            e['grad/' + k] = T.rel(a['grad'][k], v)
        for k, v in b['sd'].items():
            arrays[pre + 'sd/' + k] = v
        for k, v in b['state'].items():
            arrays[pre + 'state/' + k] = v
        assert len(set(b['opt_step'].values())) == 1
        meta['steps'].append({'loss': b['loss'], 'loss32': a['loss'], 'total_norm': b['total_norm'], 'total_norm32': a['total_norm'],
                              'opt_step': list(b['opt_step'].values())[0], 'slack': b['slack'], 'e32': e})
        for k in sorted(e):
            print('  case %s step %d  e32 %-44s %.3e' % (key, s + 1, k, e[k]))
    check_restatement(arrays, meta, r64)
    return meta, arrays


def save_sharded(key, meta, arrays):
    for old in glob.glob(os.path.join(G.OUT, 'train_step_w2vvpp.%s.npz' % key)) + glob.glob(os.path.join(G.OUT, 'train_step_w2vvpp.%s.*.npz' % key)):
        os.remove(old)
    shards, cur, size = [], {}, 0
    for k in sorted(arrays):
        nb = arrays[k].nbytes
        assert nb < T.SHARD_BYTES, k
        if cur and size + nb > T.SHARD_BYTES:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = arrays[k]
        size += nb
    shards.append(cur)
    shards[0]['meta'] = np.array(json.dumps(meta))
    for i, sh in enumerate(shards):
        name = 'train_step_w2vvpp.%s.npz' % key if len(shards) == 1 else 'train_step_w2vvpp.%s.%d.npz' % (key, i)
        path = os.path.join(G.OUT, name)
        np.savez_compressed(path, **sh)
        assert os.path.getsize(path) <= (1 << 20), path
        print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def main():
    torch.set_grad_enabled(True)
    only = sys.argv[1].split(',') if len(sys.argv) > 1 else list(CASES)
    for i, (key, spec) in enumerate(CASES.items()):
        if key in only:
            save_sharded(key, *build_case(key, spec, 7600 + 100 * i))


if __name__ == '__main__':
    main()
