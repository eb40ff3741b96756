#!/usr/bin/env python3
"""tests/golden/train_step.<case>.<n>.npz and tests/golden/train_step_w2vvpp.<case>.<n>.npz: two training steps of the REAL reference's
models (tools/gen_golden.py's stub recipe, gradients enabled), in float32 and, from the same initial state, in float64
(`model.double()`).

    python tools/gen_golden_train.py [a,b,...]

Reference symbols exercised (file:line relative to the reference tree): model/model.py:1975-2048 W2VVPP_MultiHeadAttention (criterion,
RMSprop, compute_loss), :867-887 cal_foward, :964-1001 forward (backward, clip_grad_norm_, optimizer.step), :1830-1881 and :1641-1709
the two towers with and without expert embeddings, loss.py:68-135 MarginRankingLoss; for the concat towers :279-308 VisTransformNet,
:552-726 MultiScaleTxtEncoder / MultiScaleTxtNet, :791-836 W2VVPP.__init__ (criterion, Adam / RMSprop with torch's default eps),
:840-865 compute_loss on 2-D embeddings, :2501-2519 get_model.

Arrays, name lists and scalars only.  A case is an entry of CASES: the registry key, how to build the config, how to plug the text
encoders, the arguments of randomize_model, how to draw a step's inputs, the meta fields of its own, the first seed and the file stem.
Cases a-d, all 'LAFF' with vid_dims {clip...1103: 128, X3D_L: 40}, txt_dims {bow 30, w2v 20, CLIP 128}, D 512, H 4, BatchNorm on,
with_ave, N 12, dropout 0, rmsprop at lr 1e-4, grad_clip 2:
    a   the reference's loss defaults (mrl, max_violation, t2i, margin 0.2)
    b   max_violation=False, direction='bidir'
    c   expert embeddings on both sides, l2norm off
    d   expert embeddings and l2norm on both sides
    e   'FrameLAFF': vid_dims {X3D_L: 40, mean_irCSN: 24} + the frame feature Frame_clip_ft (512, no transform) under
        attention_noAveNoAverageMul without a frame FC, txt_dims {bow 20, CLIP 512}, D 1024, H 2, B 10, Fmax 13, ragged frame counts
        that include 1 and Fmax; the loss defaults
The W2VV++ concat towers (the towers' config of tools/gen_golden_w2vvpp.py): video features {resnext 96, x3d 48, ircsn 40},
pre-extracted text features {bow 30, w2v 50, CLIP 64}, both towers to D = 64, B = 12, BatchNorm on, dropout 0 (the masks cannot be
shared with the reference), lr 1e-4, grad_clip 2:
    i    'W2VVPP', rmsprop, max_violation=True, direction 't2i'
    ii   'w2vpp_mutivis_attention' with both attentions 'concat', adam, max_violation=False, direction 'bidir' -- the case that pins
         Adam's eps to torch's default 1e-8
Each case takes two steps, every one on fresh input dicts (the reference writes into them), step 2 on other inputs.  Per step and per
run: the embeddings and the loss, the raw (unclipped) gradients of cal_foward + backward on a deep copy, their global norm, the
parameters without a gradient, and after the step the state_dict (BatchNorm statistics included) and the optimizer's state
(s<n>/state/<state name>/<param> -- RMSprop: square_avg; Adam: exp_avg, exp_avg_sq) and step.  The float64 run is stored as arrays; of
the float32 run the fixture keeps the loss and, per tensor, e32 = max |f32 - f64| / max |f64| (printed as well), which is what the
tests' tolerance rule reads.  The initial state is float32 (the float64 run starts from the same values).

A seed is accepted when, before both steps, every hinge decision of the float64 run -- and under max_violation every top-2 gap; for
the concat cases train_ref.hinge_slack of the embeddings as well -- stays at least tests/train_ref.HINGE_CLEAR from flipping and the
float32 run takes the same decisions; the search stops after 40 seeds.  Before anything is written the float64 restatement of the
tests (tests/tower_ref.py, tests/optim_ref.py) has to reproduce the float64 run to 1e-12: embeddings, loss, gradients, parameters and
optimizer state.

No committed file may exceed 1 MiB and float64 gradients do not compress, so a case is cut into numbered shards; the tests read all
shards of a case into one dict (tests/tower_ref.load_case).  The committed cases a-e were written when RMSprop's state was stored as
s<n>/sq/<param>; load_case renames that on load.
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
import gen_golden_w2vvpp as WV  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import loss_ref  # noqa: E402
import tower_ref  # noqa: E402
import train_ref  # noqa: E402

mm = G.mm
VID_DIMS = {'clip_finetune_8frame_uniform_1103': 128, 'X3D_L': 40}
TXT_DIMS = {'bow': 30, 'w2v': 20, 'CLIP': 128}
D, H, N = 512, 4, 12
SHARD_BYTES = 900 * 1024
FRAME = dict(vid_dims={'X3D_L': 40, 'mean_irCSN': 24}, frame_feats=['Frame_clip_ft'], frame_dim=512, txt_dims={'bow': 20, 'CLIP': 512},
             D=1024, H=2, B=10, Fmax=13, frame_attention='attention_noAveNoAverageMul')


def frame_cfg():
    cfg = G.framelaff_cfg(FRAME['vid_dims'], FRAME['frame_feats'], FRAME['D'], FRAME['H'], FRAME['frame_attention'], False, True, True)
    cfg.dropout = 0
    cfg.clip_opt = dict(cfg.clip_opt, size=FRAME['txt_dims']['CLIP'])
    assert (cfg.loss, cfg.optimizer, cfg.lr, cfg.grad_clip, cfg.margin, cfg.negative, cfg.max_violation, cfg.direction) == \
        ('mrl', 'rmsprop', 1e-4, 2, 0.2, False, True, 't2i')
    return cfg


def laff_cfg(max_violation=True, direction='t2i', expert=False, l2norm=False):
    cfg = G.laff_cfg(VID_DIMS, TXT_DIMS, D, H, True, False, True, ['clip_finetune_8frame_uniform_1103'])
    cfg.dropout = 0
    cfg.max_violation = max_violation
    cfg.direction = direction
    cfg.vis_expert_embedding = {'expert': expert, 'l2norm': l2norm}
    cfg.txt_expert_embedding = {'expert': expert, 'l2norm': l2norm}
    assert (cfg.loss, cfg.optimizer, cfg.lr, cfg.grad_clip, cfg.margin, cfg.multi_space, cfg.negative) == ('mrl', 'rmsprop', 1e-4, 2, 0.2, True, False)
    return cfg


def concat_cfg(optimizer, max_violation, direction):
    cfg = WV.concat_cfg(CONCAT_D, True)
    cfg.dropout = 0
    cfg.optimizer = optimizer
    cfg.max_violation = max_violation
    cfg.direction = direction
    assert (cfg.loss, cfg.lr, cfg.grad_clip, cfg.margin, cfg.negative, cfg.activation) == ('mrl', 1e-4, 2, 0.2, False, 'tanh')
    return cfg


def make_frame_inputs(g):
    B, Fmax, d = FRAME['B'], FRAME['Fmax'], FRAME['frame_dim']
    lens = g.integers(3, Fmax + 1, B)
    lens[0], lens[3] = Fmax, 1
    frames, mask = np.zeros((B, Fmax, d), np.float32), np.zeros((B, Fmax), np.float32)
    for b in range(B):
        frames[b, :lens[b]] = G.f32(g.normal(0, 1, (lens[b], d)))
        mask[b, :lens[b]] = 1
    vis = {k: G.f32(g.normal(0, 1, (B, w))) for k, w in FRAME['vid_dims'].items()}
    txt = {'bow_feature': G.f32((g.uniform(0, 1, (B, 20)) < 0.2).astype(np.float32)), 'CLIP_encoding': G.f32(g.normal(0, 1, (B, 512)))}
    return vis, txt, {'Frame_clip_ft': frames, 'mask_tensor': mask}


def make_inputs(g, vid_dims=VID_DIMS, txt_dims=TXT_DIMS):
    vis = {k: G.f32(g.normal(0, 1, (N, d))) for k, d in vid_dims.items()}
    txt = {'bow_feature': G.f32((g.uniform(0, 1, (N, txt_dims['bow'])) < 0.15).astype(np.float32)),
           'w2v_feature': G.f32(g.normal(0, 1, (N, txt_dims['w2v']))), 'CLIP_encoding': G.f32(g.normal(0, 1, (N, txt_dims['CLIP'])))}
    return vis, txt


def laff_meta(cfg, model):
    assert cfg.vis_expert_embedding == cfg.txt_expert_embedding
    return {'vid_dims': VID_DIMS, 'txt_dims': TXT_DIMS, 'D': D, 'H': H, 'N': N, 'with_ave': True, 'mul': False,
            'vis_no_transform': ['clip_finetune_8frame_uniform_1103'], 'txt_no_transform': list(cfg.txt_no_transform),
            'expert': cfg.vis_expert_embedding['expert'], 'l2norm': cfg.vis_expert_embedding['l2norm'],
            'encoder_name_list': list(model.txt_net.encoder_name_list)}


def frame_meta(cfg, model):
    return dict(laff_meta(cfg, model), vid_dims=FRAME['vid_dims'], txt_dims=FRAME['txt_dims'], D=FRAME['D'], H=FRAME['H'], N=FRAME['B'],
                with_ave=False, vis_no_transform=FRAME['frame_feats'], frame_feats={f: FRAME['frame_dim'] for f in FRAME['frame_feats']},
                vis_frame_attention=FRAME['frame_attention'], max_frame=FRAME['Fmax'])


def concat_meta(cfg, model):
    assert type(model.vis_net).__name__ == 'VisTransformNet' and type(model.txt_net).__name__ == 'MultiScaleTxtNet'
    return {'vid_dims': WV.VID_DIMS, 'txt_dims': WV.TXT_DIMS, 'D': CONCAT_D, 'H': 1, 'N': N,
            'encoder_name_list': list(model.txt_net.encoder.encoder_name_list)}


def laff_case(seed, **loss):
    return dict(model='LAFF', cfg=lambda: laff_cfg(**loss), plug=G.plug_text_encoders, randomize=(0.6, 0.8), inputs=make_inputs, meta=laff_meta,
                seed=seed, stem='train_step')


def concat_case(seed, model, **training):
    """hinge_slack: train_ref.hinge_slack of the embeddings takes part in the slack a seed is accepted by."""
    return dict(model=model, cfg=lambda: concat_cfg(**training), plug=WV.plug, randomize=(), hinge_slack=True,
                inputs=lambda g: make_inputs(g, WV.VID_DIMS, WV.TXT_DIMS), meta=concat_meta, seed=seed, stem='train_step_w2vvpp')


CONCAT_D = 64
CASES = {
    'a': laff_case(7000),
    'b': laff_case(7100, max_violation=False, direction='bidir'),
    'c': laff_case(7200, expert=True, l2norm=False),
    'd': laff_case(7300, expert=True, l2norm=True),
    'e': dict(model='FrameLAFF', cfg=frame_cfg, plug=G.plug_text_encoders, randomize=(), inputs=make_frame_inputs, meta=frame_meta, seed=7400,
              stem='train_step'),
    'i': concat_case(7600, 'W2VVPP', optimizer='rmsprop', max_violation=True, direction='t2i'),
    'ii': concat_case(7700, 'w2vpp_mutivis_attention', optimizer='adam', max_violation=False, direction='bidir'),
}
assert {k: c['stem'] for k, c in CASES.items()} == tower_ref.STEMS


def train_data(inputs, dtype):
    """Fresh dicts of fresh tensors: the reference stores the repeated no-transform feature back into vis_feats."""
    vis, txt = inputs[:2]
    frames = {k: torch.from_numpy(v.copy()).to(dtype) for k, v in inputs[2].items()} if len(inputs) > 2 else {}
    cap = {'caption': ['%d' % i for i in range(len(next(iter(vis.values()))))]}
    cap.update({k: torch.from_numpy(v.copy()).to(dtype) for k, v in txt.items()})
    return {'vis_feats': {k: torch.from_numpy(v.copy()).to(dtype) for k, v in vis.items()}, 'captions': cap, 'captions_task2': None,
            'vis_frame_feat_dict': frames, 'vis_origin_frame_tuple': None}


def decisions(txt_emb, vis_emb, cfg):
    """(smallest slack over the heads in float64 arithmetic on these embeddings, the decisions themselves: the sign of every hinge
    argument and, under max_violation, the hardest negative's index per row / column)."""
    Et, Ev = txt_emb.detach().double().numpy(), vis_emb.detach().double().numpy()
    slack, taken = np.inf, []
    for h in range(Et.shape[1]):
        t = Et[:, h] / np.linalg.norm(Et[:, h], axis=1, keepdims=True)
        v = Ev[:, h] / np.linalg.norm(Ev[:, h], axis=1, keepdims=True)
        S = v @ t.T
        slack = min(slack, loss_ref.margin_scores_slack(S, cfg.margin, cfg.max_violation, cfg.direction))
        dg = np.diag(S)
        off = ~np.eye(S.shape[0], dtype=bool)
        for name, ref, axis in (('i2t', dg[:, None], 1), ('t2i', dg[None, :], 0)):
            if cfg.direction not in (name, 'bidir'):
                continue
            arg = cfg.margin + S - ref
            taken.append((arg > 0)[off])
            if cfg.max_violation:
                taken.append(np.where(off, np.maximum(arg, 0), -np.inf).argmax(axis=axis))
    return slack, np.concatenate([np.asarray(t).reshape(-1).astype(np.int64) for t in taken])


def param_model(model):
    """The reference model's trainable tensors by name, the plugged placeholders of the text encoders left out."""
    return {k: p for k, p in model.named_parameters() if not k.startswith('txt_net.encoder.')}


def sd_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if not k.startswith('txt_net.encoder.')}


def clone(model):
    """A deep copy; the attention blocks' stashed softmax weights (non-leaf tensors of the last forward) are dropped first."""
    for m in model.modules():
        if isinstance(m.__dict__.get('weights'), torch.Tensor):
            m.weights = 0
    return copy.deepcopy(model)


def run(model, inputs, dtype, cfg, hinge_slack=False):
    """Two steps of `model` (already of `dtype`); everything recorded as float64 numpy arrays / Python scalars."""
    out = []
    for step in (0, 1):
        rec = {}
        probe = clone(model)                      # the embeddings, on a copy (a forward moves the running statistics)
        data = train_data(inputs[step], dtype)
        txt_emb = probe.txt_net(data['captions'])
        vis_emb = probe.vis_net(data['vis_feats'], txt_emb=txt_emb, vis_frame_feat_dict_input=data['vis_frame_feat_dict'] or None)
        rec['txt_emb'], rec['vis_emb'] = txt_emb.detach().double().numpy(), vis_emb.detach().double().numpy()
        heads = (lambda e: e[:, None]) if txt_emb.dim() == 2 else (lambda e: e)     # 2-D embeddings are one head
        rec['slack'], rec['decisions'] = decisions(heads(txt_emb), heads(vis_emb), cfg)
        if hinge_slack:
            rec['slack'] = min(rec['slack'], train_ref.hinge_slack(txt_emb, vis_emb, cfg.margin))
        probe = clone(model)                      # the raw gradients, on another copy
        loss, _ = probe.cal_foward(train_data(inputs[step], dtype))
        loss.backward()
        rec['loss'] = float(loss.detach().double())
        grads = {k: p.grad for k, p in param_model(probe).items()}
        rec['none'] = sorted(k for k, gr in grads.items() if gr is None)
        rec['grad'] = {k: gr.detach().double().numpy() for k, gr in grads.items() if gr is not None}
        rec['total_norm'] = float(np.sqrt(sum(float((gr ** 2).sum()) for gr in rec['grad'].values())))
        items = model(train_data(inputs[step], dtype))     # the step itself
        assert abs(float(items['triplet_loss'].detach().double()) - rec['loss']) <= 1e-6 * abs(rec['loss'])
        rec['sd'] = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in sd_of(model).items()}
        names = {id(p): k for k, p in model.named_parameters()}
        rec['state'], rec['opt_step'] = {}, {}
        for p, st in model.optimizer.state.items():
            k = names[id(p)]
            if not k.startswith('txt_net.encoder.'):
                for n in tower_ref.STATE_NAMES[cfg.optimizer]:       # whatever the case's optimizer keeps
                    rec['state'][n + '/' + k] = st[n].detach().double().clone().numpy()
                rec['opt_step'][k] = float(st['step'])
        out.append(rec)
    return out


def rel(f32, f64):
    """tower_ref.rel_err; the absolute error where the float64 tensor is zero throughout (a softmax bias's gradient can be), which
    rel_err has no finite figure for."""
    return tower_ref.rel_err(f32, f64) if np.any(f64) else float(np.abs(f32).max())


def build_case(key, spec, tries=40):
    cfg = spec['cfg']()
    for seed in range(spec['seed'], spec['seed'] + tries):
        g = G.rng(seed)
        torch.manual_seed(seed)
        model = mm.get_model(spec['model'], torch.device('cpu'), cfg)
        spec['plug'](model)
        G.randomize_model(model, g, *spec['randomize'])
        model.train()
        inputs = [spec['inputs'](g), spec['inputs'](g)]
        sd0 = {k: v.numpy().copy() for k, v in sd_of(model).items()}
        r64 = run(copy.deepcopy(model).double(), inputs, torch.float64, cfg, spec.get('hinge_slack', False))
        r32 = run(copy.deepcopy(model), inputs, torch.float32, cfg, spec.get('hinge_slack', False))
        slack = min(r['slack'] for r in r64)
        same = all(np.array_equal(a['decisions'], b['decisions']) for a, b in zip(r32, r64))
        print('case %s seed %d: slack %.2e, float32 takes the same decisions: %s' % (key, seed, slack, same))
        if slack >= train_ref.HINGE_CLEAR and same:
            break
    else:
        raise SystemExit('case %s: no seed in %d tries keeps every decision %g clear' % (key, tries, train_ref.HINGE_CLEAR))
    arrays, group = {'sd0/' + k: v for k, v in sd0.items()}, model.optimizer.param_groups[0]
    assert cfg.txt_attention == cfg.vis_attention
    meta = {'key': key, 'seed': seed, 'slack': slack, 'model': spec['model'], 'attention': cfg.txt_attention, 'batch_norm': True,
            'max_violation': cfg.max_violation, 'direction': cfg.direction, 'margin': cfg.margin, 'loss': cfg.loss,
            'optimizer': cfg.optimizer, 'lr': cfg.lr, 'grad_clip': cfg.grad_clip, 'alpha': group.get('alpha'), 'eps': group['eps'],
            'betas': list(group.get('betas', ())), 'dropout': 0, 'steps': []}
    meta.update(spec['meta'](cfg, model))
    for s, (a, b) in enumerate(zip(r32, r64)):
        pre = 's%d/' % (s + 1)
        for side, values in zip(('vis', 'txt', 'frame'), inputs[s]):
            for k, v in values.items():
                arrays[pre + 'in/' + side + '/' + k] = v
        arrays[pre + 'txt_emb'], arrays[pre + 'vis_emb'] = b['txt_emb'], b['vis_emb']
        assert a['none'] == b['none']
        e = {'txt_emb': rel(a['txt_emb'], b['txt_emb']), 'vis_emb': rel(a['vis_emb'], b['vis_emb']),
             'loss': abs(a['loss'] - b['loss']) / abs(b['loss']), 'total_norm': abs(a['total_norm'] - b['total_norm']) / b['total_norm']}
        for k, v in b['grad'].items():
            arrays[pre + 'grad/' + k] = v
            e['grad/' + k] = rel(a['grad'][k], v)
        for part in ('sd', 'state'):
            for k, v in b[part].items():
                arrays[pre + part + '/' + k] = v
        assert len(set(b['opt_step'].values())) == 1
        meta['steps'].append({'loss': b['loss'], 'loss32': a['loss'], 'total_norm': b['total_norm'], 'total_norm32': a['total_norm'],
                              'none': b['none'], 'opt_step': list(b['opt_step'].values())[0], 'slack': b['slack'], 'e32': e})
        for k in sorted(e):
            print('  case %s step %d  e32 %-70s %.3e' % (key, s + 1, k, e[k]))
    # the float64 restatement of the tests (tests/tower_ref.py, tests/optim_ref.py) has to reproduce the reference's float64 run
    tower_ref.check_restatement(arrays, meta)
    tower_ref.check_replay(arrays, meta)
    return meta, arrays


def save_sharded(key, stem, meta, arrays):
    stem = os.path.join(G.OUT, '%s.%s' % (stem, key))
    for old in glob.glob(stem + '.npz') + glob.glob(stem + '.*.npz'):
        os.remove(old)
    shards, cur, size = [], {}, 0
    for k in sorted(arrays):
        nb = arrays[k].nbytes
        assert nb < SHARD_BYTES, k
        if cur and size + nb > SHARD_BYTES:
            shards.append(cur)
            cur, size = {}, 0
        cur[k] = arrays[k]
        size += nb
    shards.append(cur)
    shards[0]['meta'] = np.array(json.dumps(meta))
    for i, sh in enumerate(shards):
        path = stem + ('.npz' if len(shards) == 1 else '.%d.npz' % i)
        np.savez_compressed(path, **sh)
        assert os.path.getsize(path) <= (1 << 20), path
        print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def main():
    torch.set_grad_enabled(True)
    only = sys.argv[1].split(',') if len(sys.argv) > 1 else list(CASES)
    for key, spec in CASES.items():
        if key in only:
            save_sharded(key, spec['stem'], *build_case(key, spec))


if __name__ == '__main__':
    main()
