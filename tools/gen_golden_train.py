#!/usr/bin/env python3
"""tests/golden/train_step.<case>.<n>.npz: two training steps of the REAL reference's 'LAFF' model (tools/gen_golden.py's stub recipe,
gradients enabled), in float32 and, from the same initial state, in float64 (`model.double()`).

    python tools/gen_golden_train.py

Reference symbols exercised (file:line relative to the reference tree): model/model.py:1975-2048 W2VVPP_MultiHeadAttention (criterion,
RMSprop, compute_loss), :867-887 cal_foward, :964-1001 forward (backward, clip_grad_norm_, optimizer.step), :1830-1881 and :1641-1709
the two towers with and without expert embeddings, loss.py:68-135 MarginRankingLoss.

Arrays, name lists and scalars only.  Cases, all 'LAFF' with vid_dims {clip...1103: 128, X3D_L: 40}, txt_dims {bow 30, w2v 20,
CLIP 128}, D 512, H 4, BatchNorm on, with_ave, N 12, dropout 0, rmsprop at lr 1e-4, grad_clip 2:
    a   the reference's loss defaults (mrl, max_violation, t2i, margin 0.2)
    b   max_violation=False, direction='bidir'
    c   expert embeddings on both sides, l2norm off
    d   expert embeddings and l2norm on both sides
    e   'FrameLAFF': vid_dims {X3D_L: 40, mean_irCSN: 24} + the frame feature Frame_clip_ft (512, no transform) under
        attention_noAveNoAverageMul without a frame FC, txt_dims {bow 20, CLIP 512}, D 1024, H 2, B 10, Fmax 13, ragged frame counts
        that include 1 and Fmax; the loss defaults
Each case takes two steps, every one on fresh input dicts (the reference writes into them), step 2 on other inputs.  Per step and per
run: the embeddings and the loss, the raw (unclipped) gradients of cal_foward + backward on a deep copy, their global norm, the
parameters without a gradient, and after the step the state_dict (BatchNorm statistics included) and RMSprop's square_avg / step.
The float64 run is stored as arrays; of the float32 run the fixture keeps the loss and, per tensor, e32 = max |f32 - f64| / max |f64|
(printed as well), which is what the tests' tolerance rule reads.  The initial state is float32 (the float64 run starts from the same
values).

A seed is accepted when, before both steps, every hinge decision of the float64 run -- and under max_violation every top-2 gap --
stays at least tests/train_ref.HINGE_CLEAR from flipping and the float32 run takes the same decisions; the search stops after 40
seeds.

No committed file may exceed 1 MiB and float64 gradients do not compress, so a case is cut into numbered shards; the tests read all
shards of a case into one dict (tests/tower_ref.load_case).
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
CASES = {
    'a': dict(),
    'b': dict(max_violation=False, direction='bidir'),
    'c': dict(expert=True, l2norm=False),
    'd': dict(expert=True, l2norm=True),
    'e': dict(frame=True),
}
FRAME = dict(vid_dims={'X3D_L': 40, 'mean_irCSN': 24}, frame_feats=['Frame_clip_ft'], frame_dim=512, txt_dims={'bow': 20, 'CLIP': 512},
             D=1024, H=2, B=10, Fmax=13, frame_attention='attention_noAveNoAverageMul')


def make_cfg(spec):
    if spec.get('frame'):
        cfg = G.framelaff_cfg(FRAME['vid_dims'], FRAME['frame_feats'], FRAME['D'], FRAME['H'], FRAME['frame_attention'], False, True, True)
        cfg.dropout = 0
        cfg.clip_opt = dict(cfg.clip_opt, size=FRAME['txt_dims']['CLIP'])
        assert (cfg.loss, cfg.optimizer, cfg.lr, cfg.grad_clip, cfg.margin, cfg.negative, cfg.max_violation, cfg.direction) == \
            ('mrl', 'rmsprop', 1e-4, 2, 0.2, False, True, 't2i')
        return cfg
    cfg = G.laff_cfg(VID_DIMS, TXT_DIMS, D, H, True, False, True, ['clip_finetune_8frame_uniform_1103'])
    cfg.dropout = 0
    cfg.max_violation = spec.get('max_violation', True)
    cfg.direction = spec.get('direction', 't2i')
    cfg.vis_expert_embedding = {'expert': bool(spec.get('expert')), 'l2norm': bool(spec.get('l2norm'))}
    cfg.txt_expert_embedding = {'expert': bool(spec.get('expert')), 'l2norm': bool(spec.get('l2norm'))}
    assert (cfg.loss, cfg.optimizer, cfg.lr, cfg.grad_clip, cfg.margin, cfg.multi_space, cfg.negative) == ('mrl', 'rmsprop', 1e-4, 2, 0.2, True, False)
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


def make_inputs(g):
    vis = {k: G.f32(g.normal(0, 1, (N, d))) for k, d in VID_DIMS.items()}
    txt = {'bow_feature': G.f32((g.uniform(0, 1, (N, 30)) < 0.15).astype(np.float32)),
           'w2v_feature': G.f32(g.normal(0, 1, (N, 20))), 'CLIP_encoding': G.f32(g.normal(0, 1, (N, 128)))}
    return vis, txt


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


def run(model, inputs, dtype, cfg):
    """Two steps of `model` (already of `dtype`); everything recorded as float64 numpy arrays / Python scalars."""
    out = []
    for step in (0, 1):
        rec = {}
        probe = clone(model)                      # the embeddings, on a copy (a forward moves the running statistics)
        data = train_data(inputs[step], dtype)
        txt_emb = probe.txt_net(data['captions'])
        vis_emb = probe.vis_net(data['vis_feats'], txt_emb=txt_emb, vis_frame_feat_dict_input=data['vis_frame_feat_dict'] or None)
        rec['txt_emb'], rec['vis_emb'] = txt_emb.detach().double().numpy(), vis_emb.detach().double().numpy()
        rec['slack'], rec['decisions'] = decisions(txt_emb, vis_emb, cfg)
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
        rec['sq'], rec['opt_step'] = {}, {}
        for p, st in model.optimizer.state.items():
            k = names[id(p)]
            if not k.startswith('txt_net.encoder.'):
                rec['sq'][k] = st['square_avg'].detach().double().clone().numpy()
                rec['opt_step'][k] = float(st['step'])
        out.append(rec)
    return out


def rel(a, b):
    top = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / top if top else float(np.abs(a - b).max())


def build_case(key, spec, first_seed, tries=40):
    cfg = make_cfg(spec)
    for seed in range(first_seed, first_seed + tries):
        g = G.rng(seed)
        torch.manual_seed(seed)
        frame = bool(spec.get('frame'))
        model = mm.get_model('FrameLAFF' if frame else 'LAFF', torch.device('cpu'), cfg)
        G.plug_text_encoders(model)
        G.randomize_model(model, g, None if frame else 0.6, None if frame else 0.8)
        model.train()
        inputs = [make_frame_inputs(g), make_frame_inputs(g)] if frame else [make_inputs(g), make_inputs(g)]
        sd0 = {k: v.numpy().copy() for k, v in sd_of(model).items()}
        m64 = copy.deepcopy(model).double()
        r64 = run(m64, inputs, torch.float64, cfg)
        r32 = run(copy.deepcopy(model), inputs, torch.float32, cfg)
        slack = min(r['slack'] for r in r64)
        same = all(np.array_equal(a['decisions'], b['decisions']) for a, b in zip(r32, r64))
        print('case %s seed %d: slack %.2e, float32 takes the same decisions: %s' % (key, seed, slack, same))
        if slack >= train_ref.HINGE_CLEAR and same:
            break
    else:
        raise SystemExit('case %s: no seed in %d tries keeps every decision %g clear' % (key, tries, train_ref.HINGE_CLEAR))
    arrays, e32 = {}, {}
    for k, v in sd0.items():
        arrays['sd0/' + k] = v
    meta = {'key': key, 'seed': seed, 'slack': slack, 'model': 'LAFF', 'vid_dims': VID_DIMS, 'txt_dims': TXT_DIMS, 'D': D, 'H': H, 'N': N,
            'with_ave': True, 'mul': False, 'batch_norm': True, 'vis_no_transform': ['clip_finetune_8frame_uniform_1103'],
            'txt_no_transform': list(cfg.txt_no_transform), 'expert': bool(spec.get('expert')), 'l2norm': bool(spec.get('l2norm')),
            'max_violation': cfg.max_violation, 'direction': cfg.direction, 'margin': cfg.margin, 'loss': cfg.loss,
            'optimizer': cfg.optimizer, 'lr': cfg.lr, 'grad_clip': cfg.grad_clip, 'alpha': 0.99, 'eps': 1e-8, 'dropout': 0,
            'encoder_name_list': list(model.txt_net.encoder_name_list), 'steps': []}
    if frame:
        meta.update(model='FrameLAFF', vid_dims=FRAME['vid_dims'], txt_dims=FRAME['txt_dims'], D=FRAME['D'], H=FRAME['H'], N=FRAME['B'],
                    with_ave=False, vis_no_transform=FRAME['frame_feats'], frame_feats={f: FRAME['frame_dim'] for f in FRAME['frame_feats']},
                    vis_frame_attention=FRAME['frame_attention'], max_frame=FRAME['Fmax'])
    for s, (a, b) in enumerate(zip(r32, r64)):
        pre = 's%d/' % (s + 1)
        for k, v in inputs[s][0].items():
            arrays[pre + 'in/vis/' + k] = v
        for k, v in inputs[s][1].items():
            arrays[pre + 'in/txt/' + k] = v
        for k, v in (inputs[s][2] if frame else {}).items():
            arrays[pre + 'in/frame/' + k] = v
        arrays[pre + 'txt_emb'], arrays[pre + 'vis_emb'] = b['txt_emb'], b['vis_emb']
        assert a['none'] == b['none']
        e = {'txt_emb': rel(a['txt_emb'], b['txt_emb']), 'vis_emb': rel(a['vis_emb'], b['vis_emb']),
             'loss': abs(a['loss'] - b['loss']) / abs(b['loss']), 'total_norm': abs(a['total_norm'] - b['total_norm']) / b['total_norm']}
        for k, v in b['grad'].items():
            arrays[pre + 'grad/' + k] = v
            e['grad/' + k] = rel(a['grad'][k], v)
        for k, v in b['sd'].items():
            arrays[pre + 'sd/' + k] = v
        for k, v in b['sq'].items():
            arrays[pre + 'sq/' + k] = v
        assert len(set(b['opt_step'].values())) == 1
        meta['steps'].append({'loss': b['loss'], 'loss32': a['loss'], 'total_norm': b['total_norm'], 'total_norm32': a['total_norm'],
                              'none': b['none'], 'opt_step': list(b['opt_step'].values())[0], 'slack': b['slack'], 'e32': e})
        for k in sorted(e):
            print('  case %s step %d  e32 %-70s %.3e' % (key, s + 1, k, e[k]))
    # the float64 restatement of the tests (tests/tower_ref.py) has to reproduce the reference's float64 run
    for s in (1, 2):
        graph = tower_ref.step_graph_of(arrays, meta, s)
        for k, v in r64[s - 1]['grad'].items():
            if not k.endswith('embedding_common.0.bias'):
                assert rel(graph['grads'][k].numpy(), v) <= 1e-12, k
    return meta, arrays


def save_sharded(key, meta, arrays):
    for old in glob.glob(os.path.join(G.OUT, 'train_step.%s.*.npz' % key)):
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
        path = os.path.join(G.OUT, 'train_step.%s.%d.npz' % (key, i))
        np.savez_compressed(path, **sh)
        assert os.path.getsize(path) <= (1 << 20), path
        print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def main():
    torch.set_grad_enabled(True)
    only = sys.argv[1].split(',') if len(sys.argv) > 1 else list(CASES)
    for i, (key, spec) in enumerate(CASES.items()):
        if key in only:
            save_sharded(key, *build_case(key, spec, 7000 + 100 * i))


if __name__ == '__main__':
    main()
