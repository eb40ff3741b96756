#!/usr/bin/env python3
"""tests/golden/selfattn.<shape>.<l2norm>.npz: the reference's own Multi_head_MyApply_selfAttention (model/Attention.py:317-470) on the CPU, in
float64 and in float32, forward and backward, for every output type this project provides, with and without l2norm_each_head.

    python tools/gen_golden_selfattn.py [blocks,sa_mean,sa_att1]

The reference is imported at generation time only (tools/gen_golden.py's recipe); arrays, names and scalars are written, nothing else.
One file per shape (N, L, H, d) of SHAPES and per l2norm_each_head (float64 gradients do not compress); per case
`<output type>.<l2norm 0|1>/`:
    x (N, L, H d) float32, gamma, beta (d,) float32 -- random, non-trivial --, dE (N, H, d) float32,
    E, dx, dgamma, dbeta of the float64 run,
    under 'Attention_1' also w (H, d), b (H,), gw (H,), with_ave, mul, dw, db and weights (get_attention_weight),
    e32/<name>: max |f32 - f64| / max |f64| of the float32 run, per output;
meta (json): the shape, the case names and per case the state_dict keys with their shapes.
'random' is run in eval mode (there it is the mean); every other type in training mode with dropout 0.
Before anything is written the restatement of the tests (tests/selfattn_ref.py) has to reproduce the float64 run to 1e-12.

tests/golden/train_step_selfattn.<case>.<n>.npz: two training steps of the reference's 'LAFF' model with both attentions
'my_self_attention', cases sa_mean (output type 'mean') and sa_att1 ('Attention_1'), with the settings, shapes and layout of case a of
tools/gen_golden_train.py, whose machinery writes them (build_case: two RMSprop steps in float64 and float32 from one initial state;
embeddings, loss, raw gradients, parameters and optimizer state after each step; a seed is accepted when every hinge decision of the
float64 run stays train_ref.HINGE_CLEAR from flipping and the float32 run takes the same decisions; the float64 restatement of the
tests -- tests/tower_ref.py with the fusion of tests/selfattn_tower.py -- has to reproduce the run to 1e-12; shards under 900 KB).
"""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import gen_golden as G  # noqa: E402  (imports the reference)
import gen_golden_train as T  # noqa: E402  (before selfattn_tower: it checks tower_ref's case list as committed)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import selfattn_ref as R  # noqa: E402
import selfattn_tower  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
SHAPES = [(5, 1, 1, 4), (5, 3, 2, 8), (5, 8, 4, 36)]
TYPES = R.OUTPUT_TYPES
MAX_BYTES = 900 * 1024


def reference_run(case, dtype):
    N, L, H, d = case['shape']
    opt = types.SimpleNamespace(attention_param_each_head={'with_ave': case['with_ave'], 'mul': case['mul']})
    m = G.ref_att.Multi_head_MyApply_selfAttention(H * d, H, d, 0.0, output_type=case['type'], encoder_num=L,
                                                   l2norm_each_head=case['l2n'], opt=opt)
    with torch.no_grad():
        m.layer_norm.weight.copy_(torch.from_numpy(case['gamma']))
        m.layer_norm.bias.copy_(torch.from_numpy(case['beta']))
        if case['type'] == 'Attention_1':
            for h, a in enumerate(m.Attention_list):
                a.embedding_common[0].weight.copy_(torch.from_numpy(case['w'][h:h + 1]))
                a.embedding_common[0].bias.copy_(torch.from_numpy(case['b'][h:h + 1]))
                a.change_raw_global_emb_weight(float(case['gw'][h]))
    m = m.to(dtype)
    m.train(case['type'] != 'random')
    x = torch.from_numpy(case['x']).to(dtype).requires_grad_(True)
    with torch.enable_grad():                                     # (gen_golden switches gradients off when it is imported)
        E = m(x)
        (E * torch.from_numpy(case['dE']).to(dtype)).sum().backward()
    out = {'E': E, 'dx': x.grad, 'dgamma': m.layer_norm.weight.grad, 'dbeta': m.layer_norm.bias.grad}
    if case['type'] == 'Attention_1':
        out['dw'] = torch.cat([a.embedding_common[0].weight.grad for a in m.Attention_list])
        out['db'] = torch.cat([a.embedding_common[0].bias.grad for a in m.Attention_list])
        out['weights'] = m.get_attention_weight()
    res = {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}
    res['state'] = {k: list(v.shape) for k, v in m.state_dict().items()}
    return res


def model_case(output_type, seed):
    def cfg():
        c = T.laff_cfg()
        c.vis_attention = c.txt_attention = selfattn_tower.ATTENTION
        c.my_self_attention_output_type = output_type
        assert c.multi_head_attention['dropout'] == 0.0 and not c.attention_l2norm
        return c
    return dict(T.laff_case(seed), cfg=cfg, stem=selfattn_tower.STEM,
                meta=lambda c, model: dict(T.laff_meta(c, model), output_type=c.my_self_attention_output_type))


MODEL_CASES = {'sa_mean': model_case('mean', 7800), 'sa_att1': model_case('Attention_1', 7900)}
assert {k: c['cfg']().my_self_attention_output_type for k, c in MODEL_CASES.items()} == selfattn_tower.CASES


def main():
    only = sys.argv[1].split(',') if len(sys.argv) > 1 else ['blocks'] + list(MODEL_CASES)
    torch.set_grad_enabled(True)
    for key, spec in MODEL_CASES.items():
        if key in only:
            T.save_sharded(key, spec['stem'], *T.build_case(key, spec))
    if 'blocks' in only:
        blocks()


def blocks():
    g = np.random.default_rng(20261021)
    for n, l2n in [(n, l2n) for n in range(len(SHAPES)) for l2n in (False, True)]:
        shape = SHAPES[n]
        N, L, H, d = shape
        arrays, names, state = {}, [], {}
        for t in TYPES:
            case = {'shape': shape, 'type': t, 'l2n': l2n, 'with_ave': l2n, 'mul': bool(n % 2),
                    'x': G.f32(g.normal(0, 1, (N, L, H * d))), 'gamma': G.f32(g.uniform(0.5, 1.5, d)),
                    'beta': G.f32(g.normal(0, 0.3, d)), 'dE': G.f32(g.normal(0, 1, (N, H, d))),
                    'w': G.f32(g.normal(0, 0.5, (H, d))), 'b': G.f32(g.normal(0, 0.5, H)), 'gw': G.f32(g.uniform(0.3, 1.0, H))}
            f64, f32 = reference_run(case, torch.float64), reference_run(case, torch.float32)
            att1 = {k: case[k] for k in ('w', 'b', 'gw', 'with_ave', 'mul')} if t == 'Attention_1' else None
            mine = R.run(case['x'], H, d, case['gamma'], case['beta'], t, l2n, att1, case['dE'])
            name = '%s.%d' % (t, l2n)
            state[name] = f64.pop('state')
            f32.pop('state')
            for k, v in f64.items():
                # db is zero but for rounding (a softmax does not see a shift of its logits): held absolutely
                err = float(np.abs(mine[k].numpy() - v).max()) if k == 'db' else R.rel_err(mine[k], v)
                assert err < 1e-12, (shape, name, k, err)
                arrays['%s/%s' % (name, k)] = v
                arrays['%s/e32/%s' % (name, k)] = np.float64(R.rel_err(f32[k], v))
            for k in ('x', 'gamma', 'beta', 'dE') + (('w', 'b', 'gw') if att1 else ()):
                arrays['%s/%s' % (name, k)] = case[k]
            if att1:
                arrays[name + '/with_ave'], arrays[name + '/mul'] = np.bool_(case['with_ave']), np.bool_(case['mul'])
            names.append(name)
        arrays['meta'] = np.array(json.dumps({'shape': shape, 'cases': names, 'state_dict': state}))
        path = os.path.join(OUT, 'selfattn.%d.%d.npz' % (n, l2n))
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, (path, size)
        print(path, size, 'bytes', len(names), 'cases')


if __name__ == '__main__':
    main()
