"""The W2VV++ model's training graph restated as a CPU torch graph in float64 or float32, built from a case of the fixture
tests/golden/train_step_w2vvpp.<case>[.<n>].npz (tools/gen_golden_train_w2vvpp.py): the two concat towers -- one TransformNet each over
the concatenated features, in training mode with dropout 0: fc1 + tanh, BatchNorm1d on batch statistics -- and the margin ranking loss
on the 2-D embeddings (the reference's base-class compute_loss).  The counterpart of tests/tower_ref.py for the concat towers; it takes
the loss, the leaves and the case loader from there and gives the device tests the absolute Jacobian of train_ref.end_to_end_bound.

Also here: device_model (this library's model built from a case, any registry key that builds the concat towers) and train_data."""
import glob
import json
import os

import numpy as np
import torch

import optim_ref  # noqa: F401  (the optimizer the fixture's state is checked against: tests/test_fc_concat_bwd_host.py)
import tower_ref
import train_ref  # noqa: F401  (the bound the device tests apply to abs_jacobian's result)

CASES = ('i', 'ii')
TXT_KEYS = tower_ref.TXT_KEYS
_cache = {}


def load_case(key):
    """({array name: array} over every shard of the case, its meta dict).  Cached: the arrays are shared and must stay unchanged."""
    if key not in _cache:
        arrays = {}
        paths = sorted(glob.glob(os.path.join(tower_ref.GOLDEN, 'train_step_w2vvpp.%s.npz' % key)) +
                       glob.glob(os.path.join(tower_ref.GOLDEN, 'train_step_w2vvpp.%s.*.npz' % key)))
        assert paths, 'no fixture for case %s' % key
        for p in paths:
            with np.load(p) as z:
                for k in z.files:
                    arrays[k] = z[k]
        meta = json.loads(str(arrays.pop('meta')))
        _cache[key] = (arrays, meta)
    return _cache[key]


def _tower(P, prefix, segments, stats, batch_norm):
    x = torch.cat(segments, 1)
    y = torch.tanh(x @ P[prefix + 'fc1.weight'].T + P[prefix + 'fc1.bias'])
    if batch_norm:
        stats[prefix] = (y.detach().mean(0), y.detach().var(0, unbiased=True))
        # (written out, as in tower_ref: torch's fused batch_norm has no batching rule for abs_jacobian's batched backward)
        y = (y - y.mean(0)) / torch.sqrt(y.var(0, unbiased=False) + 1e-5) * P[prefix + 'bn1.weight'] + P[prefix + 'bn1.bias']
    return y


def side_embedding(meta, P, side, inputs, dtype=torch.float64, stats=None):
    """One tower's (N, D) embedding on inputs = (vis {feature: array}, txt {key: array})."""
    vis, txt = inputs
    stats = {} if stats is None else stats
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)        # noqa: E731
    if side == 'txt':
        return _tower(P, 'txt_net.transformer.', [t(txt[TXT_KEYS[n]]) for n in meta['encoder_name_list']], stats, meta['batch_norm'])
    return _tower(P, 'vis_net.', [t(vis[n]) for n in meta['vid_dims']], stats, meta['batch_norm'])


def margin_loss(txt_emb, vis_emb, meta):
    """MarginRankingLoss(margin, 'cosine', max_violation, 'sum', direction)(s = txt, im = vis) on 2-D embeddings: one head."""
    return tower_ref.margin_loss(txt_emb[:, None], vis_emb[:, None], meta)


def step_graph(key, step, dtype=torch.float64, sd=None):
    """The graph of step `step` (1 or 2) of a case from the state the fixture's float64 run had before it (or from `sd`): a dict with the
    leaves P, txt_emb, vis_emb, loss, the BatchNorm batch statistics, and grads {name: d loss / d leaf}."""
    return step_graph_of(*load_case(key), step, dtype, sd)


def step_graph_of(arrays, meta, step, dtype=torch.float64, sd=None):
    if sd is None:
        sd = tower_ref.sub(arrays, 'sd0/') if step == 1 else tower_ref.sub(arrays, 's%d/sd/' % (step - 1))
    P = tower_ref.leaves_of(sd, dtype)
    pre = 's%d/in/' % step
    inputs = (tower_ref.sub(arrays, pre + 'vis/'), tower_ref.sub(arrays, pre + 'txt/'))
    stats = {}
    txt_emb, vis_emb = side_embedding(meta, P, 'txt', inputs, dtype, stats), side_embedding(meta, P, 'vis', inputs, dtype, stats)
    loss = margin_loss(txt_emb, vis_emb, meta)
    names = [k for k in P if P[k].requires_grad]
    gs = torch.autograd.grad(loss, [P[k] for k in names], retain_graph=True, allow_unused=True)
    return dict(P=P, txt_emb=txt_emb, vis_emb=vis_emb, loss=loss, stats=stats, grads=dict(zip(names, gs)), meta=meta, inputs=inputs,
                dtype=dtype)


def abs_jacobian(graph):
    """{name: sum_j |d E_j / d leaf|} over the elements of the leaf's own tower's embedding: the second term of
    train_ref.end_to_end_bound."""
    acc = {}
    for side in ('txt', 'vis'):
        names = [k for k, g in graph['grads'].items() if g is not None and k.startswith(side + '_net.')]
        leaves = [graph['P'][k] for k in names]
        acc.update({k: torch.zeros_like(v) for k, v in zip(names, leaves)})
        E = graph[side + '_emb'].reshape(-1)
        eye = torch.eye(E.numel(), dtype=E.dtype)
        for lo in range(0, E.numel(), 256):
            js = torch.autograd.grad(E, leaves, eye[lo:lo + 256], retain_graph=True, is_grads_batched=True)
            for k, j in zip(names, js):
                acc[k] += j.abs().sum(0)
    return acc


# ---- this library's model built from a case -----------------------------------------------------------------------------------------
def make_cfg(meta, **overrides):
    from laff_amd.config import make_config
    kw = dict(txt_attention='concat', vis_attention='concat', batch_norm=meta['batch_norm'], dropout=meta['dropout'],
              max_violation=meta['max_violation'], direction=meta['direction'], margin=meta['margin'], loss=meta['loss'],
              optimizer=meta['optimizer'], lr=meta['lr'], grad_clip=meta['grad_clip'])
    kw.update(overrides)
    return make_config(meta['vid_dims'], meta['txt_dims'], meta['D'], 1, meta['model'], **kw)


def device_model(key, device='cuda', sd=None, model=None, **overrides):
    """get_model(the case's registry key, or `model`) with the fixture's initial state (or `sd`; float64 arrays are rounded to fp32)
    loaded, in training mode."""
    from laff_amd.model.model import get_model
    arrays, meta = load_case(key)
    net = get_model(model or meta['model'], device, make_cfg(meta, **overrides))
    sd = tower_ref.sub(arrays, 'sd0/') if sd is None else sd
    own = net.state_dict()
    state = {k: torch.as_tensor(np.asarray(v)).to(own[k].dtype) for k, v in sd.items()}
    assert set(state) == set(own), (set(state) ^ set(own))
    net.load_state_dict(state)
    return net.train()


def train_data(key, step, device='cuda'):
    """Fresh input dicts of a step, as W2VVPP.cal_foward reads them."""
    arrays, meta = load_case(key)
    pre = 's%d/in/' % step
    cap = {'caption': ['%d' % i for i in range(meta['N'])]}
    cap.update({tower_ref.ENCODING_KEYS[k]: torch.from_numpy(v.copy()).to(device) for k, v in tower_ref.sub(arrays, pre + 'txt/').items()})
    return {'vis_feats': {k: torch.from_numpy(tower_ref.sub(arrays, pre + 'vis/')[k].copy()).to(device) for k in meta['vid_dims']},
            'captions': cap, 'vis_frame_feat_dict': {}}
