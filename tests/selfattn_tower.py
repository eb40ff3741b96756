"""The training-step fixture of the 'LAFF' model with both attentions 'my_self_attention' (tests/golden/train_step_selfattn.<case>.*.npz,
tools/gen_golden_selfattn.py) under the harness of the other training-step cases, tests/tower_ref.py and tests/train_step_check.py.

That harness restates a tower as transform layers + one fusion and reads its cases by key.  Nothing in it is edited: importing this
module registers the two new keys with their file stem and puts two dispatching functions in front of tower_ref._fusion and
tower_ref.make_cfg.  For a case whose meta says attention == 'my_self_attention' they give the self-attention restatement
(tests/selfattn_ref.py) and a config that selects the block; for every other case they call the functions they stand in front of, so
the existing cases run exactly as before.

Cases (settings of case a of tools/gen_golden_train.py: mrl, max_violation, t2i, margin 0.2, RMSprop at 1e-4, grad_clip 2, N 12, D 512,
H 4, BatchNorm on, dropout 0):
    sa_mean   my_self_attention_output_type 'mean'
    sa_att1   'Attention_1' (with_ave, no mul, as attention_param_each_head of that case)
"""
import torch

import selfattn_ref as R
import tower_ref

ATTENTION = 'my_self_attention'
CASES = {'sa_mean': 'mean', 'sa_att1': 'Attention_1'}
STEM = 'train_step_selfattn'

_fusion_before, _make_cfg_before = tower_ref._fusion, tower_ref.make_cfg


def _fusion(P, prefix, planes, meta, dtype, layer='attention_layer', head=None):
    """stack -> Multi_head_MyApply_selfAttention.  head: the planes are that head's columns only and so is the result (N, 1, d); the
    scale stays the whole block's (d // H) ** -0.5."""
    if meta.get('attention') != ATTENTION:
        return _fusion_before(P, prefix, planes, meta, dtype, layer, head)
    assert not meta['expert'] and not meta['l2norm']
    H, d = meta['H'], meta['D'] // meta['H']
    hs = range(H) if head is None else [head]
    att = prefix + layer + '.'
    a1 = None
    if meta['output_type'] == 'Attention_1':
        one = att + 'Attention_list.%d.'
        a1 = {'w': torch.stack([P[one % h + 'embedding_common.0.weight'].reshape(-1) for h in hs]),
              'b': torch.cat([P[one % h + 'embedding_common.0.bias'].reshape(1) for h in hs]),
              'gw': torch.cat([P[one % h + 'global_emb_weight_net.weight'].detach().reshape(1) for h in hs]),
              'with_ave': meta['with_ave'], 'mul': meta['mul']}
    E, _ = R.forward(torch.stack(planes, 1), len(hs), d, P[att + 'layer_norm.weight'], P[att + 'layer_norm.bias'], meta['output_type'],
                     False, a1, training=True, scale=(d // H) ** -0.5)
    return E


def _make_cfg(meta, **overrides):
    if meta.get('attention') != ATTENTION:
        return _make_cfg_before(meta, **overrides)
    kw = dict(vis_attention=ATTENTION, txt_attention=ATTENTION, my_self_attention_output_type=meta['output_type'])
    kw.update(overrides)
    return _make_cfg_before(meta, **kw)


tower_ref._fusion, tower_ref.make_cfg = _fusion, _make_cfg
tower_ref.STEMS.update({k: STEM for k in CASES})
