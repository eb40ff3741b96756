"""The 'LAFF' model with both attentions 'my_self_attention' on the MI355X: the two cases of the training-step fixture (the reference's
own model, tools/gen_golden_selfattn.py) under the rules and the code of tests/train_step_check.py -- embeddings, loss, every raw
gradient, the total norm, the post-step parameters and optimizer state, the running statistics; step one and teacher-forced step two --
then back to inference, and predict / retrieve / predict_each_head.  tests/selfattn_tower.py makes the harness know the two cases.
"""
import numpy as np
import pytest
import torch

import selfattn_tower
import tower_ref
import train_step_check as SC

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = tuple(selfattn_tower.CASES)


@pytest.mark.parametrize('key', KEYS)
def test_step_one_against_the_fixture(key):
    net = SC.check_step(key, 1)
    for tower in (net.vis_net, net.txt_net):
        assert type(tower.attention_layer).__name__ == 'Multi_head_MyApply_selfAttention'
        assert tower.attention_layer.output_type == selfattn_tower.CASES[key]


@pytest.mark.parametrize('key', KEYS)
def test_teacher_forced_step_two(key):
    """From the fixture's own state after step 1 (parameters, running statistics, RMSprop's square_avg), on step 2's inputs."""
    SC.check_step(key, 2)


@pytest.mark.parametrize('key', KEYS)
def test_back_to_inference_after_a_step(key):
    SC.back_to_inference_after_a_step(key)


def _model(output_type, seed=3):
    from laff_amd.model.model import get_model
    _, meta = tower_ref.load_case('sa_mean')
    torch.manual_seed(seed)
    net = get_model('LAFF', DEV, tower_ref.make_cfg(dict(meta, output_type=output_type)))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for tower in (net.vis_net, net.txt_net):
            ln = tower.attention_layer.layer_norm
            ln.weight.copy_(0.5 + torch.rand(ln.weight.shape, generator=g))
            ln.bias.copy_(0.3 * torch.randn(ln.bias.shape, generator=g))
    return net


# ---- predict / retrieve ---------------------------------------------------------------------------------------------------------
NV, NT = 12, 40


class _DS:
    def __init__(self, n):
        self.length = n

    def __len__(self):
        return self.length


class _VisLoader:
    def __init__(self, feats, ids, bs):
        self.feats, self.ids, self.batch_size, self.dataset = feats, ids, bs, _DS(len(ids))

    def __len__(self):
        return (len(self.ids) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, len(self.ids), self.batch_size):
            e = min(len(self.ids), s + self.batch_size)
            yield {'vis_feat_dict': {k: torch.from_numpy(v[s:e]) for k, v in self.feats.items()}, 'idxs': list(range(s, e)),
                   'vis_ids': tuple(self.ids[s:e]), 'vis_frame_feat_dict': {}}


class _TxtLoader(_VisLoader):
    def __iter__(self):
        for s in range(0, len(self.ids), self.batch_size):
            e = min(len(self.ids), s + self.batch_size)
            cap = {'caption': list(self.ids[s:e])}
            cap.update({k: torch.from_numpy(v[s:e]) for k, v in self.feats.items()})
            yield cap, list(range(s, e)), tuple(self.ids[s:e])


@pytest.mark.parametrize('output_type', ['mean', 'Attention_1'])
def test_retrieve_ranks_are_those_of_the_float64_cosines_and_each_head_agrees(output_type):
    """The embeddings are not unit-norm under 'mean': the exact-rank route of retrieve() must not assume that they are."""
    _, meta = tower_ref.load_case('sa_mean')
    net = _model(output_type).eval()
    g = np.random.default_rng(5)
    vis = {k: g.normal(0, 1, (NV, w)).astype(np.float32) for k, w in meta['vid_dims'].items()}
    txt = {'bow_encoding': (g.uniform(0, 1, (NT, meta['txt_dims']['bow'])) < 0.2).astype(np.float32),
           'w2v_encoding': g.normal(0, 1, (NT, meta['txt_dims']['w2v'])).astype(np.float32),
           'CLIP_encoding': g.normal(0, 1, (NT, meta['txt_dims']['CLIP'])).astype(np.float32)}
    owner = np.arange(NT) % NV
    vis_ids, txt_ids = ['video%d' % i for i in range(NV)], ['video%d#%d' % (owner[k], k) for k in range(NT)]
    vl, tl = _VisLoader(vis, vis_ids, 5), _TxtLoader(txt, txt_ids, 16)
    S, out_txt, out_vis = net.retrieve(tl, vl, 'cosine')
    assert list(out_txt) == txt_ids and list(out_vis) == vis_ids and tuple(S.shape) == (NT, NV)
    with torch.no_grad():
        ve = torch.cat([net.vis_net(b['vis_feat_dict'], vis_frame_feat_dict_input={}) for b in vl], 0).cpu().double()
        te = torch.cat([net.txt_net(c) for c, _, _ in tl], 0).cpu().double()
    H = te.shape[1]
    if output_type == 'mean':
        assert float((te.pow(2).sum(2).sqrt() - 1).abs().max()) > 0.1                              # far from unit rows
    tn, vn = (x / (x.pow(2).sum(2, keepdim=True).sqrt() + 1e-13 + 1e-14) for x in (te, ve))
    cube = torch.einsum('thd,vhd->htv', tn, vn)
    want = cube.mean(0)
    s_gt = want[torch.arange(NT), torch.as_tensor(owner)]
    other = torch.arange(NV)[None, :] != torch.as_tensor(owner)[:, None]
    ranks = 1 + ((want > s_gt[:, None]) & other).sum(1)
    assert torch.equal(net.last_t2v_ranks.cpu().long(), ranks)
    assert float((S.cpu().double() - want).abs().max()) <= 1e-4
    Sp, _, _ = net.predict(tl, vl, 'cosine')
    assert np.array_equal(Sp, S.cpu().numpy())
    each, _, _ = net.predict_each_head(tl, vl, 'cosine')
    assert each.shape == (H, NT, NV) and float(np.abs(each.astype(np.float64) - cube.numpy()).max()) <= 1e-4
