#!/usr/bin/env python3
"""tests/golden/w2vvpp.npz: the W2VV++ concat towers and predict() run by the REAL reference (tools/gen_golden.py's stub recipe).

    python tools/gen_golden_w2vvpp.py

Reference symbols exercised (file:line relative to the reference tree): model/model.py:279-308 VisTransformNet, :552-726
MultiScaleTxtEncoder / MultiScaleTxtNet, :751-768 W2VVPP, :1003-1079 get_txt2vis_matrix / predict, :2501-2519 get_model with the
keys 'W2VVPP', 'w2vpp_mutivis_attention' and 'LAFF' (both attentions 'concat'); predictor.py:232-270 re-enacted by gen_golden.

Arrays, id lists and scalars only.  Two cases: 'bn' (batch_norm=True, randomised running statistics) and 'nobn'.  No committed file
of this project may exceed 1 MiB and random fp32 data does not compress, so the reference's text embeddings (loader row order) go
into a second file, tests/golden/w2vvpp_txt.npz; everything else is in tests/golden/w2vvpp.npz.  The reference's own fp32 error
against the float64 restatement (tests/w2vvpp_ref.py) is stored as 'e_ref_*'.

Rank and metric checks against this fixture leave near-ties out: the ground-truth margin of a query is min_v |s - s_gt| over the
float64 scores; queries with a margin <= 1e-5 (the reference's fp32 scores are 1.7e-7 from float64, its closest competitor 1.8e-6)
are left out, and so is a caption whose score for a video is within 1e-5 of that video's own caption's (the video -> text
direction).  'keep' marks the rest, the generator insists on at least 95 % of the queries, and the seven text -> video and video ->
text metrics of the reference over the kept queries alone are stored as 't2v_metrics_kept' / 'v2t_metrics_kept' next to those
over all queries.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
import gen_golden as G  # noqa: E402  (imports the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import w2vvpp_ref as R  # noqa: E402

mm = G.mm
KEYS = ('W2VVPP', 'w2vpp_mutivis_attention', 'LAFF')
VID_DIMS = {'resnext': 96, 'x3d': 48, 'ircsn': 40}
TXT_DIMS = {'bow': 30, 'w2v': 50, 'CLIP': 64}
MARGIN = 1e-5


def concat_cfg(D, batch_norm):
    cfg = G.laff_cfg(VID_DIMS, TXT_DIMS, D, 1, False, False, batch_norm, [], clip_no_transform=False)
    cfg.txt_attention = 'concat'
    cfg.vis_attention = 'concat'
    cfg.txt_fc_same_with_vis_fc = False
    return cfg


def plug(model):
    for name in model.txt_net.encoder.encoder_name_list:
        key = {'bow_encoder': 'bow_feature', 'w2v_encoder': 'w2v_feature', 'CLIP_encoder': 'CLIP_encoding'}[name]
        setattr(model.txt_net.encoder.encoder, name, G.PreExtracted(key))


def case(arrays, txt_arrays, key, seed, Nv, Nt, bs, D, batch_norm):
    g = G.rng(seed)
    torch.manual_seed(seed)
    model = mm.get_model('W2VVPP', torch.device('cpu'), concat_cfg(D, batch_norm)).eval()
    plug(model)
    G.randomize_model(model, g)
    sd_keys = sorted(k for k in model.state_dict() if not k.startswith('txt_net.encoder.'))
    for other in KEYS[1:]:      # the other registry keys build the same two towers
        m2 = mm.get_model(other, torch.device('cpu'), concat_cfg(D, batch_norm))
        assert sorted(k for k in m2.state_dict() if not k.startswith('txt_net.encoder.')) == sd_keys, other
    vis, txt_raw, gt = G.planted(g, Nv, Nt, VID_DIMS, TXT_DIMS)
    txt = {'bow_feature': txt_raw['bow'], 'w2v_feature': txt_raw['w2v'], 'CLIP_encoding': txt_raw['CLIP']}
    vis_ids = ['video%d' % i for i in range(Nv)]
    txt_ids = ['video%d#%d' % (gt[i], i // Nv) for i in range(Nt)]
    perm = np.arange(Nt)
    for s in range(0, Nt, bs):
        e = min(Nt, s + bs)
        perm[s:e] = g.permutation(perm[s:e])
    vloader, tloader = G.FakeVisLoader(vis, vis_ids, bs), G.FakeTxtLoader(txt, txt_ids, bs, perm)
    scores, out_txt_ids, out_vis_ids = model.predict(tloader, vloader, 'cosine', record_emb=True)
    txt_emb = torch.cat([model.txt_net(cap) for cap, _, _ in tloader], dim=0).numpy()       # loader row order
    vis_emb = model.video_all_embs.numpy()

    # float64 restatement: the reference's own error, and the near-tie mask of the rank checks
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    act = 'tanh'
    v64 = R.tower_from_sd(sd, 'vis_net.', [vis[n] for n in VID_DIMS], act)
    t64 = R.tower_from_sd(sd, 'txt_net.transformer.', [txt[k][perm] for k in ('bow_feature', 'w2v_feature', 'CLIP_encoding')], act)
    s64 = R.cosine(t64, v64)
    gt_out = np.array([out_vis_ids.index(t.split('#')[0]) for t in out_txt_ids])
    margin = R.gt_margin(s64, gt_out)
    keep = margin > MARGIN
    for v in range(Nv):                 # video -> text: a caption of another video within MARGIN of one of this video's own captions
        own = np.flatnonzero(keep & (gt_out == v))
        oth = np.flatnonzero(keep & (gt_out != v))
        if len(own) and len(oth):
            near = (np.abs(s64[oth, v][:, None] - s64[own, v][None, :]) <= MARGIN).any(axis=1)
            keep[oth[near]] = False
    assert keep.mean() >= 0.95, 'case %s seed %d: only %.1f %% of the queries have a margin above %g' % (key, seed, 100 * keep.mean(), MARGIN)
    p = key + '/'
    for k, v in vis.items():
        arrays[p + 'vis/' + k] = v
    for k, v in txt.items():
        arrays[p + 'txt/' + k] = v
    for k in sd_keys:
        arrays[p + 'sd/' + k] = sd[k]
    arrays[p + 'perm'] = perm.astype(np.int64)
    arrays[p + 'scores'] = scores.astype(np.float32)
    arrays[p + 'video_all_embs'] = vis_emb
    arrays[p + 'e_ref_vis'] = np.float64(np.abs(vis_emb - v64).max())
    arrays[p + 'e_ref_txt'] = np.float64(np.abs(txt_emb - t64).max())
    arrays[p + 'e_ref_scores'] = np.float64(np.abs(scores - s64).max())
    arrays[p + 'emb_absmax'] = np.float64(max(np.abs(v64).max(), np.abs(t64).max()))
    arrays[p + 'keep'] = keep
    arrays[p + 'min_margin'] = np.float64(margin.min())
    arrays[p + 'ranks64'] = R.ranks_of_gt(s64, gt_out).astype(np.int64)
    t2v, v2t = G.predictor_metrics(scores, list(out_txt_ids), list(out_vis_ids))
    arrays[p + 't2v_metrics'] = np.array(t2v, np.float64)
    arrays[p + 'v2t_metrics'] = np.array(v2t, np.float64)
    t2v, v2t = G.predictor_metrics(scores[keep], [t for t, k in zip(out_txt_ids, keep) if k], list(out_vis_ids))
    arrays[p + 't2v_metrics_kept'] = np.array(t2v, np.float64)
    arrays[p + 'v2t_metrics_kept'] = np.array(v2t, np.float64)
    txt_arrays[p + 'txt_emb'] = txt_emb
    for nm, v in (('txt_ids', txt_ids), ('vis_ids', vis_ids), ('txt_ids_out', list(out_txt_ids)), ('vis_ids_out', list(out_vis_ids))):
        arrays[p + nm] = np.array(json.dumps(v))
    print('%s: kept %d / %d queries, min margin %.2e, e_ref vis %.2e txt %.2e scores %.2e, |y| <= %.2f' % (
        key, keep.sum(), len(keep), margin.min(), arrays[p + 'e_ref_vis'], arrays[p + 'e_ref_txt'], arrays[p + 'e_ref_scores'],
        arrays[p + 'emb_absmax']))
    return dict(key=key, vid_dims=VID_DIMS, txt_dims=TXT_DIMS, D=D, bs=bs, batch_norm=batch_norm, Nv=Nv, Nt=Nt, seed=seed,
                sd_keys=sd_keys, encoder_name_list=list(model.txt_net.encoder.encoder_name_list))


def main():
    arrays, txt_arrays = {}, {}
    cases = [case(arrays, txt_arrays, 'bn', 911, 120, 300, 64, 256, True),
             case(arrays, txt_arrays, 'nobn', 912, 40, 90, 32, 64, False)]
    arrays['cases'] = np.array(json.dumps(cases))
    arrays['registry_keys'] = np.array(json.dumps(list(KEYS)))
    G.save('w2vvpp', **arrays)
    G.save('w2vvpp_txt', **txt_arrays)


if __name__ == '__main__':
    main()
