"""Pins the float64 fuse restatement (tests/fuse_ref.py) against the fp32 oracle and the reference's golden vectors.  CPU only."""
import numpy as np
import torch

import fuse_ref as R
from oracle import laff_oracle as O

TOL = 2e-6    # fp32 oracle / golden against float64: unit-norm outputs, softmax weights


def close(a, b, tol=TOL):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0
    assert d <= tol, d


def test_attention_1_golden(golden):
    g = golden('attention_1')
    for c in g.json('cases'):
        k = c['key']
        x = g[k + '/x'] if c.get('own_x') else g['x']
        E, a = R.attention(x[:, :, None, :], g[k + '/w'], g[k + '/b'], np.float32(c['gw']), c['with_ave'], c['mul'])
        close(E[:, 0], g[k + '/out'])
        if k + '/weights' in g:
            exp = g[k + '/weights'] - (np.float32(c['gw']) / x.shape[1] if c['with_ave'] else 0)   # (the reference stashes + gw/L)
            close(a[:, 0], exp)
    E, a = R.attention(g['x'][:, :, None, :], just_average=True)
    assert a is None
    close(E[:, 0], g['just_average/out'])


def test_multi_head_golden(golden):
    g = golden('multi_head')
    for c in g.json('cases'):
        k = c['key']
        att = O.attention_from_sd(g.sub(k + '/sd/'), '', c['H'], c['with_ave'], c['mul'], c['split_head'], c['l2norm_each_head'])
        x = g[k + '/x']
        H = c['H']
        d = x.shape[2] // H if c['split_head'] else x.shape[2]
        X = torch.stack([R.dense_plane(x[:, l], H, d, split_head=c['split_head']) for l in range(x.shape[1])], 1)
        E, _ = R.attention(X, att['w'], att['b'], att['gw'], c['with_ave'], c['mul'], c['l2norm_each_head'])
        close(E, g[k + '/out'])


def test_framelaff_golden(golden):
    """The frame vectors of the golden cases without a frame FC (with one, the FC runs over the padded zeros first: not the kernel's
    input)."""
    g = golden('framelaff')
    seen = 0
    for c in g.json('cases'):
        k = c['key']
        if c['vis_frame_addFC'] or k + '/frame_vec' not in g:
            continue
        sd = g.sub(k + '/sd/')
        with_ave, mul = O.FRAME_ATTENTION_FLAGS[c['vis_frame_attention']]
        p = 'vis_net.frame_attention.%s.0.' % c['frame_feats'][0]
        w, b, gw = sd[p + 'embedding_common.0.weight'], sd[p + 'embedding_common.0.bias'], sd[p + 'global_emb_weight_net.weight']
        frames = g[k + '/frames']
        close(R.frame_attention(frames, w, b, gw, with_ave, mul), g[k + '/frame_vec'])
        if k + '/lens' in g:
            close(R.frame_attention(frames, w, b, gw, with_ave, mul, lens=g[k + '/lens']), g[k + '/frame_vec'])
        seen += 1
    assert seen


def test_planes_and_attention_match_the_oracle():
    """Tiled planes with folded affine, deferred activations, per-head l2norm, split and unsplit heads: against
    oracle.multi_head_attention on the planes O.transform_net makes."""
    g = np.random.default_rng(3)
    N, H, d = 23, 3, 20
    D = H * d
    for split_head in (True, False):
        for l2, with_ave, mul in ((False, False, False), (True, True, True), (False, True, False), (True, False, True)):
            ours, theirs = [], []
            for i, act in enumerate(('tanh', 'relu', 'sigmoid', None)):
                tile = split_head and i % 2 == 1
                width = d if (tile or not split_head) else D
                x = g.normal(0, 1, (N, width)).astype(np.float32)
                sc = g.uniform(0.5, 1.5, D if split_head else d).astype(np.float32)
                sh = g.normal(0, 0.1, D if split_head else d).astype(np.float32)
                ours.append(R.dense_plane(x, H, d, tile, split_head, sc, sh, act))
                theirs.append(O.transform_net(x, act=act, bn=None, tile_heads=H if tile else 1) * sc + sh)
            w = g.uniform(-1, 1, (H, d)).astype(np.float32)
            b = g.normal(0, 0.3, H).astype(np.float32)
            gw = g.uniform(0, 1, H).astype(np.float32)
            E, _ = R.attention(torch.stack(ours, 1), w, b, gw, with_ave, mul, l2)
            close(E, O.multi_head_attention(np.stack(theirs, 1), w, b, gw, H, with_ave, mul, split_head, l2))
            A, _ = R.attention(torch.stack(ours, 1), just_average=True)
            if split_head:
                close(A.reshape(N, D), O.just_average(np.stack(theirs, 1)), 1e-6)


def test_single_head_weights_match_attention_1():
    g = np.random.default_rng(4)
    x = g.normal(0, 1, (31, 5, 48)).astype(np.float32)
    w = g.normal(0, 0.3, 48).astype(np.float32)
    for with_ave, mul in ((False, False), (True, True)):
        out, a = O.attention_1(x, w, np.float32(0.2), with_ave, mul, np.float32(0.4), return_weights=True)
        E, aw = R.attention(x[:, :, None, :], w, [0.2], [0.4], with_ave, mul)
        close(E[:, 0], out)
        close(aw[:, 0], a)


def test_gather_plane_is_the_fc_of_the_densified_rows():
    """The CSR gather (out-of-range ids dropped, values None as ones, a row with no ids) against O.transform_net on the dense
    bag-of-words."""
    g = np.random.default_rng(5)
    N, Dk, H, d = 6, 70, 2, 12
    counts = [0, 1, 3, 9, 64, 2]
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = g.integers(-5, Dk + 5, indptr[-1]).astype(np.int32)
    val = g.uniform(0.5, 3, indptr[-1]).astype(np.float32)
    W = g.normal(0, 0.2, (H * d, Dk)).astype(np.float32)
    bias = g.normal(0, 0.1, H * d).astype(np.float32)
    sc, sh = g.uniform(0.5, 1.5, H * d).astype(np.float32), g.normal(0, 0.1, H * d).astype(np.float32)
    for values in (val, None):
        dense = np.zeros((N, Dk), np.float64)
        for n in range(N):
            for p in range(indptr[n], indptr[n + 1]):
                if 0 <= idx[p] < Dk:
                    dense[n, idx[p]] += 1.0 if values is None else values[p]
        ref = O.transform_net(dense.astype(np.float32), W, bias, 'tanh') * sc + sh
        got = R.gather_plane(indptr, idx, values, np.ascontiguousarray(W.T), H, d, bias, sc, sh, 'tanh')
        close(got.reshape(N, H * d), ref, 1e-6)


def test_row_scale_is_the_expert_l2norm():
    g = np.random.default_rng(6)
    x = g.normal(0, 1, (9, 40)).astype(np.float32)
    p = R.dense_plane(x, 4, 10)
    close((p * R.row_scale(p)).reshape(9, 40), O.l2norm(x), 1e-7)
    p1 = R.dense_plane(x[:, :10], 4, 10, split_head=False)
    close((p1 * R.row_scale(p1, split_head=False))[:, 2], O.l2norm(x[:, :10]), 1e-7)


def test_frame_attention_matches_the_oracle():
    """Lens, mask and full length, all four FRAME_ATTENTION_FLAGS, videos of 0, 1 and Fmax frames; frames past a video's length
    hold garbage that the restatement must ignore (the oracle gets them zeroed)."""
    g = np.random.default_rng(7)
    B, Fmax, d = 7, 9, 16
    lens = np.array([0, 1, 3, 9, 8, 4, 9], np.int32)
    frames = g.normal(0, 1, (B, Fmax, d)).astype(np.float32)
    zeroed = frames.copy()
    for i in range(B):
        zeroed[i, lens[i]:] = 0
    mask = np.zeros((B, Fmax + 3), np.float32)
    for i in range(B):
        mask[i, :lens[i]] = 1
    w = g.normal(0, 0.3, d).astype(np.float32)
    for with_ave, mul in O.FRAME_ATTENTION_FLAGS.values():
        ref = O.frame_attention(zeroed, w, np.float32(0.3), with_ave, mul, np.float32(0.6))
        close(R.frame_attention(frames, w, 0.3, 0.6, with_ave, mul, lens=lens), ref)
        close(R.frame_attention(frames, w, 0.3, 0.6, with_ave, mul, mask=mask), ref)
        close(R.frame_attention(zeroed, w, 0.3, 0.6, with_ave, mul), ref)
