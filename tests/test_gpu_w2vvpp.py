"""W2VV++ concat towers on a real MI355X: the segmented-K FC kernel against float64, its invariants, the towers and predict() against
the reference's fixture, a W2VV++-sized run.

Kernel tolerance (not a fixed number): per case e_ref = the error of torch-CPU fp32 F.linear on the concatenated input (same epilogue)
against float64; the device must stay within 2 x e_ref (a different but equally long fp32 summation order), floor 4 ulp of the largest
|y|.  The ratios err / bound are printed; the worst seen on an MI355X is recorded in DESIGN.md 4.13.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import w2vvpp_ref as R
from laff_amd import ops
from laff_amd.config import make_config
from laff_amd.model import get_model
from util import load_sd, maxdiff

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TXT_KEY = {'bow_feature': 'bow_encoding', 'w2v_feature': 'w2v_encoding', 'CLIP_encoding': 'CLIP_encoding'}
RATIOS = []


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_rows(g, N, Dk, nnz, repeat=False, empty_row=None, ones=False):
    """Random CSR (indptr, indices, values) with ~nnz entries per row, columns unsorted; repeat: row 0 names one column three times;
    empty_row: that row has no entries; ones: every value is 1."""
    indptr, idx, val = [0], [], []
    for i in range(N):
        k = 0 if i == empty_row else int(g.integers(1, max(2, min(2 * nnz, Dk + 1))))
        cols = g.integers(0, Dk, k)
        if repeat and i == 0 and N > 0:
            cols = np.concatenate([cols, [cols[0] if k else 0] * 2]) if k else np.array([0, 0])
        v = np.ones(len(cols), np.float32) if ones else g.normal(0, 1, len(cols)).astype(np.float32)
        idx += list(cols)
        val += list(v)
        indptr.append(len(idx))
    return np.array(indptr, np.int32), np.array(idx, np.int32), np.array(val, np.float32)


def csr_dense64(csr, N, Dk):
    indptr, idx, val = csr
    d = np.zeros((N, Dk), np.float64)
    for i in range(N):
        for p in range(indptr[i], indptr[i + 1]):
            d[i, idx[p]] += float(val[p])
    return d


def to_torch_csr(csr, N, Dk):
    indptr, idx, val = csr
    return torch.sparse_csr_tensor(dv(indptr), dv(idx), dv(val), size=(N, Dk))


def epilogue64(y, bias, bn, act):
    if bias is not None:
        y = y + bias.astype(np.float64)
    y = R.ACTS[act](y)
    if bn is not None:
        y = y * bn[0].astype(np.float64) + bn[1].astype(np.float64)
    return y


def epilogue32(y, bias, bn, act):
    if bias is not None:
        y = y + torch.from_numpy(bias)
    y = {None: lambda t: t, 'tanh': torch.tanh, 'relu': torch.relu, 'sigmoid': torch.sigmoid}[act](y)
    if bn is not None:
        y = y * torch.from_numpy(bn[0]) + torch.from_numpy(bn[1])
    return y


def run_case(name, seed, N, D, kinds, act='tanh', with_bn=True, with_bias=True, strided=False, repeat=False, empty_row=None, ones=False):
    """kinds: list of ('d', width) / ('s', width).  Returns the device output."""
    g = np.random.default_rng(seed)
    K = sum(w for _, w in kinds)
    W = (g.normal(0, 1, (D, K)) / np.sqrt(max(K, 1))).astype(np.float32)
    bias = g.normal(0, 0.1, D).astype(np.float32) if with_bias else None
    bn = (g.uniform(0.5, 1.5, D).astype(np.float32), g.normal(0, 0.1, D).astype(np.float32)) if with_bn else None
    segs_dev, x64, x32 = [], [], []
    for kind, w in kinds:
        if kind == 'd':
            x = g.normal(0, 1, (N, w)).astype(np.float32)
            if strided:
                buf = torch.full((N, w + 5), float('nan'), device=DEV)
                buf[:, :w] = dv(x)
                segs_dev.append(buf[:, :w])
            else:
                segs_dev.append(dv(x))
            x64.append(x.astype(np.float64))
            x32.append(x)
        else:
            csr = csr_rows(g, N, w, 10, repeat=repeat, empty_row=empty_row, ones=ones)
            segs_dev.append(to_torch_csr(csr, N, w))
            d64 = csr_dense64(csr, N, w)
            x64.append(d64)
            x32.append(d64.astype(np.float32))
    out = ops.fc_concat_act_bn(segs_dev, dv(W), None if bias is None else dv(bias), None if bn is None else dv(bn[0]),
                               None if bn is None else dv(bn[1]), act)
    assert tuple(out.shape) == (N, D)
    if N == 0:
        return out
    ref = epilogue64(np.concatenate(x64, 1) @ W.astype(np.float64).T, bias, bn, act)
    cpu = epilogue32(F.linear(torch.from_numpy(np.concatenate(x32, 1)), torch.from_numpy(W)), bias, bn, act).numpy()
    e_ref = float(np.abs(cpu - ref).max())
    bound = max(2 * e_ref, 4 * float(np.spacing(np.float32(np.abs(ref).max()))))
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), name
    err = float(np.abs(got - ref).max())
    RATIOS.append((err / bound, name))
    print('fc_concat %-34s N=%5d D=%4d K=%5d  err %.3e  e_ref %.3e  bound %.3e  ratio %.3f' % (name, N, D, K, err, e_ref, bound, err / bound))
    assert err <= bound, (name, err, bound)
    return out


def test_kernel_against_float64_over_shapes_segments_and_epilogues():
    s = 1000
    for N in (0, 1, 255, 257, 5000):
        run_case('dense-only N', s, N, 256, [('d', 30), ('d', 50), ('d', 40)]); s += 1
        run_case('sparse-only N', s, N, 256, [('s', 500)]); s += 1
        run_case('mixed N', s, N, 256, [('s', 512), ('d', 50), ('d', 512)]); s += 1
    for D in (4, 256, 2048, 8192):
        run_case('mixed D', s, 257, D, [('d', 500), ('s', 2048), ('d', 1)]); s += 1
    for w in (1, 30, 50, 500, 512, 2048):
        run_case('one dense segment w=%d' % w, s, 255, 256, [('d', w)]); s += 1
        run_case('one sparse segment w=%d' % w, s, 255, 256, [('s', w)]); s += 1
    run_case('8 dense segments', s, 257, 256, [('d', w) for w in (1, 30, 50, 500, 512, 2048, 4, 33)]); s += 1
    run_case('8 mixed segments', s, 257, 256, [('d', 30), ('s', 50), ('d', 500), ('s', 512), ('d', 1), ('s', 2048), ('d', 512), ('s', 1)]); s += 1
    for act in (None, 'tanh', 'relu', 'sigmoid'):
        for with_bn, with_bias in ((True, True), (False, False), (True, False), (False, True)):
            run_case('act %s bn %d bias %d' % (act, with_bn, with_bias), s, 255, 256, [('d', 50), ('s', 500), ('d', 512)], act, with_bn, with_bias); s += 1
    run_case('empty CSR row', s, 255, 256, [('s', 500), ('d', 30)], empty_row=3); s += 1
    run_case('repeated column indices', s, 255, 256, [('s', 500), ('d', 30)], repeat=True); s += 1
    run_case('values = ones', s, 255, 256, [('s', 500), ('d', 512)], ones=True); s += 1
    run_case('strided X (ldx > Dk)', s, 257, 256, [('d', 30), ('d', 512), ('d', 500)], strided=True); s += 1
    worst = max(RATIOS)
    print('fc_concat worst err / bound: %.3f (%s)' % worst)


def _problem(seed, N, D, widths, sparse_at=()):
    g = np.random.default_rng(seed)
    K = sum(widths)
    W = dv((g.normal(0, 1, (D, K)) / np.sqrt(K)).astype(np.float32))
    segs = []
    for j, w in enumerate(widths):
        if j in sparse_at:
            csr = csr_rows(g, N, w, 10)
            segs.append(to_torch_csr(csr, N, w))
        else:
            segs.append(dv(g.normal(0, 1, (N, w)).astype(np.float32)))
    return dict(segments=segs, weight=W, bias=dv(g.normal(0, 0.1, D).astype(np.float32)),
                bn_scale=dv(g.uniform(0.5, 1.5, D).astype(np.float32)), bn_shift=dv(g.normal(0, 0.1, D).astype(np.float32)), activation='tanh')


def test_mixed_launch_equals_dense_launch_on_the_densified_segment():
    q = _problem(5, 300, 256, [500, 50, 512], sparse_at=(0,))
    mixed = ops.fc_concat_act_bn_grouped([q])[0]
    dense = ops.fc_concat_act_bn_grouped([dict(q, segments=[q['segments'][0].to_dense()] + q['segments'][1:])])[0]
    x64 = np.concatenate([s.to_dense().cpu().numpy().astype(np.float64) if s.layout == torch.sparse_csr else s.cpu().numpy().astype(np.float64)
                          for s in q['segments']], 1)
    bn = (q['bn_scale'].cpu().numpy(), q['bn_shift'].cpu().numpy())
    ref = epilogue64(x64 @ q['weight'].cpu().numpy().astype(np.float64).T, q['bias'].cpu().numpy(), bn, 'tanh')
    cpu = epilogue32(F.linear(torch.from_numpy(x64.astype(np.float32)), q['weight'].cpu()), q['bias'].cpu().numpy(), bn, 'tanh').numpy()
    bound = max(2 * np.abs(cpu - ref).max(), 4 * np.spacing(np.float32(np.abs(ref).max())))
    print('mixed vs dense launch: %.3e, bound %.3e' % (maxdiff(mixed, dense), bound))
    assert np.abs(mixed.cpu().numpy() - ref).max() <= bound and np.abs(dense.cpu().numpy() - ref).max() <= bound
    assert maxdiff(mixed, dense) <= bound          # the CSR path against the MFMA path on the same data: the same bound


def test_grouped_equals_single_launches_bitwise_and_rows_do_not_depend_on_the_batch():
    a = _problem(6, 5000, 256, [30, 500, 50], sparse_at=(1,))
    b = _problem(7, 333, 512, [96, 48, 40])
    both = ops.fc_concat_act_bn_grouped([a, b])
    assert torch.equal(both[0], ops.fc_concat_act_bn_grouped([a])[0]) and torch.equal(both[1], ops.fc_concat_act_bn_grouped([b])[0])
    for r in (0, 1, 127, 128, 2571, 4999):           # a row computed alone == the same row inside 5,000
        whole = a['segments'][1]                      # the row's own entries, in their CSR order
        lo, hi = (int(x) for x in whole.crow_indices()[r:r + 2])
        sp = torch.sparse_csr_tensor(torch.tensor([0, hi - lo], dtype=torch.int32, device=DEV), whole.col_indices()[lo:hi].contiguous(),
                                     whole.values()[lo:hi].contiguous(), size=(1, whole.shape[1]))
        alone = ops.fc_concat_act_bn_grouped([dict(a, segments=[a['segments'][0][r:r + 1], sp, a['segments'][2][r:r + 1]])])[0]
        assert torch.equal(alone[0], both[0][r]), r
    sub = ops.fc_concat_act_bn_grouped([dict(b, segments=[s[100:229] for s in b['segments']])])[0]
    assert torch.equal(sub, both[1][100:229])
    with pytest.raises(ValueError, match='out is'):           # a caller's `out` of the wrong shape is refused, not written past
        ops.fc_concat_act_bn_grouped([dict(b, out=torch.empty((10, 512), device=DEV))])


def test_graph_capture_and_replay_equals_eager_and_changed_weights_are_picked_up():
    cfg = make_config({'a': 96, 'b': 48}, {'bow': 30, 'w2v': 50}, 256, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat', batch_norm=True)
    torch.manual_seed(11)
    model = get_model('W2VVPP', DEV, cfg).eval()
    g = np.random.default_rng(12)
    bow = dv((g.random((200, 30)) < 0.2).astype(np.float32)).to_sparse_csr()
    bow = torch.sparse_csr_tensor(bow.crow_indices().to(torch.int32), bow.col_indices().to(torch.int32), bow.values(), size=bow.shape)
    cap = {'caption': ['x'] * 200, 'bow_encoding': bow, 'w2v_encoding': dv(g.normal(0, 1, (200, 50)).astype(np.float32))}
    with torch.no_grad():
        eager = model.txt_net(cap).clone()
        tr = model.txt_net.transformer
        q = dict(segments=[cap['bow_encoding'], cap['w2v_encoding']], weight=tr.fc1.weight.detach(), weight_t={0: tr.weight_t_block(0, 30)},
                 bias=tr.fc1.bias.detach(), bn_scale=tr.bn_affine()[0], bn_shift=tr.bn_affine()[1], activation='tanh',
                 out=torch.zeros((200, 256), device=DEV))
        ops.fc_concat_act_bn_grouped([q])                     # warm-up outside the capture
        torch.cuda.synchronize()
        q['out'].zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.fc_concat_act_bn_grouped([q])
        q['out'].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(q['out'], eager)
        # changed weights / BatchNorm statistics are picked up (caches keyed on data_ptr / _version)
        tr.fc1.weight.mul_(0.5)                               # (in place on the parameter itself: bumps its _version, as load_state_dict does)
        tr.fc1.weight[:, :30] += 0.01
        tr.bn1.running_mean.add_(0.1)
        changed = model.txt_net(cap)
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        ref = R.tower_from_sd(sd, 'txt_net.transformer.', [bow.to_dense().cpu().numpy(), cap['w2v_encoding'].cpu().numpy()])
        assert maxdiff(changed, ref) <= 5e-6 and maxdiff(changed, eager) > 1e-3


class _DS:
    def __init__(self, n):
        self.length = n

    def __len__(self):
        return self.length


class VisLoader:
    def __init__(self, feats, ids, bs):
        self.feats, self.ids, self.batch_size, self.dataset = feats, ids, bs, _DS(len(ids))

    def __len__(self):
        return (len(self.ids) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, len(self.ids), self.batch_size):
            e = min(len(self.ids), s + self.batch_size)
            yield {'vis_feat_dict': {k: torch.from_numpy(np.array(v[s:e])) for k, v in self.feats.items()}, 'idxs': list(range(s, e)),
                   'vis_ids': tuple(self.ids[s:e]), 'vis_frame_feat_dict': {}, 'vis_origin_frame_tuple': (None,) * (e - s)}


class TxtLoader:
    def __init__(self, feats, ids, bs, perm):
        self.feats, self.ids, self.batch_size, self.perm, self.dataset = feats, ids, bs, perm, _DS(len(ids))

    def __len__(self):
        return (len(self.ids) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, len(self.ids), self.batch_size):
            order = self.perm[s:min(len(self.ids), s + self.batch_size)]
            cap = {'caption': [self.ids[i] for i in order]}
            cap.update({k: torch.from_numpy(np.array(v[order])) for k, v in self.feats.items()})
            yield cap, [int(i) for i in order], tuple(self.ids[i] for i in order)


@pytest.mark.parametrize('name', ['W2VVPP', 'w2vpp_mutivis_attention', 'LAFF'])
def test_towers_and_predict_against_the_reference_fixture(golden, name):
    from laff_amd import predictor
    g, gt_ = golden('w2vvpp'), golden('w2vvpp_txt')
    for c in g.json('cases'):
        k = c['key'] + '/'
        cfg = make_config(c['vid_dims'], c['txt_dims'], c['D'], 1, 'W2VVPP', batch_norm=c['batch_norm'], txt_attention='concat',
                          vis_attention='concat')
        model = get_model(name, DEV, cfg).eval()
        res = load_sd(model, g.sub(k + 'sd/'))
        assert not res.unexpected_keys and not res.missing_keys
        sd = g.sub(k + 'sd/')
        vis = {n: g[k + 'vis/' + n] for n in c['vid_dims']}
        txt = {TXT_KEY[n]: v for n, v in g.sub(k + 'txt/').items()}
        perm = g[k + 'perm']
        v64 = R.tower_from_sd(sd, 'vis_net.', [vis[n] for n in c['vid_dims']])
        t64 = R.tower_from_sd(sd, 'txt_net.transformer.', [txt[e][perm] for e in ('bow_encoding', 'w2v_encoding', 'CLIP_encoding')])
        s64 = R.cosine(t64, v64)
        ulp4 = 4 * float(np.spacing(np.float32(g[k + 'emb_absmax'])))
        bound_v, bound_t = max(2 * float(g[k + 'e_ref_vis']), ulp4), max(2 * float(g[k + 'e_ref_txt']), ulp4)
        ve = model.encode_video({n: torch.from_numpy(np.array(v)) for n, v in vis.items()})
        cap = {'caption': ['x'] * len(perm)}
        cap.update({e: torch.from_numpy(np.array(v[perm])) for e, v in txt.items()})
        te = model.encode_text(cap)
        assert ve.dim() == 2 and te.dim() == 2
        ev, et = maxdiff(ve, v64), maxdiff(te, t64)
        print('%s %s: vis %.3e / %.3e  txt %.3e / %.3e  (ratios %.3f %.3f)' % (name, c['key'], ev, bound_v, et, bound_t, ev / bound_v, et / bound_t))
        assert ev <= bound_v and et <= bound_t
        assert maxdiff(ve, g[k + 'video_all_embs']) <= bound_v + float(g[k + 'e_ref_vis'])      # the reference's own rows: its error on top
        assert maxdiff(te, gt_[k + 'txt_emb']) <= bound_t + float(g[k + 'e_ref_txt'])
        # a CSR bag-of-words stays sparse and gives the same embeddings within the same bound
        sp = cap['bow_encoding'].to(DEV).to_sparse_csr()
        cap_sp = dict(cap, bow_encoding=torch.sparse_csr_tensor(sp.crow_indices().to(torch.int32), sp.col_indices().to(torch.int32), sp.values(),
                                                                size=sp.shape))
        assert maxdiff(model.encode_text(cap_sp), t64) <= bound_t
        vis_ids, txt_ids = g.json(k + 'vis_ids'), g.json(k + 'txt_ids')
        vl = VisLoader(vis, vis_ids, c['bs'])
        tl = TxtLoader(txt, txt_ids, c['bs'], perm)
        keep = g[k + 'keep']
        for prec in ('fp16x3', 'fp32'):
            model.sim_precision = prec
            scores, out_txt, out_vis = model.predict(tl, vl, 'cosine', record_emb=False)
            assert list(out_txt) == g.json(k + 'txt_ids_out') and list(out_vis) == g.json(k + 'vis_ids_out')
            es = maxdiff(scores, g[k + 'scores'])
            print('%s %s %s: scores vs the reference %.3e, vs float64 %.3e' % (name, c['key'], prec, es, maxdiff(scores, s64)))
            assert es <= 2e-6
            ranks = model.last_t2v_ranks.cpu().numpy()
            assert np.array_equal(ranks[keep], g[k + 'ranks64'][keep])
            # ranks of our own fp32 embeddings in float64: exact equality, every query
            own = R.cosine(model.txt_net(cap).cpu().numpy(), model.video_all_embs.cpu().numpy())
            gt = predictor.gt_columns(out_txt, out_vis)
            assert np.array_equal(ranks, R.ranks_of_gt(own, np.asarray(gt)))
            # the seven metrics of both directions against the reference's: over the queries that are not near-ties (the fixture's
            # 'keep': 285 of 300 in the 'bn' case, all in 'nobn'), and over all queries where none is left out
            S, _, _ = model.retrieve(tl, vl)
            kept = torch.as_tensor(np.flatnonzero(keep), device=S.device)
            t2v, v2t = predictor.retrieval_metrics(S[kept].contiguous(), [t for t, kk in zip(out_txt, keep) if kk], out_vis)
            np.testing.assert_allclose(t2v, g[k + 't2v_metrics_kept'], rtol=0, atol=1e-9)
            np.testing.assert_allclose(v2t, g[k + 'v2t_metrics_kept'], rtol=0, atol=1e-9)
            if keep.all():
                t2v, v2t = predictor.retrieval_metrics(S, out_txt, out_vis, state=model.last_rank_state)
                np.testing.assert_allclose(t2v, g[k + 't2v_metrics'], rtol=0, atol=1e-9)
                np.testing.assert_allclose(v2t, g[k + 'v2t_metrics'], rtol=0, atol=1e-9)
        model.sim_precision = None
        model.coalesce_loader_batches = False
        try:
            sb, tb, vb = model.predict(tl, vl, 'cosine')
        finally:
            model.coalesce_loader_batches = True
        assert list(tb) == g.json(k + 'txt_ids_out') and maxdiff(sb, g[k + 'scores']) <= 2e-6


def test_concat_on_one_side_attention_on_the_other():
    from oracle import laff_oracle as O
    g = np.random.default_rng(21)
    cfg = make_config({'a': 40, 'b': 24}, {'bow': 30, 'w2v': 20}, 256, 1, 'w2vpp_mutivis_attention', txt_attention='attention_noAveNoAverageMul',
                      vis_attention='concat', batch_norm=True)
    torch.manual_seed(22)
    model = get_model('w2vpp_mutivis_attention', DEV, cfg).eval()
    vis = {'a': g.normal(0, 1, (50, 40)).astype(np.float32), 'b': g.normal(0, 1, (50, 24)).astype(np.float32)}
    txt = {'bow_encoding': g.normal(0, 1, (70, 30)).astype(np.float32), 'w2v_encoding': g.normal(0, 1, (70, 20)).astype(np.float32)}
    ve = model.encode_video({k: torch.from_numpy(v) for k, v in vis.items()})
    te = model.encode_text(dict({k: torch.from_numpy(v) for k, v in txt.items()}, caption=['x'] * 70))
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    v64 = R.tower_from_sd(sd, 'vis_net.', [vis['a'], vis['b']])
    assert ve.dim() == 2 and te.dim() == 2 and maxdiff(ve, v64) <= 5e-6
    planes = [R.tower_from_sd(sd, 'txt_net.transform_layer.%s_transform.' % e, [txt[k]]) for e, k in (('bow_encoder', 'bow_encoding'), ('w2v_encoder', 'w2v_encoding'))]
    pre = 'txt_net.attention_layer.'
    t64 = O.attention_1(np.stack(planes, axis=1), sd[pre + 'embedding_common.0.weight'].reshape(-1), sd[pre + 'embedding_common.0.bias'].reshape(()),
                        False, False, sd[pre + 'global_emb_weight_net.weight'].reshape(()))
    assert maxdiff(te, t64) <= 5e-6
    assert maxdiff(model.get_txt2vis_matrix(te, ve, precision='fp16x3'), R.cosine(t64, v64)) <= 2e-6
    # a concat side against a multi-head side: the ValueError of mismatched ranks, no broadcast
    cfg = make_config({'a': 40}, {'bow': 30}, 256, 4, 'LAFF', vis_attention='concat')
    m2 = get_model('LAFF', DEV, cfg).eval()
    with pytest.raises(ValueError, match='txt_embs'):
        m2.get_txt2vis_matrix(m2.encode_text({'caption': ['x'] * 3, 'bow_encoding': torch.zeros(3, 30)}), m2.encode_video({'a': torch.zeros(5, 40)}))


def test_w2vvpp_sized_run_allocates_no_concatenated_matrix():
    from laff_amd import predictor
    Nt, Nv, D, V = 40000, 10000, 2048, 10000
    g = np.random.default_rng(31)
    cfg = make_config({'resnext': 2048, 'resnet': 2048}, {'rnn': 1024, 'bow': V, 'w2v': 500}, D, 1, 'W2VVPP', txt_attention='concat',
                      vis_attention='concat', batch_norm=True)
    torch.manual_seed(32)
    model = get_model('W2VVPP', DEV, cfg).eval()
    gt = np.arange(Nt) % Nv
    lat = g.normal(0, 1, (Nv, 32)).astype(np.float32)
    mk = lambda z, d: dv((z @ g.normal(0, 1, (32, d)).astype(np.float32) / np.float32(np.sqrt(32)) + 0.5 * g.normal(0, 1, (z.shape[0], d)).astype(np.float32)))
    zt = lat[gt] + 0.3 * g.normal(0, 1, (Nt, 32)).astype(np.float32)
    vis = {'resnext': mk(lat, 2048), 'resnet': mk(lat, 2048)}
    nnz = g.integers(5, 16, Nt)
    indptr = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int32)
    cols = ((gt.repeat(nnz) * 7 + g.integers(0, 40, indptr[-1])) % V).astype(np.int32)
    bow = torch.sparse_csr_tensor(dv(indptr), dv(cols), torch.ones(int(indptr[-1]), device=DEV), size=(Nt, V))
    cap = {'caption': ['x'] * Nt, 'rnn_encoding': mk(zt, 1024), 'bow_encoding': bow, 'w2v_encoding': mk(zt, 500)}
    with torch.no_grad():
        model.txt_net.transformer.weight_t_block(1024, V)         # the cached transposed bow block belongs to the weights
        model.encode_text({'caption': ['x'] * 8, 'rnn_encoding': cap['rnn_encoding'][:8], 'w2v_encoding': cap['w2v_encoding'][:8],
                           'bow_encoding': torch.zeros((8, V), device=DEV)})      # warm-up: BatchNorm folds cached
        model.encode_video({k: v[:8] for k, v in vis.items()})
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        te = model.encode_text(cap)
        ve = model.encode_video(vis)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base
    outputs = 4 * D * (Nt + Nv)
    print('W2VV++-sized run: %.1f MB allocated beyond inputs and weights (outputs %.1f MB; a concatenated text input would be %.1f MB)' % (
        extra / 2**20, outputs / 2**20, 4 * Nt * (1024 + V + 500) / 2**20))
    assert extra <= outputs + 64 * 2**20
    rows = np.unique(np.concatenate([[0, Nt - 1], g.integers(0, Nt, 70)]))
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    bow_rows = np.zeros((len(rows), V))
    for i, r in enumerate(rows):
        np.add.at(bow_rows[i], cols[indptr[r]:indptr[r + 1]], 1.0)
    t64 = R.tower_from_sd(sd, 'txt_net.transformer.', [cap['rnn_encoding'][rows].cpu().numpy(), bow_rows, cap['w2v_encoding'][rows].cpu().numpy()])
    vrows = np.unique(np.concatenate([[0, Nv - 1], g.integers(0, Nv, 70)]))
    v64 = R.tower_from_sd(sd, 'vis_net.', [vis['resnext'][vrows].cpu().numpy(), vis['resnet'][vrows].cpu().numpy()])
    def cpu32(prefix, segs):
        bn = tuple(torch.from_numpy(sd[prefix + 'bn1.' + k]) for k in ('weight', 'bias', 'running_mean', 'running_var'))
        y = torch.tanh(F.linear(torch.from_numpy(np.concatenate(segs, 1).astype(np.float32)), torch.from_numpy(sd[prefix + 'fc1.weight']),
                                torch.from_numpy(sd[prefix + 'fc1.bias'])))
        return F.batch_norm(y, bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5).numpy()
    t32 = cpu32('txt_net.transformer.', [cap['rnn_encoding'][rows].cpu().numpy(), bow_rows, cap['w2v_encoding'][rows].cpu().numpy()])
    v32 = cpu32('vis_net.', [vis['resnext'][vrows].cpu().numpy(), vis['resnet'][vrows].cpu().numpy()])
    bt = max(2 * np.abs(t32 - t64).max(), 4 * np.spacing(np.float32(np.abs(t64).max())))
    bv = max(2 * np.abs(v32 - v64).max(), 4 * np.spacing(np.float32(np.abs(v64).max())))
    et, ev = maxdiff(te[rows], t64), maxdiff(ve[vrows], v64)
    print('W2VV++-sized run: sampled rows vs float64: txt %.3e / %.3e  vis %.3e / %.3e (ratios %.3f %.3f)' % (et, bt, ev, bv, et / bt, ev / bv))
    assert len(rows) >= 64 and len(vrows) >= 64 and et <= bt and ev <= bv
    # exact ranks against the float64 ranks of our own embeddings
    T = ops.pack_rows(te, True, 1e-13, 'fp16x3')
    Vp = ops.pack_rows(ve, True, 1e-13, 'fp16x3')
    gtd = torch.as_tensor(gt, dtype=torch.int32, device=DEV)
    for cap_ in (None, 8 * ops.default_pair_cap(Nt)):          # retrieve()'s own ladder: the default pair list, then an 8x larger one
        S, count, st = ops.exact_ranks(te, ve, T, Vp, gtd, pair_cap=cap_)
        if not st.overflowed():
            break
        del S, count, st
    else:
        raise AssertionError('the pair list overflowed with the 8x list')
    ranks = (count + 1).cpu().numpy()
    q = np.unique(g.integers(0, Nt, 256))
    own = R.cosine(te[q].cpu().numpy(), ve.cpu().numpy())
    assert np.array_equal(ranks[q], R.ranks_of_gt(own, gt[q]))
