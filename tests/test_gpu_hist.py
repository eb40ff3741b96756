"""The 'hist' measure on a real MI355X: ops.sim_hist against the reference's float64 outputs (tests/golden/hist_sim*.npz) within the
reference's own fp32 error, its layout and edge cases, and the function / model surface built on it.

Tolerance everywhere: 4 e_ref + 2^-23, e_ref = the reference's own max |fp32 - float64| on the same inputs (read from the fixture, or
evaluated here with torch on the CPU where the inputs are the test's own).  Factor 4: the kernel sums in another order and takes the
union from the row sums; 2^-23 is one ulp at 1.0, for cases whose e_ref is 0."""
import numpy as np
import pytest
import torch

import hist_ref as R
from conftest import GOLDEN
from laff_amd import evaluation, loss, ops
from laff_amd.config import make_config
from laff_amd.model import get_model
from laff_amd.model.model import TransformNet

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ULP = 2.0 ** -23
ALL = [(c, k) for c in R.CASES for k in R.kinds_of(c)]


@pytest.fixture(scope='module')
def fx():
    return R.load_fixture(GOLDEN)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def ref_error(T, V, heads, eps):
    """the reference formula in fp32 (torch, CPU) against float64: (its error e, the float64 result)"""
    t, v = torch.as_tensor(np.asarray(T, dtype=np.float32)), torch.as_tensor(np.asarray(V, dtype=np.float32))
    t, v = t.reshape(t.shape[0], heads, -1), v.reshape(v.shape[0], heads, -1)
    s32 = torch.stack([torch.minimum(t[:, None, h], v[None, :, h]).sum(-1) / (torch.maximum(t[:, None, h], v[None, :, h]).sum(-1) + eps)
                       for h in range(heads)], 0).mean(0).numpy()
    s64 = R.hist_sim(T, V, heads, eps)
    return float(np.abs(s32 - s64).max()), s64


def close(got, want, e, what=''):
    err, tol = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()), 4 * e + ULP
    print('%s err %.3e  tol %.3e  (e_ref %.3e)' % (what, err, tol, e))
    assert err <= tol, what


@pytest.mark.parametrize('c,kind', ALL, ids=['%s-%s' % (R.case_name(c), k) for c, k in ALL])
def test_accuracy_against_the_reference_float64(fx, c, kind):
    p = '%s/%s/' % (R.case_name(c), kind)
    Nt, Nv, K, H = c
    T, V, e = dev(fx[p + 'T']), dev(fx[p + 'V']), float(fx[p + 'e_ref'])
    S = ops.sim_hist(T, V, heads=H, eps=R.EPS)
    assert S.shape == (Nt, Nv) and S.dtype == torch.float32
    close(S.cpu().numpy(), fx[p + 'out64'], e, p)
    if H > 1:
        S3 = ops.sim_hist(T.view(Nt, H, -1), V.view(Nv, H, -1), eps=R.EPS)
        assert torch.equal(S3, S)
        close(S3.cpu().numpy(), fx[p + 'out64'], e, p + '3-D')


def test_padding_columns_of_a_pitched_output_are_never_written():
    g = np.random.default_rng(3)
    T, V = g.random((3, 5), dtype=np.float32), g.random((1030, 5), dtype=np.float32)
    out = ops.alloc_scores(3, 1030, torch.device(DEV, torch.cuda.current_device()))
    assert out.stride(0) == 1056
    whole = out.as_strided((3, 1056), (1056, 1))
    whole.fill_(-7.0)
    S = ops.sim_hist(dev(T), dev(V), eps=R.EPS, out=out)
    assert S.data_ptr() == out.data_ptr()
    e, want = ref_error(T, V, 1, R.EPS)
    close(S.cpu().numpy(), want, e, 'pitched')
    assert bool((whole[:, 1030:] == -7.0).all())


def test_row_views_with_a_pitch_give_bitwise_the_contiguous_result(fx):
    for c in [(130, 65, 515, 1), (64, 257, 128, 8)]:
        p = '%s/sigmoid/' % R.case_name(c)
        Nt, Nv, K, H = c
        T, V = dev(fx[p + 'T']), dev(fx[p + 'V'])
        wide_t, wide_v = torch.full((Nt, K + 6), 9.0, device=DEV), torch.full((Nv, K + 3), 9.0, device=DEV)
        wide_t[:, 1:1 + K], wide_v[:, 1:1 + K] = T, V
        tv, vv = wide_t[:, 1:1 + K], wide_v[:, 1:1 + K]
        assert tv.data_ptr() % 16 == 4 and tv.stride(0) == K + 6
        assert torch.equal(ops.sim_hist(tv, vv, heads=H, eps=R.EPS), ops.sim_hist(T, V, heads=H, eps=R.EPS))


def test_a_preallocated_out_is_honoured_and_a_wrong_one_refused():
    T, V = torch.rand(9, 20, device=DEV), torch.rand(11, 20, device=DEV)
    out = torch.empty(9, 11, device=DEV)
    S = ops.sim_hist(T, V, out=out)
    assert S.data_ptr() == out.data_ptr() and torch.equal(out, ops.sim_hist(T, V))
    with pytest.raises(ValueError, match=r'out must be \(9, 11\)'):
        ops.sim_hist(T, V, out=torch.empty(11, 9, device=DEV))
    with pytest.raises(TypeError):
        ops.sim_hist(T, V.double())
    with pytest.raises(ValueError, match='differ in heads or width'):
        ops.sim_hist(T, V[:, :19])


def test_degenerate_rows():
    g = np.random.default_rng(5)
    T, V = g.random((6, 40), dtype=np.float32), g.random((9, 40), dtype=np.float32)
    T[2] = 0
    V[4] = 0
    S = ops.sim_hist(dev(T), dev(V), eps=R.EPS).cpu().numpy()
    e, want = ref_error(T, V, 1, R.EPS)
    assert S[2, 4] == 0.0                                                 # zero x zero
    assert (S[2] == 0.0).all() and (S[:, 4] == 0.0).all()                # zero x non-negative
    close(S, want, e, 'degenerate')                                       # every other entry is what it is without the zero rows
    S0 = ops.sim_hist(dev(T), dev(V), eps=0.0).cpu().numpy()
    assert np.isnan(S0[2, 4]) and np.isnan(S0).sum() == 1                 # IEEE 0 / 0, and only there
    keep = ~np.isnan(S0)
    close(S0[keep], R.hist_sim(T, V, 1, 0.0)[keep], e, 'eps = 0')
    Tn, Vn = -g.random((2, 40), dtype=np.float32) - 0.5, -g.random((3, 40), dtype=np.float32) - 0.25     # negative-valued pairs
    e, want = ref_error(Tn, Vn, 1, R.EPS)
    assert want.min() > 1                                                 # min is the more negative side: |sum min| > |sum max|
    close(ops.sim_hist(dev(Tn), dev(Vn), eps=R.EPS).cpu().numpy(), want, e, 'negative')


def test_an_empty_side_gives_an_empty_matrix():
    T, V = torch.rand(4, 12, device=DEV), torch.rand(5, 12, device=DEV)
    assert ops.sim_hist(T[:0], V).shape == (0, 5) and ops.sim_hist(T, V[:0]).shape == (4, 0)
    assert ops.sim_hist(T.view(4, 3, 4)[:0], V.view(5, 3, 4)).shape == (0, 5)


def test_two_runs_are_bitwise_equal(fx):
    p = 't130v65k515h1/sigmoid/'
    T, V = dev(fx[p + 'T']), dev(fx[p + 'V'])
    assert torch.equal(ops.sim_hist(T, V, eps=R.EPS), ops.sim_hist(T, V, eps=R.EPS))


def test_function_surface_against_the_restatement():
    g = np.random.default_rng(9)
    q, r = g.random((21, 50), dtype=np.float32), g.random((34, 50), dtype=np.float32)
    for fn, eps in ((loss.hist_sim, 1e-14), (loss.jaccard_sim, 1e-8)):
        e, want = ref_error(q, r, 1, eps)
        got = fn(dev(q), dev(r))
        assert got.shape == (21, 34) and got.is_cuda
        close(got.cpu().numpy(), want, e, fn.__name__)
    e, want = ref_error(q, r, 1, 0.0)
    got = evaluation.hist_sim(q, r, device=DEV)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (21, 34)
    close(got, want, e, 'evaluation.hist_sim')
    from laff_amd.model.model import W2VVPP
    e, want = ref_error(q, r, 1, 1e-14)
    close(W2VVPP.compute_sim(dev(q), dev(r), 'hist', device=DEV).cpu().numpy(), want, e, 'compute_sim')
    with pytest.raises(NotImplementedError):                              # the two refusals that stay
        evaluation.compute_sim(q, r, measure='hist')
    with pytest.raises(NotImplementedError):
        loss.MarginRankingLoss(measure='hist')


# ---- model surface -------------------------------------------------------------------------------------------------------
NV, PER, H, D = 20, 3, 2, 64
_SHARED = {}


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
            yield {'vis_feat_dict': {k: torch.from_numpy(v[s:e]) for k, v in self.feats.items()}, 'idxs': list(range(s, e)),
                   'vis_ids': tuple(self.ids[s:e]), 'vis_frame_feat_dict': {}}


class TxtLoader:
    def __init__(self, feats, ids, bs):
        self.feats, self.ids, self.batch_size, self.dataset = feats, ids, bs, _DS(len(ids))

    def __len__(self):
        return (len(self.ids) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, len(self.ids), self.batch_size):
            e = min(len(self.ids), s + self.batch_size)
            cap = {'caption': list(self.ids[s:e])}
            cap.update({k: torch.from_numpy(v[s:e]) for k, v in self.feats.items()})
            yield cap, list(range(s, e)), tuple(self.ids[s:e])


def setup():
    """a small 'LAFF' model (H = 2, d = 32) with 60 captions over 20 videos, ids in the `vid#k` protocol; built once.

    'hist' is the measure of non-negative spaces.  A freshly initialised tower gives unit-norm heads of tanh features centred on zero,
    for which sum max can come out near zero: restated in float64, |S| reaches 8.7 on these very inputs, where two neighbouring fp32
    numbers are 2^-20 apart and no fp32 matrix can be within 2^-22 of anything.  So every FC bias is set to 1: the features are then
    predominantly positive, as concept scores are, and the measure is well conditioned (`well_conditioned` below holds it to that).
    Signed inputs are covered by the fixture's 'signed' kind and by test_degenerate_rows."""
    if not _SHARED:
        g = np.random.default_rng(7)
        cfg = make_config({'a': 64, 'b': 48}, {'bow': 40, 'w2v': 24}, D, H, 'LAFF', [], [])
        torch.manual_seed(11)
        model = get_model('LAFF', DEV, cfg).eval()
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, TransformNet) and m.fc1 is not None:
                    m.fc1.bias.fill_(1.0)
        model.coalesce_loader_batches = False         # one launch set per loader batch: the route embeddings() below takes as well
        vis = {'a': g.normal(0, 1, (NV, 64)).astype(np.float32), 'b': g.normal(0, 1, (NV, 48)).astype(np.float32)}
        vis_ids = ['video%d' % i for i in range(NV)]
        txt_ids = ['video%d#%d' % (i, k) for i in range(NV) for k in range(PER)]
        txt = {'bow_encoding': g.normal(0, 1, (NV * PER, 40)).astype(np.float32),
               'w2v_encoding': g.normal(0, 1, (NV * PER, 24)).astype(np.float32)}
        _SHARED['m'] = model, VisLoader(vis, vis_ids, 8), TxtLoader(txt, txt_ids, 25), txt_ids, vis_ids
    return _SHARED['m']


def embeddings(model, vl, tl):
    with torch.no_grad():
        ve = torch.cat([model.vis_net(b['vis_feat_dict'], vis_frame_feat_dict_input={}) for b in vl], 0)
        te = torch.cat([model.txt_net(c) for c, _, _ in tl], 0)
    return te, ve


def well_conditioned(te, ve):
    """every pair and head has sum max >= (sum |t| + sum |v|) / 4 (twice the fixture generator's margin for its 'signed' kind), so that
    |J| <= 4 for every head, |S| <= 4, and fp32 numbers of S's size are at most 2^-22 apart"""
    t, v = te.cpu().numpy().astype(np.float64), ve.cpu().numpy().astype(np.float64)
    union = np.maximum(t[:, None], v[None]).sum(-1)
    return bool((union >= (np.abs(t).sum(-1)[:, None] + np.abs(v).sum(-1)[None]) / 4).all())


def test_get_txt2vis_matrix_on_the_models_own_embeddings():
    model, vl, tl, _, _ = setup()
    te, ve = embeddings(model, vl, tl)
    assert te.shape == (NV * PER, H, D // H) and ve.shape == (NV, H, D // H) and well_conditioned(te, ve)
    e, want = ref_error(te.cpu().numpy().reshape(NV * PER, -1), ve.cpu().numpy().reshape(NV, -1), H, 1e-14)
    S = model.get_txt2vis_matrix(te, ve, 'hist')
    close(S.cpu().numpy(), want, e, 'get_txt2vis_matrix 3-D')
    assert torch.equal(model.get_txt2vis_matrix(te, ve, 'hist', precision='bf16'), S)          # precision is ignored
    e, want = ref_error(te[:, 1].cpu().numpy(), ve[:, 1].cpu().numpy(), 1, 1e-14)
    close(model.get_txt2vis_matrix(te[:, 1].contiguous(), ve[:, 1].contiguous(), 'hist').cpu().numpy(), want, e, '2-D')
    with pytest.raises(NotImplementedError):
        model.get_txt2vis_matrix(te, ve, 'euclidean')


def test_predict_ranks_are_those_of_the_returned_matrix():
    model, vl, tl, txt_ids, vis_ids = setup()
    S, out_txt, out_vis = model.predict(tl, vl, 'hist')
    assert isinstance(S, np.ndarray) and S.dtype == np.float32 and S.shape == (NV * PER, NV)
    assert list(out_txt) == txt_ids and list(out_vis) == vis_ids
    ranks = model.last_t2v_ranks.cpu().numpy()
    assert model.last_rank_state is None
    Sd, _, _ = model.retrieve(tl, vl, 'hist')
    assert np.array_equal(Sd.cpu().numpy(), S)
    gt = np.arange(NV * PER) // PER
    s_gt = S[np.arange(NV * PER), gt]
    other = np.arange(NV)[None, :] != gt[:, None]
    assert np.array_equal(ranks, 1 + ((S > s_gt[:, None]) & other).sum(axis=1))
    te, ve = embeddings(model, vl, tl)
    assert np.array_equal(model.get_txt2vis_matrix(te, ve, 'hist').cpu().numpy(), S)
    Sb, _, _ = model.predict_batch(tl, vl, 'hist')
    assert np.array_equal(Sb, S)
    cube, _, _ = model.predict_each_head(tl, vl, 'hist')
    assert cube.shape == (H, NV * PER, NV) and well_conditioned(te, ve)
    err = float(np.abs(cube.astype(np.float64).mean(0) - S).max())
    print('mean over heads against predict: err %.3e  bound %.3e' % (err, 2.0 ** -22))
    assert err <= 2.0 ** -22
    with pytest.raises(NotImplementedError):
        model.predict(tl, vl, 'euclidean')


def test_a_column_scatter_works_as_for_cosine():
    model, vl, tl, _, _ = setup()
    S, _, _ = model.predict(tl, vl, 'hist')

    class Shuffled(VisLoader):
        """the same videos handed over in another order, under their dataset indices"""
        def __iter__(self):
            for b in VisLoader.__iter__(self):
                idx = b['idxs'][::-1]
                yield {'vis_feat_dict': {k: torch.from_numpy(self.feats[k][idx]) for k in self.feats}, 'idxs': idx,
                       'vis_ids': tuple(self.ids[i] for i in idx), 'vis_frame_feat_dict': {}}
    shuffled = Shuffled(vl.feats, vl.ids, 8)
    cols = np.concatenate([b['idxs'] for b in shuffled])
    Ss, _, _ = model.predict(tl, shuffled, 'hist')
    assert model.last_t2v_ranks is None and Ss.shape == S.shape
    Sc, _, _ = model.predict(tl, vl, 'cosine')
    Scs, _, _ = model.predict(tl, shuffled, 'cosine')
    # retrieve() gathers the embeddings by dataset index and scatters the columns back through the same list, whatever the measure
    assert np.array_equal(Ss[:, cols], S) and np.abs(Scs[:, cols] - Sc).max() <= 1e-6


def test_cosine_predict_is_bitwise_what_the_existing_route_gives():
    model, vl, tl, _, _ = setup()
    S, _, _ = model.predict(tl, vl, 'cosine')
    ranks = model.last_t2v_ranks.clone()
    assert model.last_rank_state is not None
    te, ve = embeddings(model, vl, tl)
    prec = model.sim_precision or model.predict_precision
    gt = torch.arange(NV * PER, device=te.device, dtype=torch.int32) // PER
    T, V = ops.pack_rows(te.contiguous(), True, 1e-13, prec), ops.pack_rows(ve.contiguous(), True, 1e-13, prec)
    want, count, _ = ops.exact_ranks(te.contiguous(), ve.contiguous(), T, V, gt)
    assert np.array_equal(want.cpu().numpy(), S) and torch.equal(count + 1, ranks)
    plain = model.get_txt2vis_matrix(te, ve, 'cosine', prec)
    assert float((plain - want).abs().max()) <= 1e-6                      # the resolved matrix is the plain GEMM's, to its band
