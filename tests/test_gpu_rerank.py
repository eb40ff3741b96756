"""Re-ranking on a real MI355X: laff_amd.model.ReRank against the float64 outputs of the reference (tests/golden/rerank.npz) and the
float64 restatement (tests/rerank_ref.py); predict_rerank / predict_rerank_tkb_simple on a synthetic 2-head LAFF model.

The bound of an fp32 result against float64 is the project's rule for an fp32 computation with a different but equally long summation
order: max(2 e_ref, 4 ulp of the largest value), e_ref = the reference's own |fp32 - fp64| on the case.  A flipped set membership
moves a result by ~1e-3 and more.

`pytest -s` prints err, bound and ratio per case; docs/experiments.md ("Re-ranking") is where the ratios are recorded.
"""
import numpy as np
import pytest
import torch

import rerank_cases as RC
import rerank_ref as R
from laff_amd import synth
from laff_amd.model import ReRank

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = ['q1g40k5', 'q3g70k6', 'q2g60k7', 'q5g130k20', 'q2g50k6asym']
_SHARED = {}


def ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def bound(e_ref, want):
    return max(2.0 * float(e_ref), 4.0 * ulp32(want))


def case(z, name):
    Q, G, k1, k2, topk = (int(v) for v in z[name + '/params'])
    return dict(k1=k1, k2=k2, topk=topk, blocks=tuple(z[name + '/' + k] for k in ('q_g', 'q_q', 'g_g')))


def dev_blocks(c):
    return tuple(torch.from_numpy(a).to(DEV) for a in c['blocks'])


def one_at_a_time(golden):
    """every fixture case run alone, device tensors in and out (computed once, compared by several tests)"""
    if 'single' not in _SHARED:
        z = golden('rerank')
        _SHARED['single'] = {n: ReRank.re_ranking(*dev_blocks(case(z, n)), k1=case(z, n)['k1'], k2=case(z, n)['k2']) for n in CASES}
    return _SHARED['single']


@pytest.mark.parametrize('name', CASES)
def test_re_ranking_against_float64(golden, name):
    z = golden('rerank')
    got = one_at_a_time(golden)[name]
    want = z[name + '/out64']
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    err, b = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()), bound(z[name + '/e_ref'], want)
    print('re_ranking %-12s err %.3e  bound %.3e  ratio %.2f' % (name, err, b, err / b))
    assert err <= b


def test_numpy_in_numpy_out_and_other_lambda(golden):
    z = golden('rerank')
    c = case(z, 'q2g60k7')
    got = ReRank.re_ranking(*c['blocks'], k1=c['k1'], k2=c['k2'])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, one_at_a_time(golden)['q2g60k7'].cpu().numpy())
    want = R.re_ranking(*c['blocks'], k1=c['k1'], k2=c['k2'], lambda_value=0.85)
    got = ReRank.re_ranking(*c['blocks'], k1=c['k1'], k2=c['k2'], lambda_value=0.85)
    assert np.abs(got - want).max() <= bound(z['q2g60k7/e_ref'], want)


def test_batched_call_is_bit_identical(golden):
    """Problems of unequal size in ONE launch set (the cases that share k1 = 6), through pitched views, and a list chunked by a small
    byte budget: all bit-identical to the one-at-a-time results."""
    from laff_amd import ops
    z = golden('rerank')
    single = one_at_a_time(golden)
    names = ['q3g70k6', 'q2g50k6asym']
    probs = [dev_blocks(case(z, n)) for n in names]
    for k2 in (1, 3):
        got = ops.rerank_run(probs, 6, k2)
        for n, p, o in zip(names, probs, got):
            alone = single[n] if case(z, n)['k2'] == k2 else ReRank.re_ranking(*p, k1=6, k2=k2)
            assert torch.equal(o, alone), (n, k2)
    # pitched views: the blocks cut out of larger matrices
    qg, qq, gg = probs[0]
    big = torch.full((80, 96), 9.0, device=DEV)
    big[:70, :70] = gg
    bq = torch.full((3, 77), 9.0, device=DEV)
    bq[:, :70] = qg
    got = ops.rerank_run([(bq[:, :70], qq, big[:70, :70]), probs[1]], 6, 1)
    assert torch.equal(got[0], single['q3g70k6'])
    # 20 problems: more than one launch group, chunked by a byte budget that holds three of them
    c = case(z, 'q1g40k5')
    many = [dev_blocks(c) for _ in range(20)]
    need = ops.rerank_workspace_bytes([(1, 40)], c['k1'], c['k2'])
    outs = ReRank.re_ranking_batched(many, k1=c['k1'], k2=c['k2'], budget_bytes=3 * need)
    outs += ops.rerank_run(many, c['k1'], c['k2'])
    assert len(outs) == 40 and all(torch.equal(o, single['q1g40k5']) for o in outs)


@pytest.mark.parametrize('name', CASES)
def test_tkb_simple_counts_exact_and_output_against_float64(golden, name):
    z = golden('rerank')
    c = case(z, name)
    qg, qq, gg = dev_blocks(c)
    count = ReRank.tkb_counts(gg, c['k1'])
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), R.tkb_counts(c['blocks'][2], c['k1']))
    got = ReRank.re_ranking_tkb_simple(qg, qq, gg, topK=c['topk'], k1=c['k1'])
    want = z[name + '/tkb64']
    err, b = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()), bound(z[name + '/e_tkb'], want)
    print('tkb_simple %-12s err %.3e  bound %.3e  ratio %.2f' % (name, err, b, err / b))
    assert err <= b
    assert np.array_equal(got.cpu().numpy() == 0, want == 0)
    host = ReRank.re_ranking_tkb_simple(*c['blocks'], topK=c['topk'], k1=c['k1'])
    assert isinstance(host, np.ndarray) and np.array_equal(host, got.cpu().numpy())


def test_largest_supported_problem_runs_in_bounds():
    """N = 4096 at k1 = 32, k2 = 8 (every limit at once): finite, and the rows it can be checked on cheaply are right -- the
    blend's distance term alone bounds the result: lambda D <= out <= (1 - lambda) + lambda D."""
    g = torch.Generator(device=DEV).manual_seed(5)
    e = torch.nn.functional.normalize(torch.randn(4096, 32, generator=g, device=DEV), dim=1)
    qq, qg, gg = e[:1] @ e[:1].T, e[:1] @ e[1:].T, e[1:] @ e[1:].T
    out = ReRank.re_ranking(qg, qq, gg, k1=32, k2=8)
    assert tuple(out.shape) == (1, 4095) and bool(torch.isfinite(out).all())
    D = R.distances(qg.cpu().numpy(), qq.cpu().numpy(), gg.cpu().numpy())[0, 1:]
    o = out.cpu().numpy()[0].astype(np.float64)
    assert (o >= 0.3 * D - 1e-6).all() and (o <= 0.7 + 0.3 * D + 1e-6).all() and (o < 0.7 + 0.3 * D - 1e-3).any()


# ---- every stage against float64, up to the limits ---------------------------------------------------------------------------------
# The device runs each case once with a workspace the test owns (filled with a sentinel first); what the four kernels left in it
# is compared in the order they ran, so a failure names the first stage that went wrong: rank / colmax (exact), cnt1 / idx1 (the
# expansion sets, and nothing written past them), val1, cnt2 / idx2 (the non-zero pattern after query expansion), val2, the output.
# The bound of val1, val2 and the output is the project's rule with e32 = |fp32 - fp64| of the fp32 rendering of the same stage
# on the same inputs (rerank_cases.case); the lists and sets have no tolerance.
SENT = 0xA5
SENT_I = int(np.frombuffer(bytes([SENT] * 4), dtype=np.int32)[0])


def run_on_device(cases, lambda_value=0.3):
    """the cases as ONE ops.rerank_run call; per case what the workspace holds afterwards, and the output, as numpy"""
    from laff_amd import ops
    k1, k2 = cases[0]['k1'], cases[0]['k2']
    assert all(c['k1'] == k1 and c['k2'] == k2 for c in cases)
    sizes = [(c['Q'], c['G']) for c in cases]
    probs = [tuple(torch.from_numpy(a).to(DEV) for a in c['blocks']) for c in cases]
    ws = torch.full((ops.rerank_workspace_bytes(sizes, k1, k2),), SENT, dtype=torch.uint8, device=DEV)
    outs = ops.rerank_run(probs, k1, k2, lambda_value, workspace=ws)
    views = R.workspace_views(ws, sizes, k1, k2)
    return [dict({k: t.cpu().numpy() for k, t in v.items()}, out=o.cpu().numpy()) for v, o in zip(views, outs)]


def first_bad_row(ok):
    bad = np.flatnonzero(~np.asarray(ok).reshape(len(ok), -1).all(axis=1))
    return 'first wrong row %d of %d wrong' % (bad[0], len(bad)) if len(bad) else 'none'


def report(label, stage, got, want, b):
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('stages %-16s %-4s err %.3e  bound %.3e  ratio %.2f' % (label, stage, err, b, err / b))
    return err


def check_sparse(label, which, c, dev):
    """cnt / idx equal to the float64 index lists, strictly increasing, the rest of every row untouched; val to the bound"""
    want_idx, want_val = c['s64']['idx' + which], c['s64']['val' + which]
    cnt, idx, val = dev['cnt' + which], dev['idx' + which], dev['val' + which]
    N, L = idx.shape
    n = np.array([len(e) for e in want_idx])
    assert N == c['N'] and n.max() <= L
    assert np.array_equal(cnt, n), '%s: cnt%s: %s' % (label, which, first_bad_row(cnt == n))
    used = np.arange(L)[None, :] < n[:, None]
    want = np.full((N, L), SENT_I, dtype=np.int32)
    want[used] = np.concatenate(want_idx)
    assert np.array_equal(idx, want), '%s: idx%s (members, or a write past cnt): %s' % (label, which, first_bad_row(idx == want))
    assert (np.diff(idx.astype(np.int64), axis=1)[used[:, 1:]] > 0).all(), '%s: idx%s not strictly increasing' % (label, which)
    clean = val.view(np.int32) == SENT_I
    assert clean[~used].all(), '%s: val%s written past cnt: %s' % (label, which, first_bad_row(clean | used))
    want = np.concatenate(want_val)
    err = report(label, 'val' + which, val[used], want, c['bound']['val' + which])
    assert err <= c['bound']['val' + which], '%s: val%s' % (label, which)


def check_stages(c, dev, label):
    s = c['s64']
    assert dev['rank'].shape == s['rank'].shape and dev['out'].shape == s['out'].shape == (c['Q'], c['G'])
    assert np.array_equal(dev['rank'], s['rank']), '%s: rank: %s' % (label, first_bad_row(dev['rank'] == s['rank']))
    assert dev['colmax'].dtype == np.float32 and np.array_equal(dev['colmax'].astype(np.float64), s['colmax']), '%s: colmax' % label
    check_sparse(label, '1', c, dev)
    if c['k2'] != 1:
        check_sparse(label, '2', c, dev)
    err = report(label, 'out', dev['out'], s['out'], c['bound']['out'])
    print('stages %-16s largest cnt1 %d cnt2 %d  N %d  gap %.2e' % (label, c['cnt1'], c['cnt2'], c['N'], c['gap']))
    assert np.isfinite(dev['out']).all() and err <= c['bound']['out'], '%s: out' % label


@pytest.mark.parametrize('name', list(RC.CASES))
def test_every_stage_against_float64(name):
    """n4096 is every limit at once (N = 4096, k1 = 32, k2 = 8), every element of every stage compared."""
    c = RC.case(name)
    check_stages(c, run_on_device([c])[0], name)


def test_one_launch_group_of_unequal_problems_every_stage():
    """N = 33, 1030, 65 and 257 in one launch group: grids and LDS slabs sized for the largest, which is not the first."""
    cs = [RC.case(n) for n in RC.GROUP]
    assert [c['N'] for c in cs] == [33, 1030, 65, 257]
    for c, dev in zip(cs, run_on_device(cs)):
        check_stages(c, dev, 'group/' + c['name'])


@pytest.mark.parametrize('lam', [0.0, 1.0])
def test_the_blend_at_its_ends(lam):
    """lambda = 1: the result is D; lambda = 0: the Jaccard term alone (what stages() gives at that lambda), both to the bound"""
    c = RC.case(RC.LAMBDA_CASE, lam)
    dev = run_on_device([c], lam)[0]
    check_stages(c, dev, '%s/lambda=%g' % (c['name'], lam))
    s, Q = c['s64'], c['Q']
    if lam == 1.0:
        assert np.abs(dev['out'].astype(np.float64) - s['D'][:, Q:]).max() <= RC.bound(c['e32']['out'], s['D'][:, Q:])
    else:
        mid = RC.case(RC.LAMBDA_CASE)['s64']
        jac = (mid['out'] - 0.3 * mid['D'][:, Q:]) / 0.7
        assert np.abs(s['out'] - jac).max() <= 1e-12 and s['out'].min() >= 0.0 and (s['out'] < 0.999).any()


def tkb_inputs(seed, Q, G):
    """rows without ties: a permutation of G distinct values each"""
    g = np.random.default_rng(seed)
    base = (np.arange(G, dtype=np.float64) / G).astype(np.float32)
    return g.permuted(np.tile(base, (Q, 1)), axis=1), g.permuted(np.tile(base, (G, 1)), axis=1)


def tkb32(q_g, g_g, topK, k1):
    """the neighbour-count re-ranking with fp32 log, square, sum and division: where its tolerance comes from"""
    count = R.tkb_counts(g_g, k1)
    out = np.zeros(q_g.shape, dtype=np.float32)
    for r in range(q_g.shape[0]):
        cand = np.argsort(-q_g[r].astype(np.float64), kind='stable')[:topK]
        out[r, cand] = np.log((count[cand] + 1).astype(np.float32))
    return out / (np.sqrt((out * out).sum(axis=1, keepdims=True)) + np.float32(1e-13) + np.float32(1e-14))


@pytest.mark.parametrize('Q,G,k1,K', [(1, 1, 1, 1), (2, 7, 7, 7), (2, 7, 3, 0), (0, 7, 3, 4), (0, 7, 7, 0), (3, 300, 300, 300),
                                      (2, 257, 1, 256)])
def test_neighbour_count_kernels_at_their_argument_edges(Q, G, k1, K):
    """ops.rerank_tkb at G = 1, k1 = G, K = G, K = 0 and Q = 0: counts exactly equal, log(count + 1) on the candidates, 0 elsewhere"""
    from laff_amd import ops
    q_g, g_g = tkb_inputs(100 * G + k1, Q, G)
    nn = np.argsort(-g_g.astype(np.float64), axis=1, kind='stable')[:, :k1].astype(np.int32)
    cand = np.argsort(-q_g.astype(np.float64), axis=1, kind='stable')[:, :K].astype(np.int32).reshape(Q, K)
    out, count = ops.rerank_tkb(torch.from_numpy(nn).to(DEV), torch.from_numpy(cand).to(DEV), G)
    want_count = R.tkb_counts(g_g, k1)
    assert count.dtype == torch.int32 and np.array_equal(count.cpu().numpy(), want_count)
    assert k1 != G or (want_count == G + 1).all()
    want = np.zeros((Q, G))
    for r in range(Q):
        want[r, cand[r]] = np.log(want_count[cand[r]] + 1.0)
    got = out.cpu().numpy()
    assert got.shape == (Q, G) and got.dtype == np.float32 and np.array_equal(got == 0, want == 0)
    assert (want == 0).sum() == Q * (G - K)
    if Q and K:
        e32 = np.abs(np.log((want_count + 1).astype(np.float32)).astype(np.float64) - np.log(want_count + 1.0)).max()
        assert np.abs(got - want).max() <= bound(e32, want)


@pytest.mark.parametrize('shape', [(1, 1), (1, 3), (3, 1), (2, 2), (1, 2, 1)])
def test_l2norm_of_fewer_than_four_floats(shape):
    """the row normalisation behind re_ranking_tkb_simple at G = 1: its packed buffer is never shorter than 16 bytes"""
    from laff_amd import loss
    x = (np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1.5) * np.float32(0.75)
    got = loss.l2norm(torch.from_numpy(x).to(DEV), dim=len(shape) - 1).cpu().numpy()
    want = x.astype(np.float64) / (np.sqrt((x.astype(np.float64) ** 2).sum(axis=-1, keepdims=True)) + 1e-13 + 1e-14)
    assert got.shape == shape and np.abs(got - want).max() <= 4 * ulp32(want)


@pytest.mark.parametrize('Q,G,k1,topK', [(1, 1, 1, 1), (2, 7, 7, 7), (2, 7, 7, 3000), (3, 9, 1, 1), (2, 130, 130, 129)])
def test_re_ranking_tkb_simple_at_its_argument_edges(Q, G, k1, topK):
    q_g, g_g = tkb_inputs(100 * G + k1 + topK, Q, G)
    got = ReRank.re_ranking_tkb_simple(torch.from_numpy(q_g).to(DEV), torch.ones(Q, Q, device=DEV), torch.from_numpy(g_g).to(DEV),
                                       topK=topK, k1=k1).cpu().numpy()
    assert np.array_equal(ReRank.tkb_counts(torch.from_numpy(g_g).to(DEV), k1).cpu().numpy(), R.tkb_counts(g_g, k1))
    want = R.re_ranking_tkb_simple(q_g, None, g_g, topK=topK, k1=k1)
    e32 = float(np.abs(tkb32(q_g, g_g, topK, k1) - want).max())
    err, b = float(np.abs(got - want).max()), bound(e32, want)
    print('tkb edge (%d, %d, k1 %d, topK %d) err %.3e  bound %.3e  ratio %.2f' % (Q, G, k1, topK, err, b, err / b))
    assert got.shape == (Q, G) and np.array_equal(got == 0, want == 0) and (want == 0).sum() == Q * (G - min(topK, G))
    assert err <= b


# ---- the predictors ------------------------------------------------------------------------------------------------------------
NV, NT, H, D_HEAD, FEAT, TOPK, K1, SEED = 96, 10, 2, 32, 64, 48, 6, 0
SCORE_TOL = 2e-6          # the project's score tolerance for predict()'s default route (fp16x3 split operands)
TIE_GAP = 2e-6            # a query is left out only if its own blocks have a neighbour gap below this


class _DS:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class VisLoader:
    def __init__(self, feats, bs):
        self.feats, self.n, self.batch_size, self.dataset = feats, next(iter(feats.values())).shape[0], bs, _DS(NV)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, self.n, self.batch_size):
            e = min(self.n, s + self.batch_size)
            yield {'vis_feat_dict': {k: v[s:e] for k, v in self.feats.items()}, 'idxs': list(range(s, e)),
                   'vis_ids': tuple('v%d' % i for i in range(s, e)), 'vis_frame_feat_dict': {}}


class TxtLoader:
    """text batches of 7 and 3: a per-batch row index would address the wrong query in the second batch"""

    def __init__(self, feats, bs=7):
        self.feats, self.n, self.batch_size, self.dataset = feats, next(iter(feats.values())).shape[0], bs, _DS(NT)

    def __len__(self):
        return (self.n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for s in range(0, self.n, self.batch_size):
            e = min(self.n, s + self.batch_size)
            cap = {'caption': ['t%d' % i for i in range(s, e)]}
            cap.update({k: v[s:e] for k, v in self.feats.items()})
            yield cap, list(range(s, e)), tuple('v%d#0' % i for i in range(s, e))


def predict_setup():
    if 'predict' not in _SHARED:
        dev = torch.device('cuda', torch.cuda.current_device())
        model = synth.build_model(H, D_HEAD, dev, feat_dim=FEAT, seed=1234 + SEED)
        vis, txt, _, _ = synth.make_features(NT, NV, dev, feat_dim=FEAT, seed=1234 + SEED)
        vl, tl = VisLoader(vis, 40), TxtLoader(txt)
        t2i, _, _ = model.predict(tl, vl, 'cosine')
        with torch.no_grad():
            ev = model.vis_net(vis, vis_frame_feat_dict_input={}).cpu().numpy().astype(np.float64).reshape(NV, H, -1)
            et = model.txt_net(txt).cpu().numpy().astype(np.float64).reshape(NT, H, -1)
        ev, et = (e / np.linalg.norm(e, axis=2, keepdims=True) for e in (ev, et))
        _SHARED['predict'] = model, vl, tl, np.array(t2i), ev, et
    return _SHARED['predict']


def check_predictor(out, cand, s, gg, t2i, ev, et, term, gap):
    assert out.dtype == np.float32 and out.shape == (NT, NV)
    assert cand.shape == (NT, TOPK) and s.shape == (NT, TOPK) and gg.shape == (NT, TOPK, TOPK)
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1.0).max() <= 1e-6        # unit rows, every query
    kept = 0
    for r in range(NT):
        order = np.argsort(-t2i[r].astype(np.float64), kind='stable')[:TOPK]
        assert np.array_equal(cand[r], order), r                                              # the K best columns, descending
        # the blocks as consumed: float64 cosines (mean over heads) of the fp32 embeddings
        s64 = np.einsum('hd,khd->k', et[r], ev[cand[r]]) / H
        g64 = np.einsum('ihd,jhd->ij', ev[cand[r]], ev[cand[r]]) / H
        assert np.abs(s[r] - s64).max() <= SCORE_TOL and np.abs(gg[r] - g64).max() <= SCORE_TOL, r
        rest = np.setdiff1d(np.arange(NV), cand[r])
        ratio = out[r, rest].astype(np.float64) / t2i[r, rest].astype(np.float64)             # untouched columns: t2i / |row|
        assert np.abs(ratio / ratio[0] - 1.0).max() <= 1e-5, r
        g = gap(s[r][None], gg[r])
        if g < TIE_GAP:
            print('query %d left out: gap %.2e' % (r, g))
            continue
        kept += 1
        row = t2i[r].astype(np.float64)
        row[cand[r]] = s[r].astype(np.float64) + 2.0 * term(s[r][None], gg[r])[0]
        want = R.l2norm_rows(row[None])[0]
        err, b = float(np.abs(out[r] - want).max()), bound(E_REF_PREDICT, want)
        print('query %d gap %.2e  err %.3e  bound %.3e  ratio %.2f' % (r, g, err, b, err / b))
        assert err <= b, r
    assert kept >= 8


#: the reference's own |fp32 - fp64| on the fixture's k1 = 6 cases (9.7e-8, 7.1e-8), its larger one: predict's rows are the same
#: computation at N = 49, scaled by reranking_weight / |row| < 1
E_REF_PREDICT = 9.74e-8


def test_predict_rerank_against_the_restatement_on_its_own_blocks():
    model, vl, tl, t2i, ev, et = predict_setup()
    out, cand, s, gg = model.predict_rerank(tl, vl, 'cosine', t2i, topK=TOPK, k1=K1, return_blocks=True)
    one = np.ones((1, 1))
    check_predictor(out, cand, s, gg, t2i, ev, et, lambda sr, g: R.re_ranking(sr, one, g, k1=K1),
                    lambda sr, g: R.neighbour_gap(sr, one, g, K1))
    plain = model.predict_rerank(tl, vl, 'cosine', t2i, topK=TOPK, k1=K1)
    assert isinstance(plain, np.ndarray) and np.array_equal(plain, out)
    small = model.predict_rerank(tl, vl, 'cosine', t2i, topK=1000, k1=K1)                       # topK above Nv: all 96 candidates
    assert small.shape == (NT, NV) and np.isfinite(small).all()


def test_predict_rerank_tkb_simple_against_the_restatement_on_its_own_blocks():
    model, vl, tl, t2i, ev, et = predict_setup()
    out, cand, s, gg = model.predict_rerank_tkb_simple(tl, vl, 'cosine', t2i, topK=TOPK, k1=K1, return_blocks=True)

    def gap(sr, g):                                                        # the k1 + 1 largest of every gg row, and s itself
        top = -np.sort(-g.astype(np.float64), axis=1)[:, :K1 + 1]
        return float(min(-np.diff(top, axis=1).max(), np.abs(np.diff(np.sort(sr[0].astype(np.float64)))).min()))
    check_predictor(out, cand, s, gg, t2i, ev, et, lambda sr, g: R.re_ranking_tkb_simple(sr, None, g, topK=TOPK, k1=K1), gap)
