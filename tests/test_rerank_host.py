"""Re-ranking without a GPU: the float64 restatement (tests/rerank_ref.py) against the reference's own outputs
(tests/golden/rerank.npz), the integer forms the kernels use, the C entry points' argument checks and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rerank_ref as R
from conftest import ROOT

CASES = ['q1g40k5', 'q3g70k6', 'q2g60k7', 'q5g130k20', 'q2g50k6asym']


def case(z, name):
    Q, G, k1, k2, topk = (int(v) for v in z[name + '/params'])
    return dict(Q=Q, G=G, k1=k1, k2=k2, topk=topk, q_g=z[name + '/q_g'], q_q=z[name + '/q_q'], g_g=z[name + '/g_g'])


def test_fixture_holds_the_cases_the_feature_is_specified_on(golden):
    z = golden('rerank')
    got = {tuple(int(v) for v in z[n + '/params'][:4]) for n in CASES}
    assert {(1, 40, 5, 3), (3, 70, 6, 1), (2, 60, 7, 2), (5, 130, 20, 6)} <= got and len(got) == 5
    a = z['q2g50k6asym/g_g']
    assert np.abs(a - a.T).max() > 1e-3                                  # deliberately non-symmetric
    for n in CASES:
        c = case(z, n)
        assert z[n + '/q_g'].dtype == z[n + '/out32'].dtype == np.float32 and z[n + '/out64'].dtype == np.float64
        assert z[n + '/out32'].shape == z[n + '/out64'].shape == (c['Q'], c['G'])
        assert float(z[n + '/gap']) >= 1e-6 and R.neighbour_gap(c['q_g'], c['q_q'], c['g_g'], c['k1']) == pytest.approx(float(z[n + '/gap']))
        assert float(z[n + '/e_ref']) == float(np.abs(z[n + '/out32'] - z[n + '/out64']).max()) <= 1e-6


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(golden, name):
    z = golden('rerank')
    c = case(z, name)
    got = R.re_ranking(c['q_g'], c['q_q'], c['g_g'], k1=c['k1'], k2=c['k2'])
    assert np.abs(got - z[name + '/out64']).max() <= 1e-12
    assert np.abs(got - z[name + '/out32']).max() <= float(z[name + '/e_ref']) + 1e-12
    tkb = R.re_ranking_tkb_simple(c['q_g'], c['q_q'], c['g_g'], topK=c['topk'], k1=c['k1'])
    assert np.abs(tkb - z[name + '/tkb64']).max() <= 1e-12
    assert np.abs(tkb - z[name + '/tkb32']).max() <= float(z[name + '/e_tkb']) + 1e-12
    assert (tkb == 0).sum(axis=1).tolist() == [c['G'] - c['topk']] * c['Q']


def test_transposed_gallery_block_gives_another_result(golden):
    """D reads COLUMN i of the block matrix: the non-symmetric case tells it from a row read."""
    z = golden('rerank')
    c = case(z, 'q2g50k6asym')
    wrong = R.re_ranking(c['q_g'], c['q_q'], np.ascontiguousarray(c['g_g'].T), k1=c['k1'], k2=c['k2'])
    assert np.abs(wrong - z['q2g50k6asym/out64']).max() > 1e-3


def test_integer_forms_agree_with_the_reference_expressions():
    for k1 in range(1, 33):
        assert R.round_half_even(k1) == int(np.around(k1 / 2)), k1
    assert R.round_half_even(5) == 2 and R.round_half_even(7) == 4
    for n_set in range(0, 34):                                            # |R(c, kh)| <= kh + 1 <= 17; up to a full list of 33
        for n_both in range(0, n_set + 1):
            assert R.overlap_int(n_both, n_set) == R.overlap_float(n_both, n_set), (n_both, n_set)


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()

    def ws(sizes, k1=20, k2=6):
        arr = (_lib.RerankProblem * len(sizes))()
        for a, (Q, G) in zip(arr, sizes):
            a.Q, a.G = Q, G
        return lib.laff_rerank_workspace_bytes(arr, len(sizes), k1, k2, C.byref(n))

    def pad(b):
        return (b + 255) // 256 * 256
    # N = 3001 at the defaults: cap = 21 * 12 = 252, L2 = min(6 * 252, 3001) = 1512
    N = 3001
    want = pad(N * 21 * 4) + 3 * pad(N * 4) + 2 * pad(N * 252 * 4) + 2 * pad(N * 1512 * 4)
    assert ws([(1, 3000)]) == 0 and n.value == want
    assert ws([(1, 3000), (1, 3000)]) == 0 and n.value == 2 * want
    assert ws([(3, 70)], 6, 1) == 0 and n.value == pad(73 * 7 * 4) + 2 * pad(73 * 4) + 2 * pad(73 * 35 * 4)    # k2 = 1: V is not copied
    assert ws([]) == 0 and n.value == 0
    assert ws([(1, 40)], 33) == -5 and b'k1=33' in lib.laff_last_error()
    assert ws([(1, 40)], 0) == -5 and b'k1=0' in lib.laff_last_error()
    assert ws([(1, 40)], 20, 9) == -5 and b'k2=9' in lib.laff_last_error()
    assert ws([(1, 40)], 5, 7) == -5 and b'k2=7' in lib.laff_last_error()           # k2 <= k1 + 1
    assert ws([(1, 40)], 20, 0) == -5 and b'k2=0' in lib.laff_last_error()
    assert ws([(1, 40), (1, 4096)]) == -5 and b'problem 1: N=Q+G=4097' in lib.laff_last_error()
    assert ws([(1, 19)]) == -5 and b'N=Q+G=20' in lib.laff_last_error()            # fewer items than a neighbour list
    assert ws([(0, 40)]) == -5 and ws([(1, 0)]) == -5
    assert ws([(1, 4095)], 32, 8) == 0
    assert lib.laff_rerank_workspace_bytes(None, 1, 20, 6, C.byref(n)) == -1

    fake = 4096                                                         # never dereferenced: every call below fails its checks first

    def run(Q=1, G=40, k1=20, k2=6, lam=0.3, qq=fake, ldqg=None, w=C.c_void_p(4096), wb=1 << 30, P=1):
        arr = (_lib.RerankProblem * 1)()
        a = arr[0]
        a.qq, a.qg, a.gg, a.out, a.Q, a.G = qq, fake, fake, fake, Q, G
        a.ldqq, a.ldqg, a.ldgg, a.ldo = Q, G if ldqg is None else ldqg, G, G
        return lib.laff_rerank_run(None, arr, P, k1, k2, lam, w, wb)
    assert run(k1=33) == -5 and lib.laff_last_error().startswith(b'laff_rerank_run: k1=33')
    assert run(G=4096) == -5 and b'N=Q+G=4097' in lib.laff_last_error()
    assert run(lam=1.5) == -1 and b'lambda_value' in lib.laff_last_error()
    assert run(qq=None) == -1 and b'null pointer' in lib.laff_last_error()
    assert run(ldqg=39) == -2 and b'pitch' in lib.laff_last_error()
    assert run(wb=16) == -1 and b'workspace too small' in lib.laff_last_error()
    assert run(w=None) == -1 and b'workspace too small' in lib.laff_last_error()
    assert run(w=C.c_void_p(4100)) == -3 and b'256-byte aligned' in lib.laff_last_error()
    assert run() == -1 and b'null ctx' in lib.laff_last_error()         # valid arguments: only then the ctx
    assert run(P=0) == 0                                                # no problem: nothing to launch

    p = C.c_void_p(4096)
    assert lib.laff_rerank_tkb(None, p, 40, 41, p, 1, 20, p, p, 40) == -2 and b'k1=41' in lib.laff_last_error()
    assert lib.laff_rerank_tkb(None, p, 40, 6, p, 1, 41, p, p, 40) == -2
    assert lib.laff_rerank_tkb(None, p, 40, 6, p, 1, 20, p, p, 39) == -2
    assert lib.laff_rerank_tkb(None, None, 40, 6, p, 1, 20, p, p, 40) == -1 and b'null argument' in lib.laff_last_error()
    assert lib.laff_rerank_tkb(None, p, 40, 6, p, 1, 20, p, p, 40) == -1 and b'null ctx' in lib.laff_last_error()


def test_python_surface_refuses_what_the_kernels_do_not_support():
    """The limits raise before anything is moved to a device (there is no CPU path to fall back to)."""
    from laff_amd.model import ReRank
    g = np.random.default_rng(0)
    qg, qq, gg = (g.random(s).astype(np.float32) for s in ((1, 40), (1, 1), (40, 40)))
    with pytest.raises(RuntimeError, match='k1=33'):
        ReRank.re_ranking(qg, qq, gg, k1=33)
    with pytest.raises(RuntimeError, match='k2=9'):
        ReRank.re_ranking(qg, qq, gg, k2=9)
    with pytest.raises(RuntimeError, match='N=Q.G=20'):
        ReRank.re_ranking(qg[:, :19], qq, gg[:19, :19])
    with pytest.raises(ValueError, match='blocks must be'):
        ReRank.re_ranking(qg, qq, gg[:, :39])
    with pytest.raises(ValueError, match='k1=41'):
        ReRank.re_ranking_tkb_simple(qg, qq, gg, k1=41)
    with pytest.raises(TypeError, match='all numpy arrays or all device tensors'):
        import torch
        ReRank.re_ranking(qg, torch.ones(1, 1), gg)
    assert not hasattr(ReRank, 'Concept_re_ranking') and not hasattr(ReRank, 'process_query')
    from laff_amd.model.model import W2VVPP
    import inspect
    for name in ('predict_rerank', 'predict_rerank_tkb_simple'):
        assert list(inspect.signature(getattr(W2VVPP, name)).parameters) == [
            'self', 'txt_loader', 'vis_loader', 'measure', 't2i_matrix', 'topK', 'k1', 'reranking_weight', 'return_blocks']


def test_rerank_entry_points_in_header_library_and_binding_at_the_header_abi():
    from laff_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    fields = re.search(r'typedef struct laff_rerank_problem \{(.*?)\} laff_rerank_problem;', text, flags=re.S).group(1)
    names = re.findall(r'(\w+);', fields.replace(', ', '; int '))
    assert names == [n for n, _ in _lib.RerankProblem._fields_]


# ---- the stage-by-stage restatement, its fp32 rendering, the workspace layout and the generated cases ----------------------------
def test_stages_and_re_ranking_are_one_computation(golden):
    z = golden('rerank')
    for n in CASES:
        c = case(z, n)
        s = R.stages(c['q_g'], c['q_q'], c['g_g'], c['k1'], c['k2'], 0.3)
        assert np.array_equal(s['out'], R.re_ranking(c['q_g'], c['q_q'], c['g_g'], k1=c['k1'], k2=c['k2']))
        N = c['Q'] + c['G']
        assert s['rank'].shape == (N, c['k1'] + 1) and s['colmax'].shape == (N,) and len(s['idx1']) == len(s['idx2']) == N
        for i in range(N):
            assert (np.diff(s['idx1'][i]) > 0).all() and (np.diff(s['idx2'][i]) > 0).all()
            assert abs(s['val1'][i].sum() - 1.0) <= 1e-12 and abs(s['val2'][i].sum() - 1.0) <= 1e-12
            assert (s['idx1'][i] is s['idx2'][i]) == (c['k2'] == 1)


@pytest.mark.parametrize('name', CASES)
def test_fp32_rendering_has_the_reference_s_own_fp32_error(golden, name):
    """stages(dtype=float32) is the reference's fp32 computation: on the fixture its distance from float64 is the recorded e_ref
    within a factor 2 either way, and its output is within the project's bound of the reference's fp32 output."""
    import rerank_cases as RC
    z = golden('rerank')
    c = case(z, name)
    s32 = R.stages(c['q_g'], c['q_q'], c['g_g'], c['k1'], c['k2'], 0.3, dtype=np.float32)
    assert s32['out'].dtype == np.float32 and s32['val1'][0].dtype == np.float32 and s32['colmax'].dtype == np.float32
    out64, e_ref = z[name + '/out64'], float(z[name + '/e_ref'])
    e32 = float(np.abs(s32['out'].astype(np.float64) - out64).max())
    print('%-12s e_ref %.3e  rendering %.3e' % (name, e_ref, e32))
    assert e_ref / 2 <= e32 <= 2 * e_ref
    assert np.abs(s32['out'].astype(np.float64) - z[name + '/out32']).max() <= RC.bound(e_ref, out64)


def test_vectorised_expansion_sets_equal_the_loop_form(golden):
    import rerank_cases as RC
    z = golden('rerank')
    todo = [(tuple(case(z, n)[k] for k in ('q_g', 'q_q', 'g_g')), case(z, n)['k1']) for n in CASES]
    todo += [(RC.blocks_of(n)[0], RC.CASES[n][2]) for n in ('n2', 'n6', 'n33_q2', 'n65', 'g129_q5', 'n257')]
    todo.append((RC.ring_blocks(402, 32), 32))
    for blocks, k1 in todo:
        rank = R.neighbour_lists(R.distances(*blocks), k1)
        slow, fast = R.expansion_sets(rank, k1), R.expansion_sets_fast(rank, k1)
        assert len(slow) == len(fast) and all(a == b.tolist() for a, b in zip(slow, fast))


def test_workspace_layout_total_is_the_library_s():
    import torch
    from laff_amd import ops
    combos = [([(1, 1)], 1, 1), ([(1, 1)], 1, 2), ([(1, 5)], 5, 3), ([(1, 32)], 32, 8), ([(2, 31)], 32, 8), ([(3, 60)], 20, 6),
              ([(3, 70)], 6, 1), ([(5, 1025)], 32, 1), ([(2, 4094)], 32, 8), ([(1, 3000)], 20, 6), ([(1, 40)], 7, 2),
              ([(1, 32), (3, 1027), (1, 64), (5, 252)], 32, 8), ([(3, 70), (2, 50), (1, 9)], 6, 3), ([(1, 600), (4, 590)], 31, 1)]
    for sizes, k1, k2 in combos:
        layout, total = R.workspace_layout(sizes, k1, k2)
        assert total == ops.rerank_workspace_bytes(sizes, k1, k2), (sizes, k1, k2)
        assert len(layout) == len(sizes) and all(o % 256 == 0 for d in layout for o, _, _ in d.values())
    sizes, k1, k2 = [(1, 32), (2, 40)], 32, 8
    _, total = R.workspace_layout(sizes, k1, k2)
    ws = torch.zeros(total, dtype=torch.uint8)
    views = R.workspace_views(ws, sizes, k1, k2)
    assert tuple(views[0]['rank'].shape) == (33, 33) and views[0]['rank'].dtype == torch.int32
    assert tuple(views[1]['val2'].shape) == (42, 42) and views[1]['val2'].dtype == torch.float32      # L2 = min(8 * 594, 42)
    end = views[1]['val2'].data_ptr() - ws.data_ptr() + 4 * views[1]['val2'].numel()      # the last piece ends inside the last 256 bytes
    assert total - 256 < end <= total
    one = R.workspace_views(torch.zeros(R.workspace_layout([(3, 70)], 6, 1)[1], dtype=torch.uint8), [(3, 70)], 6, 1)[0]
    assert one['idx2'].data_ptr() == one['idx1'].data_ptr() and one['cnt2'].data_ptr() == one['cnt1'].data_ptr()


def test_generated_cases_meet_their_conditions_and_cover_what_they_are_there_for():
    """Every case of the table: values on the 2^-17 lattice, neighbour gap >= 2e-6 (asserted inside rerank_cases.case, for the tie
    case on all pairs but the planted ones), fp32 lists equal to the float64 lists -- and the coverage the table exists for."""
    import rerank_cases as RC
    cs = {n: RC.case(n) for n in RC.CASES}
    for n, c in cs.items():
        print('%-11s N %4d  gap %.2e  largest cnt1 %3d cnt2 %3d' % (n, c['N'], c['gap'], c['cnt1'], c['cnt2']))
        assert c['gap'] >= 2e-6
    cap = 33 * 18
    for n in RC.SMALLEST:                                              # L1 == N: every list is the whole problem
        c = cs[n]
        assert c['N'] == c['k1'] + 1 and min((c['k1'] + 1) * (R.round_half_even(c['k1']) + 2), c['N']) == c['N']
        assert all(sorted(r.tolist()) == list(range(c['N'])) for r in c['s64']['rank'])
    assert any(min(c['k2'] * cap, c['N']) == c['N'] for c in cs.values() if c['k1'] == 32 and c['k2'] != 1)      # L2 == N
    assert {c['N'] % 4 for c in cs.values()} == {0, 1, 2, 3}
    assert {cs[n]['N'] for n in ('n63', 'n64', 'n65', 'n66', 'n67')} == {63, 64, 65, 66, 67}
    assert [cs[n]['N'] for n in RC.GROUP] == [33, 1030, 65, 257] and all(cs[n]['k1'] == 32 and cs[n]['k2'] == 8 for n in RC.GROUP)
    assert cs['ring']['cnt1'] > 64 and cs['n1030']['cnt1'] > 64        # the second trip of the expansion write-out
    ring = cs['ring']['s64']
    assert cs['ring']['cnt2'] > 512 and len(ring['idx2'][0]) > 256     # the Jaccard scatter's third and second trip
    assert (np.abs(ring['out'] - (0.7 + 0.3 * ring['D'][:, 1:])) > 1e-3).all()      # no output at its trivial value
    # the ring's lists are the ones written down
    offs = np.array(RC.ring_offsets(32))
    assert all(np.array_equal(ring['rank'][1 + i], 1 + (i + offs) % 1028) for i in range(1028))
    # the planted ties: equal values 64, 1 and far apart, inside the list and across its end, resolved to the lower index
    t = cs['ties']
    D = R.distances(*t['blocks'])
    order = np.argsort(D, axis=1, kind='stable')
    seen = set()
    for i, p in t['planted']:
        a, b = int(order[i, p]), int(order[i, p + 1])
        assert D[i, a] == D[i, b] and a < b and (p + 1 <= 32) == (b in t['s64']['rank'][i]) and a in t['s64']['rank'][i]
        seen.add((min(b - a, 2), p))
        assert b - a in (1, 64) or (b - a) % 64 not in (0, 1, 63)
    assert seen == {(1, 4), (2, 4), (1, 32), (2, 32)} and len(t['planted']) == 6
    assert not np.array_equal(t['s64']['rank'], cs['n1030']['s64']['rank'])
