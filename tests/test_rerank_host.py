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
    lib = C.CDLL(_lib.LIB_PATH)
    for s in ('laff_rerank_workspace_bytes', 'laff_rerank_run', 'laff_rerank_tkb'):
        assert re.search(r'\b%s\s*\(' % s, text) and hasattr(lib, s) and s in _lib.SIGNATURES
    abi = re.findall(r'^#define LAFF_ABI_VERSION (\d+)$', text, flags=re.M)
    assert len(abi) == 1 and lib.laff_abi_version() == _lib.ABI_VERSION == int(abi[0]) >= 32
    fields = re.search(r'typedef struct laff_rerank_problem \{(.*?)\} laff_rerank_problem;', text, flags=re.S).group(1)
    names = re.findall(r'(\w+);', fields.replace(', ', '; int '))
    assert names == [n for n, _ in _lib.RerankProblem._fields_]
