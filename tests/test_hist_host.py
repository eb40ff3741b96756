"""The 'hist' measure without a GPU: the fixture (tests/golden/hist_sim*.npz) against the float64 restatement (tests/hist_ref.py), the
C entry point's argument checks and the ABI, and the Python surface's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hist_ref as R
from conftest import GOLDEN

ALL = [(c, k) for c in R.CASES for k in R.kinds_of(c)]


@pytest.fixture(scope='module')
def fx():
    return R.load_fixture(GOLDEN)


def test_fixture_holds_exactly_the_cases_the_feature_is_specified_on(fx):
    assert R.CASES == [(1, 1, 1, 1), (5, 7, 3, 1), (65, 130, 37, 1), (130, 65, 515, 1), (33, 129, 111, 3), (64, 257, 128, 8),
                       (257, 64, 512, 1), (70, 50, 3981, 1)]
    assert {k.rsplit('/', 1)[0] for k in fx} == {'%s/%s' % (R.case_name(c), k) for c, k in ALL}
    assert [R.kinds_of(c) for c in R.CASES] == [R.KINDS[:2]] * 2 + [R.KINDS] * 6          # signed: d >= 16 only
    for c, kind in ALL:
        p = '%s/%s/' % (R.case_name(c), kind)
        Nt, Nv, K, H = c
        assert tuple(int(v) for v in fx[p + 'params']) == c
        assert fx[p + 'T'].dtype == fx[p + 'V'].dtype == fx[p + 'out32'].dtype == np.float32 and fx[p + 'out64'].dtype == np.float64
        assert fx[p + 'T'].shape == (Nt, K) and fx[p + 'V'].shape == (Nv, K)
        assert fx[p + 'out32'].shape == fx[p + 'out64'].shape == (Nt, Nv)
        assert float(fx[p + 'e_ref']) == float(np.abs(fx[p + 'out32'] - fx[p + 'out64']).max()) <= 1e-6
        if kind != 'signed':
            assert fx[p + 'T'].min() >= 0 and fx[p + 'V'].min() >= 0
        else:
            assert fx[p + 'T'].min() < 0 and fx[p + 'V'].min() < 0
    for f in os.listdir(GOLDEN):
        if f.startswith('hist_sim'):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f


@pytest.mark.parametrize('c,kind', ALL, ids=['%s-%s' % (R.case_name(c), k) for c, k in ALL])
def test_restatement_reproduces_the_reference(fx, c, kind):
    p = '%s/%s/' % (R.case_name(c), kind)
    got = R.hist_sim(fx[p + 'T'], fx[p + 'V'], heads=c[3], eps=R.EPS)
    assert np.abs(got - fx[p + 'out64']).max() <= 1e-12
    assert np.abs(got - fx[p + 'out32']).max() <= float(fx[p + 'e_ref']) + 1e-12
    if c[3] > 1:                                                        # the 3-D form is the same computation
        again = R.hist_sim(fx[p + 'T'].reshape(c[0], c[3], -1), fx[p + 'V'].reshape(c[1], c[3], -1), eps=R.EPS)
        assert np.array_equal(again, got)


def test_entry_point_in_header_library_and_binding_at_the_header_abi():
    """(The entry point itself: test_cabi.py, ENTRY_POINTS.)"""
    assert 'sim_hist.hip' in __import__('laff_amd.build', fromlist=['SOURCES']).SOURCES


def test_c_entry_point_refuses_bad_arguments_without_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)                                             # never dereferenced: every call below ends in its checks

    def call(T=fake, ldt=8, V=fake, ldv=8, Nt=2, Nv=3, H=2, d=4, eps=1e-8, S=fake, lds=3):
        rc = lib.laff_sim_hist(None, T, ldt, V, ldv, Nt, Nv, H, d, eps, S, lds)
        return rc, lib.laff_last_error()

    def refused(code, what, **k):
        rc, msg = call(**k)
        return rc == code and msg.startswith(b'laff_sim_hist: ') and what in msg
    assert refused(-1, b'T is null', T=None) and refused(-1, b'V is null', V=None) and refused(-1, b'S is null', S=None)
    assert refused(-2, b'Nt=-1', Nt=-1) and refused(-2, b'Nv=-5', Nv=-5)
    assert refused(-2, b'H=0', H=0) and refused(-2, b'd=0', d=0) and refused(-2, b'd=-3', d=-3)
    assert refused(-2, b'H*d=4294967296', H=1 << 16, d=1 << 16, ldt=1 << 40, ldv=1 << 40)
    assert refused(-2, b'ldt=7', ldt=7) and refused(-2, b'ldv=7', ldv=7) and refused(-2, b'lds=2', lds=2)
    assert refused(-1, b'eps=-1', eps=-1.0) and refused(-1, b'eps=nan', eps=float('nan'))
    assert refused(-1, b'null ctx')                                     # valid arguments: only then the ctx
    assert refused(-1, b'null ctx', eps=0.0, ldt=1 << 33, lds=1 << 33)  # eps = 0 and 64-bit pitches are valid
    assert call(Nt=0, T=None, S=None)[0] == 0 and call(Nv=0, V=None, S=None, lds=0)[0] == 0    # an empty side: nothing to launch
    assert refused(-2, b'lds=2', Nt=0, lds=2)                           # ... but still checked


def test_python_surface_refuses_before_anything_reaches_a_device():
    from laff_amd import evaluation, loss, ops
    from laff_amd.config import make_config
    from laff_amd.model import get_model
    assert 'sim_hist' in ops.__all__
    a, b = torch.rand(3, 8), torch.rand(4, 8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.sim_hist(a, b)
    with pytest.raises(RuntimeError, match='no CPU path'):
        loss.hist_sim(a, b)
    with pytest.raises(RuntimeError, match='no CPU path'):
        loss.jaccard_sim(a, b)
    with pytest.raises((RuntimeError, AssertionError)):                 # numpy in, but no device to compute on
        evaluation.hist_sim(a.numpy(), b.numpy(), device='cuda' if not torch.cuda.is_available() else 'cpu')
    cfg = make_config({'a': 16}, {'bow': 8}, 64, 2, 'LAFF', [], [])
    m = get_model('LAFF', 'cpu', cfg).eval()
    te, ve = torch.rand(3, 2, 32), torch.rand(4, 2, 32)
    with pytest.raises(NotImplementedError):
        m.get_txt2vis_matrix(te, ve, 'euclidean')
    with pytest.raises(NotImplementedError):
        m.compute_sim(te[:, 0], ve[:, 0], 'euclidean')
    with pytest.raises(NotImplementedError):
        m.retrieve([], [], 'euclidean')
    with pytest.raises(RuntimeError, match='no CPU path') as e:         # 'hist' is a measure now: what stops it here is the device
        m.get_txt2vis_matrix(te, ve, 'hist')
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(RuntimeError, match='no CPU path') as e:
        m.compute_sim(te[:, 0], ve[:, 0], 'hist', device='cpu')
    assert not isinstance(e.value, NotImplementedError)
    with pytest.raises(ValueError):
        m.get_txt2vis_matrix(te, ve[:, 0], 'hist')                     # a 3-D side against a 2-D one


def test_width_and_dtype_mismatches_are_refused(monkeypatch):
    """ops.sim_hist's own checks, with the device test taken out of the way (they come before any library call)."""
    from laff_amd import ops
    monkeypatch.setattr(ops, '_dev', lambda t, name, dtype=torch.float32: t)
    monkeypatch.setattr(ops, '_context', lambda device: pytest.fail('a refused call reached the library'))
    a = torch.rand(3, 8)
    with pytest.raises(ValueError, match='differ in heads or width'):
        ops.sim_hist(a, torch.rand(4, 9))
    with pytest.raises(ValueError, match='differ in heads or width'):
        ops.sim_hist(a.view(3, 2, 4), torch.rand(4, 4, 2))
    with pytest.raises(ValueError, match='differ in heads or width'):
        ops.sim_hist(a.view(3, 2, 4), torch.rand(4, 8))
    with pytest.raises(ValueError, match='does not split into 3 heads'):
        ops.sim_hist(a, torch.rand(4, 8), heads=3)
    with pytest.raises(ValueError, match='contiguous rows'):
        ops.sim_hist(a.t(), torch.rand(4, 3))
    with pytest.raises(ValueError, match=r'out must be \(3, 4\)'):
        ops.sim_hist(a, torch.rand(4, 8), out=torch.empty(4, 3))
