"""Host checks of the device dropout + training-mode BatchNorm1d stage: the Philox mask of tests/dropout_bn_ref.py
against the generator's known-answer vectors and a scalar evaluation, the float64 formulas against float64 torch autograd, the plan, the
refusals of the two entry points (which need no GPU), the ABI, and the module's opt-in keyword."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropout_bn_ref as R

SEED = 0x0123456789abcdef


@pytest.mark.parametrize('counter, key, want', R.KNOWN_ANSWERS, ids=['zeros', 'ones', 'pi'])
def test_known_answer_vectors(counter, key, want):
    assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == want
    assert tuple(R.philox_scalar(counter, key)) == want


@pytest.mark.parametrize('p', [0.2, 0.5])
def test_mask_equals_the_scalar_evaluation(p):
    N, D = 5, 7
    mask = R.keep_mask(SEED, N, D, p)
    assert mask.shape == (N, D) and mask.dtype == bool
    for n in range(N):
        for c in range(D):
            assert bool(mask[n, c]) == R.keep_scalar(SEED, n, c, p), (n, c)
    # a negative int64 seed is the unsigned word with the same bits; p == 0 keeps everything; the threshold is floor(p 2^32)
    assert np.array_equal(R.keep_mask(-1, N, D, p), R.keep_mask(2 ** 64 - 1, N, D, p))
    assert R.keep_mask(SEED, N, D, 0.0).all() and not np.array_equal(mask, R.keep_mask(SEED + 1, N, D, p))
    assert R.threshold(0.5) == 2 ** 31 and R.threshold(0.2) == 858993459 and R.threshold(0.0) == 0
    assert R.scale32(0.2) == np.float32(1.25) and R.scale32(0.5) == np.float32(2.0)


@pytest.mark.parametrize('p', [0.0, 0.2])
def test_formulas_equal_float64_autograd(p):
    N, D, momentum, eps = 9, 6, 0.3, 1e-5
    g = torch.Generator().manual_seed(3)
    a = torch.randn(N, D, generator=g, dtype=torch.float64)
    dy = torch.randn(N, D, generator=g, dtype=torch.float64)
    gamma, beta = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(D, generator=g, dtype=torch.float64), torch.rand(D, generator=g, dtype=torch.float64) + 0.5
    keep = R.keep_mask(SEED, N, D, p)
    bn = torch.nn.BatchNorm1d(D, eps=eps, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    at = a.clone().requires_grad_(True)
    y = bn(at * torch.from_numpy(keep) / (1.0 - p))
    y.backward(dy)
    f = R.forward(a, keep, p, gamma, beta, rm, rv, momentum, eps)
    da, dgamma, dbeta = R.backward(dy, a, keep, p, gamma, f['mean'], f['invstd'])
    for name, got, want in (('y', f['y'], y), ('da', da, at.grad), ('dgamma', dgamma, bn.weight.grad), ('dbeta', dbeta, bn.bias.grad),
                            ('running_mean', f['running_mean'], bn.running_mean), ('running_var', f['running_var'], bn.running_var)):
        want = want.detach().numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * float(np.abs(want).max()), err_msg=name)
    # without a BatchNorm stage: y = a (.) m and da = dy (.) m
    f0 = R.forward(a, keep, p)
    assert np.array_equal(f0['y'], a.numpy() * keep / (1.0 - p))
    assert np.array_equal(R.backward(dy, a, keep, p)[0], dy.numpy() * (keep / (1.0 - p)))


def test_plan_names_the_shapes_that_are_cut():
    from laff_amd import ops
    chunks, nbytes, launches, rows = ops.dropout_bn_train_plan(128, 512)
    assert (chunks, nbytes, launches) == (1, 0, 1) and rows == 256                       # the training batch: one launch, no workspace
    assert ops.dropout_bn_train_plan(rows, 4096)[:3] == (1, 0, 1)
    assert ops.dropout_bn_train_plan(rows + 1, 260)[:3] == (2, 2 * 2 * 260 * 8, 2)        # the smallest N that is cut
    assert ops.dropout_bn_train_plan(8192, 512)[:3] == (32, 32 * 2 * 512 * 8, 2)
    assert ops.dropout_bn_train_plan(8192, 512, has_bn=False)[:3] == (1, 0, 1)            # nothing is summed: nothing is cut
    assert ops.dropout_bn_train_plan(0, 5, has_bn=False)[:3] == (1, 0, 1)


def test_refusals_need_no_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    E_ARG, E_SHAPE = -1, -2
    seed = C.c_ulonglong(7)
    vec = (C.c_float * 8)()
    g = C.cast(vec, C.c_void_p)

    def fwd(N=4, D=8, p=0.2, seed=C.cast(C.pointer(seed), C.c_void_p), gamma=g, momentum=0.1, eps=1e-5):
        rc = lib.laff_dropout_bn_train(None, None, N, D, D, p, seed, gamma, g, g, g, momentum, eps, None, D, g, g, None, 0)
        return rc, lib.laff_last_error().decode()

    def bwd(N=4, D=8, p=0.2, seed=C.cast(C.pointer(seed), C.c_void_p), gamma=g):
        rc = lib.laff_dropout_bn_train_backward(None, None, D, None, N, D, D, p, seed, gamma, g, g, None, D, None, None, None, 0)
        return rc, lib.laff_last_error().decode()

    for call in (fwd, bwd):
        for kw, code, text in (
                (dict(N=1), E_ARG, 'N >= 2'), (dict(N=0), E_ARG, 'N >= 2'),                # one value per channel, as torch refuses it
                (dict(p=-0.1), E_ARG, 'outside [0, 1)'), (dict(p=1.0), E_ARG, 'outside [0, 1)'), (dict(p=float('nan')), E_ARG, 'outside'),
                (dict(seed=None), E_ARG, 'needs a seed'),
                (dict(p=0.0, gamma=None), E_ARG, 'nothing to do'),
                (dict(D=0), E_SHAPE, 'D>=1'), (dict(N=-1), E_SHAPE, 'N>=0')):
            rc, msg = call(**kw)
            assert rc == code and text in msg, (call.__name__, kw, rc, msg)
        # everything in order: the null ctx is what is left to refuse; p == 0 needs no seed; one row is fine without statistics
        for kw in (dict(), dict(p=0.0, seed=None), dict(N=1, gamma=None), dict(N=0, gamma=None)):
            rc, msg = call(**kw)
            assert rc == E_ARG and 'null ctx' in msg, (call.__name__, kw, rc, msg)
    for kw, text in ((dict(eps=0.0), 'eps'), (dict(eps=-1e-5), 'eps'), (dict(momentum=-0.1), 'momentum'), (dict(momentum=1.5), 'momentum')):
        rc, msg = fwd(**kw)
        assert rc == E_ARG and text in msg, (kw, rc, msg)
    assert 'null ctx' in fwd(momentum=0.0)[1] and 'null ctx' in fwd(momentum=1.0)[1]
    out = (C.c_int * 4)()
    assert lib.laff_dropout_bn_train_plan(4, 0, 1, out) == E_SHAPE and lib.laff_dropout_bn_train_plan(4, 8, 1, None) == E_ARG


def test_ops_refuse_host_and_non_fp32_tensors():
    from laff_amd import ops
    a, v = torch.randn(4, 8), torch.ones(8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.dropout_bn_train(a, 0.0, None, v, v, v, v, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.dropout_bn_train_backward(a, a, 0.0, None, v, v, v)


def test_header_binding_and_library_agree_on_the_abi_and_the_new_symbols():
    """(The entry points themselves: test_cabi.py, ENTRY_POINTS.)"""
    from laff_amd import ops
    assert 'bn_train.hip' in __import__('laff_amd.build', fromlist=['SOURCES']).SOURCES
    for name in ('dropout_bn_train', 'dropout_bn_train_backward', 'dropout_bn_train_plan'):
        assert callable(getattr(ops, name)) and name in ops.__all__


def test_device_norm_is_opt_in_and_refuses_what_it_does_not_compute():
    from laff_amd.model import model
    net = model.TransformNet((8, 16), batch_norm=True, activation='tanh', dropout=0.2)
    assert net.device_norm is False
    assert model.TransformNet((8, 16), batch_norm=True, activation='tanh', dropout=0.2, device_norm=True).device_norm is True
    tower = torch.nn.ModuleList([net, torch.nn.Sequential(model.TransformNet((8, 16), batch_norm=False, activation='tanh'))])
    assert model.use_device_norm(tower) is tower and net.device_norm and tower[1][0].device_norm
    model.use_device_norm(tower, False)
    assert not net.device_norm and not tower[1][0].device_norm
    x = torch.randn(4, 8)
    for field, value, text in (('momentum', None, 'momentum=None'), ('affine', False, 'affine=False'),
                               ('track_running_stats', False, 'track_running_stats=False')):
        bad = model.TransformNet((8, 16), batch_norm=True, activation='tanh', dropout=0.2, device_norm=True).train()
        setattr(bad.bn1, field, value)
        with pytest.raises(NotImplementedError, match=text):
            bad(x)
        with pytest.raises(NotImplementedError, match=text):
            bad.plane(x)
        bad.device_norm = False
        with pytest.raises(RuntimeError, match='no CPU path'):                            # the default route: today's message
            bad(x)
