"""Host checks of the differentiable FC projection: the hand-written float64 formulas of tests/fc_bwd_ref.py against
torch autograd, what TransformNet refuses in training mode, and laff_fc_backward_plan, which needs no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fc_bwd_ref as R


@pytest.mark.parametrize('activation', R.ACTIVATIONS, ids=str)
def test_formulas_equal_float64_autograd(activation):
    g = torch.Generator().manual_seed(3)
    N, Dk, D = 7, 5, 9
    x = torch.randn(N, Dk, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(D, Dk, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    da = torch.randn(N, D, generator=g, dtype=torch.float64)
    a = R.forward_torch(x, w, b, activation)
    want = torch.autograd.grad(a, (x, w, b), da)
    got = R.backward(x, w, a, da, activation)
    for t, r in zip(got, want):
        np.testing.assert_allclose(t, r.numpy(), rtol=0, atol=1e-13 * float(r.abs().max()))
    # the bounds are those of the docstring: positive, and of the outputs' shapes
    for t, bd in zip(got, R.bounds(x, w, da)):
        assert bd.shape == t.shape and (bd > 0).all()


def _net(**kw):
    from laff_amd.model.model import TransformNet
    return TransformNet((8, 16), batch_norm=kw.pop('batch_norm', False), activation='tanh', dropout=0.0, **kw).train()


def test_training_mode_refusals_name_what_is_missing():
    x = torch.randn(4, 8)
    csr = torch.eye(4, 8).to_sparse_csr()
    for call in (lambda m, t, **k: m.plane(t, **k), lambda m, t, **k: m(t)):
        with pytest.raises(NotImplementedError, match='sparse'):
            call(_net(), csr)
        with pytest.raises(TypeError, match='fp32'):
            call(_net(), x.double())
        with pytest.raises(RuntimeError, match='no CPU path'):
            call(_net(), x)
    with pytest.raises(NotImplementedError, match='fc=False'):
        _net(fc=False, batch_norm=True).plane(torch.randn(4, 16))
    with pytest.raises(NotImplementedError, match='fc=False.*tiled over 2 heads'):
        _net(fc=False, batch_norm=True).plane(torch.randn(4, 8), heads=2)
    with pytest.raises(NotImplementedError, match='fc=False'):
        _net(fc=False, batch_norm=True)(torch.randn(4, 16))
    with pytest.raises(NotImplementedError, match='extra_shift'):
        _net().plane(x, extra_shift=torch.zeros(16))


def test_concat_problem_stays_inference_only():
    with pytest.raises(NotImplementedError, match='inference path only'):
        _net().concat_problem([torch.randn(4, 3), torch.randn(4, 5)])


def test_plan_needs_no_gpu():
    from laff_amd import _lib, ops
    lib = _lib.load()
    out = (ctypes.c_int * 4)()
    assert lib.laff_fc_backward_plan(128, 512, 4096, 0, 1, out) == 0
    assert out[0] == 1 and out[1] == 0                              # the training batch: no cut of the sum over N, no workspace
    assert lib.laff_fc_backward_plan(128, 4096, 4096, 0, 1, out) == 0 and out[0] == 1 and out[1] == 0
    # with dX its sum over D = 4096 is cut, and the partial tiles need room
    assert lib.laff_fc_backward_plan(128, 4096, 4096, 1, 1, out) == 0 and out[0] == 1 and out[2] > 1 and out[1] == out[2] * 128 * 4096 * 4
    chunks, nbytes, chunks_dx, _ = ops.fc_backward_plan(129, 100, 64)
    assert chunks == 2 and chunks_dx == 1 and nbytes == chunks * (64 * 100 + 64) * 4
    # the shape alone decides the cuts; the wanted outputs only how much of the workspace is needed (db's share always)
    assert ops.fc_backward_plan(129, 100, 64, want_dx=False, want_dw=False) == (chunks, chunks * 64 * 4, chunks_dx, 0)
    assert ops.fc_backward_plan(0, 3, 5)[:2] == (1, 0)
    assert lib.laff_fc_backward_plan(4, 0, 4, 1, 1, out) == -2 and b'laff_fc_backward_plan' in lib.laff_last_error()
    assert lib.laff_fc_backward_plan(4, 4, 4, 1, 1, None) == -1
    # argument errors of the launch itself come back before any GPU work
    assert lib.laff_fc_backward(None, None, 1, 1, 1, None, 1, 1, 0, None, 1, None, 1, None, 1, None, 1, None, None, 0) == -1
