"""Host checks of the differentiable bag-of-words projection: the float64 restatement of tests/fc_gather_bwd_ref.py
against torch autograd on the densified input, ops.csr_transpose on host tensors against a plain transposition, the ABI, and the
refusals of laff_fc_gather_backward, which need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

import fc_bwd_ref as R
import fc_gather_bwd_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pattern():
    """N = 5, Dk = 6: row 2 is empty, column 4 is empty, row 3 names word 1 twice, and ids -1, Dk and Dk + 5 are among the entries."""
    N, Dk = 5, 6
    rows = [[(0, 1.0), (3, 2.0), (-1, 7.0)], [(1, 1.0), (6, 5.0), (5, 3.0)], [], [(1, 1.0), (2, 4.0), (1, 0.5), (11, 9.0)],
            [(0, 2.0), (5, 1.0), (3, 1.0)]]
    crow = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    col = np.array([c for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float32)
    return N, Dk, crow, col, val


def _csr(N, Dk, crow, col, val):
    return torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=(N, Dk),
                                   check_invariants=False)


@pytest.mark.parametrize('activation', G.ACTIVATIONS, ids=str)
def test_restatement_equals_float64_autograd_on_the_densified_input(activation):
    N, Dk, crow, col, val = _pattern()
    D = 8
    g = torch.Generator().manual_seed(5)
    dense = torch.from_numpy(G.dense_from_csr(crow, col, val, N, Dk))
    assert dense[3, 1] == 1.5 and dense[2].abs().sum() == 0 and dense[:, 4].abs().sum() == 0 and float(dense.sum()) == 16.5
    w = torch.randn(D, Dk, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(D, generator=g, dtype=torch.float64, requires_grad=True)
    da = torch.randn(N, D, generator=g, dtype=torch.float64)
    a = R.forward_torch(dense, w, b, activation)
    want = torch.autograd.grad(a, (w, b), da)
    got = G.backward(dense.numpy(), a, da, activation)
    for t, r in zip(got, want):
        np.testing.assert_allclose(t, r.numpy(), rtol=0, atol=1e-13 * float(r.abs().max()))
    bw, bb = G.bounds(G.dense_from_csr(crow, col, val, N, Dk, magnitude=True), da)
    assert bw.shape == got[0].shape and bb.shape == got[1].shape and (bb > 0).all()
    assert (bw[:, [0, 1, 2, 3, 5]] > 0).all() and (bw[:, 4] == 0).all()             # an empty column admits only the exact zero
    # column by column from the transposed pattern: the same numbers
    from laff_amd import ops
    colptr, rows, values = ops.csr_transpose(_csr(N, Dk, crow, col, val))
    for v in range(Dk):
        cv, _ = G.column(colptr.numpy(), rows.numpy(), values.numpy(), v, a.detach().numpy(), da.numpy(), activation)
        np.testing.assert_allclose(cv, got[0][:, v], rtol=0, atol=1e-13 * float(np.abs(got[0]).max()))


def test_csr_transpose_on_the_host_equals_a_plain_transposition():
    from laff_amd import ops
    N, Dk, crow, col, val = _pattern()
    colptr, rows, values = ops.csr_transpose(_csr(N, Dk, crow, col, val))
    assert (colptr.dtype, rows.dtype, values.dtype) == (torch.int32, torch.int32, torch.float32)
    assert not colptr.is_cuda and tuple(colptr.shape) == (Dk + 1,) and rows.shape == values.shape
    colptr, rows, values = colptr.numpy(), rows.numpy(), values.numpy()
    plain = G.transpose_plain(crow, col, val, N, Dk)
    assert plain[4] == [] and plain[1] == [(1, 1.0), (3, 1.0), (3, 0.5)]           # the empty column; the repeated index, in CSR order
    for v in range(Dk):
        got = list(zip(rows[colptr[v]:colptr[v + 1]].tolist(), values[colptr[v]:colptr[v + 1]].tolist()))
        assert got == plain[v], v
    # ids -1, Dk and Dk + 5 are in no column's range: one entry in front of colptr[0], two behind colptr[Dk]
    assert colptr[0] == 1 and colptr[Dk] == len(col) - 2 and (np.diff(colptr) >= 0).all()
    assert 2 not in rows[colptr[0]:colptr[Dk]]                                       # the empty row
    np.testing.assert_array_equal(G.dense_from_csc(colptr, rows, values, N, Dk), G.dense_from_csr(crow, col, val, N, Dk))
    # an empty matrix
    colptr, rows, values = ops.csr_transpose(torch.zeros(0, 3).to_sparse_csr())
    assert colptr.tolist() == [0, 0, 0, 0] and rows.numel() == 0 and values.numel() == 0
    with pytest.raises(ValueError, match='sparse_csr'):
        ops.csr_transpose(torch.zeros(2, 3))


def test_header_binding_and_library_agree_on_the_abi_and_the_new_symbol():
    from laff_amd import ops
    header = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert re.search(r'\bint laff_fc_gather_backward\(laff_ctx\* ctx, const int\* colptr,', header)
    assert 'fc_gather_bwd.hip' in __import__('laff_amd.build', fromlist=['SOURCES']).SOURCES
    assert callable(ops.fc_gather_backward) and callable(ops.csr_transpose)
    assert 'fc_gather_backward' in ops.__all__ and 'csr_transpose' in ops.__all__


def test_refusals_need_no_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    call = lib.laff_fc_gather_backward
    #            ctx  colptr rows values nnz N  Dk D  act  A  lda dA ldda dW lddw db
    assert call(None, None, None, None, 1, 1, 1, 4, 0, None, 4, None, 4, None, 1, None) == -1          # a null ctx: before anything else
    assert call(None, None, None, None, 0, 0, 1, 4, 0, None, 4, None, 4, None, 1, None) == -1


def test_training_mode_messages():
    from laff_amd.model.model import TransformNet
    net = TransformNet((8, 16), batch_norm=False, activation='tanh', dropout=0.0).train()
    csr = torch.eye(4, 8).to_sparse_csr()
    with pytest.raises(NotImplementedError, match=r'sparse.*move it to the device'):
        net(csr)
    with pytest.raises(NotImplementedError, match='on the device'):
        net.concat_train([torch.randn(4, 3), torch.randn(4, 5)])
    with pytest.raises(RuntimeError, match='concat_problem'):
        net.eval().concat_train([torch.randn(4, 8)])
