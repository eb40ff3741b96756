"""Host checks of the differentiable GRU caption encoder, without a GPU: the hand-written float64 backpropagation through
time of tests/gru_bwd_ref.py against torch autograd through nn.GRU, the batch arrays the host prepares, the plan / reserve / workspace
queries and the argument refusals of the C entry points, and the explicit switch of GruTxtEncoder."""
import ctypes as C

import numpy as np
import pytest
import torch

import gru_bwd_ref as R
from laff_amd import txt2vec as T


def _problem(seed, N, H, bidirectional, pooling, V=50, we_dim=20, max_len=9):
    g = np.random.default_rng(seed)
    lens = g.integers(1, max_len + 1, N)
    lens[0] = 1
    lens[-1] = max_len
    ids = [g.integers(0, V, L) for L in lens]
    k = 1.0 / H ** 0.5
    sd = {'we.weight': g.normal(0, 1, (V, we_dim))}
    for sfx in ('_l0', '_l0_reverse') if bidirectional else ('_l0',):
        for name, shape in (('weight_ih', (3 * H, we_dim)), ('weight_hh', (3 * H, H)), ('bias_ih', (3 * H,)), ('bias_hh', (3 * H,))):
            sd['rnn.%s%s' % (name, sfx)] = g.uniform(-k, k, shape)
    width = H if pooling == 'last' else 2 * H if (pooling == 'mean_last' or bidirectional) else H
    return ids, sd, g.normal(0, 1, (N, width))


@pytest.mark.parametrize('net,pooling', [('gru', 'mean'), ('gru', 'last'), ('gru', 'mean_last'), ('bigru', 'mean'), ('bigru', 'last')])
def test_bptt_equals_float64_autograd(net, pooling):
    bi = net == 'bigru'
    ids, sd, dout = _problem(5, 7, 8, bi, pooling)
    out_a, want = R.autograd_grads(ids, sd, pooling, bi, dout)
    out_b, got = R.bptt(ids, sd, pooling, bi, dout)
    assert R.rel_err(out_b, out_a) <= 1e-14
    for k, w in want.items():
        if got[k] is None:                                         # bigru + last: the output is the forward half only
            assert bi and pooling == 'last' and k.endswith('_reverse') and not np.any(w)
        else:
            assert R.rel_err(got[k], w) <= 1e-13, k
    # rows of the embedding that no caption used have no gradient
    used = np.unique(np.concatenate(ids))
    assert not np.any(np.delete(got['we.weight'], used, axis=0))


def test_train_arrays_are_the_packed_layout():
    tokens = np.array([[5, 7, 5, 2], [7, 7, 9, 0], [3, 0, 0, 0]], np.int32)      # lengths 3, 2, 2, 1 (sorted rows), time-major
    pos, flat, seg_off, seg_tok, seg_pos = T.gru_train_arrays(tokens, [4, 3, 1])
    assert pos.tolist() == [[0, 1, 2, 3], [4, 5, 6, 0], [7, 0, 0, 0]]
    assert flat.tolist() == [5, 7, 5, 2, 7, 7, 9, 3]
    assert seg_tok.tolist() == [2, 3, 5, 7, 9] and seg_off.tolist() == [0, 1, 2, 4, 7, 8]
    assert seg_pos.tolist() == [3, 7, 0, 2, 1, 4, 5, 6]            # ascending positions inside a token: a fixed order of summation
    assert all(a.dtype == np.int32 for a in (pos, flat, seg_off, seg_tok, seg_pos))


def test_queries_and_refusals_need_no_gpu():
    from laff_amd import _lib, ops
    lib = _lib.load()
    n = C.c_size_t()
    # the reserve: five planes of [M, H] per direction; bigru + last runs the forward direction only
    assert ops.gru_train_reserve_bytes(100, 64) == 5 * 100 * 64 * 4
    assert ops.gru_train_reserve_bytes(100, 64, bidirectional=True) == 2 * 5 * 100 * 64 * 4
    assert ops.gru_train_reserve_bytes(100, 64, bidirectional=True, pooling='last') == 5 * 100 * 64 * 4
    assert lib.laff_gru_train_reserve_bytes(10, 48, 1, 0, 0, C.byref(n)) == -2
    assert lib.laff_gru_train_reserve_bytes(10, 64, 2, 0, 0, C.byref(n)) == -5 and b'num_layers=2' in lib.laff_last_error()
    assert lib.laff_gru_train_reserve_bytes(10, 64, 1, 1, 2, C.byref(n)) == -5 and b'mean_last' in lib.laff_last_error()
    assert lib.laff_gru_train_reserve_bytes(10, 64, 1, 0, 0, None) == -1
    # the plan: the tile of every launch, from the active rows of the two directions it serves
    assert ops.gru_backward_plan([3, 2, 1], 64) == ((0, 0, 0), (0, 0, 0))
    big = 512 * 64 - 63                                             # H = 32: one unit tile, so 512 row tiles of 64
    assert ops.gru_backward_plan([big, big - 1, 1], 32) == ((1, 0, 0), (0, 0, 1))
    assert ops.gru_backward_plan([big - 1, 1], 32) == ((0, 0), (0, 0))
    half = 256 * 64 - 63                                            # both directions share a launch: half the rows suffice ...
    assert ops.gru_backward_plan([half, 1], 32, bidirectional=True) == ((1, 1), (1, 1))
    assert ops.gru_backward_plan([half, 1], 32, bidirectional=True, pooling='last') == ((0, 0), (0, 0))     # ... unless only one runs
    bs = (C.c_int * 3)(3, 4, 1)
    out = (C.c_int * 3)()
    assert lib.laff_gru_backward_plan(bs, 3, 64, 0, 0, out, out) == -1 and b'non-increasing' in lib.laff_last_error()
    assert lib.laff_gru_backward_plan(None, 3, 64, 0, 0, out, out) == -1
    assert lib.laff_gru_backward_plan(bs, 3, 48, 0, 0, out, out) == -2
    # the workspace: carry, dGI, dGH, dX only for d_we, the partial tiles of the weight GEMMs; regions on 256 bytes
    N, H, D, M = 3, 64, 20, 6
    r256 = lambda b: (b + 255) // 256 * 256
    fc = max(ops.fc_backward_plan(M, H, 3 * H, want_dx=False)[1], ops.fc_backward_plan(M, D, 3 * H, want_dx=False)[1])
    base = r256(N * H * 4) + 2 * r256(M * 3 * H * 4)
    assert ops.gru_backward_workspace_bytes([3, 2, 1], N, H, D, want_dwe=False) == base + r256(fc)
    with_dx = ops.gru_backward_workspace_bytes([3, 2, 1], N, H, D)
    assert with_dx >= base + r256(M * D * 4) + r256(fc)
    assert ops.gru_backward_workspace_bytes([3, 2, 1], N, H, D, bidirectional=True) > 2 * base
    assert lib.laff_gru_backward_workspace_bytes(bs, 3, 3, 64, 20, 1, 0, 0, 1, C.byref(n)) == -1
    # argument errors of the launches come back before any GPU work, with their name
    fake = C.c_void_p(4096)
    ok = (C.c_int * 3)(3, 2, 1)
    gr = (C.c_void_p * 4)()

    def enc(M_=6, reserve=fake, rbytes=1 << 20, H_=64):
        return lib.laff_gru_encode_train(None, fake, fake, fake, ok, 3, 3, M_, H_, 1, 0, 0, fake, fake, fake, None, None, None, fake, 64,
                                         fake, 1 << 20, reserve, rbytes)
    assert enc() == -1 and b'laff_gru_encode_train: null ctx' in lib.laff_last_error()
    assert enc(M_=7) == -1 and b'batch_sizes sum to 6' in lib.laff_last_error()
    assert enc(rbytes=5 * 6 * 64 * 4 - 1) == -1 and b'reserve too small' in lib.laff_last_error()
    assert enc(reserve=C.c_void_p(4100)) == -3 and b'reserve' in lib.laff_last_error()
    assert enc(H_=48) == -2

    def bwd(M_=6, lddo=64, wbytes=1 << 20, ws=fake, X=fake, d_we=None, seg=None, U=0):
        return lib.laff_gru_backward(None, fake, fake, ok, 3, 3, M_, 64, 20, 1, 0, 0, fake, lddo, fake, 1 << 20, X, fake, fake, None, None,
                                     seg, seg, seg, U, 50, d_we, gr, None, ws, wbytes)
    assert bwd() == -1 and b'laff_gru_backward: null ctx' in lib.laff_last_error()
    assert bwd(M_=5) == -1 and b'batch_sizes sum to 6' in lib.laff_last_error()
    assert bwd(lddo=63) == -2 and b'lddo' in lib.laff_last_error()
    assert bwd(wbytes=base + r256(fc) - 1) == -1 and b'workspace too small' in lib.laff_last_error()
    assert bwd(ws=C.c_void_p(4100)) == -3
    assert bwd(d_we=fake) == -1 and b'token segments' in lib.laff_last_error()
    assert bwd(d_we=fake, seg=fake, U=7) == -1 and b'distinct tokens' in lib.laff_last_error()
    gr[0] = 4096
    assert bwd(X=None) == -1 and b'null X' in lib.laff_last_error()
    assert lib.laff_gru_pack_whh_t(None, fake, 48, fake) == -2
    assert lib.laff_gru_pack_whh_t(None, fake, 64, fake) == -1 and b'null ctx' in lib.laff_last_error()
    assert lib.laff_gru_gather_rows(None, fake, 0, 4, fake, 3, fake) == -2
    assert lib.laff_gru_gather_rows(None, fake, 5, 4, fake, 3, fake) == -1 and b'null ctx' in lib.laff_last_error()


def _vocab():
    v = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>', 'a', 'b']:
        v.add(w)
    return v


def test_switch_is_explicit_and_off_by_default(monkeypatch):
    """differentiable=False leaves forward on today's path whatever .training says: ops.gru_encode runs, the training entry does not."""
    from laff_amd import ops
    enc = T.GruTxtEncoder(T.IdxVec(_vocab()), 4, 32, device='cpu')
    assert enc.differentiable is False and enc.training
    calls = []
    monkeypatch.setattr(enc, '_tables', lambda: [('P', 'W', 'b')])
    monkeypatch.setattr(ops, 'gru_encode', lambda *a, **k: calls.append('gru_encode') or 'features')
    monkeypatch.setattr(ops, 'gru_encode_train', lambda *a, **k: calls.append('gru_encode_train'))
    monkeypatch.setattr(ops, 'gru_gather_rows', lambda *a, **k: calls.append('gru_gather_rows'))
    out = enc({'caption': ['a b', 'b']})
    assert out == {'text_features': 'features'} and calls == ['gru_encode']
    b = enc.to_device(enc.t2v_idx.batch(['a b', 'b']))
    assert type(b) is T.GruBatch
    # the switch alone changes the batch that to_device prepares ...
    on = T.GruTxtEncoder(T.IdxVec(_vocab()), 4, 32, device='cpu', differentiable=True)
    tb = on.to_device(on.t2v_idx.batch(['a b', 'b']))
    assert type(tb) is T.GruTrainBatch and tb.flat.tolist() == [1, 1, 4, 5, 5, 2, 2] and tb[:4][3] == [2, 2, 2, 1]
    # ... and eval mode or disabled gradients keep the inference path
    monkeypatch.setattr(on, '_tables', lambda: [('P', 'W', 'b')])
    del calls[:]
    on.eval()({'caption': ['a b']})
    with torch.no_grad():
        on.train()({'caption': ['a b']})
    assert calls == ['gru_encode', 'gru_encode']


def test_differentiable_refusals():
    on = T.GruTxtEncoder(T.IdxVec(_vocab()), 4, 32, device='cpu', differentiable=True).train()
    with pytest.raises(RuntimeError, match='no CPU path'):
        on({'caption': ['a b']})
    with pytest.raises(TypeError, match='fp32'):
        on.double()({'caption': ['a b']})
    with pytest.raises(TypeError, match='GruTrainBatch'):
        on.float().encode_batch(T.GruBatch(None, None, None, [1]))
    with pytest.raises(NotImplementedError, match='rnn_layer'):
        T.GruTxtEncoder(T.IdxVec(_vocab()), 4, 32, rnn_layer=2, device='cpu', differentiable=True)
