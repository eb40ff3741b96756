"""laff_fc_gather_backward, ops.fc_gather_backward / csr_transpose, and the training-mode TransformNet on a sparse (CSR) input and on a
concat layer, on the MI355X.

Kernel level.  The saved forward output A is an input of the call, so the reference is the float64 evaluation of the formulas of
tests/fc_gather_bwd_ref.py on the very fp32 A, dA and values handed to the device.  The bound is derived, not measured, and holds element
by element (u = 2^-24, magnitudes in float64, |X| the densified pattern with the magnitudes of repeated entries added):

    |dW - ref| <= (N + 4) u |dA|^T |X|        |db - ref| <= (N + 4) u sum_n |dA|

A column's fmaf chain has as many terms as the column has entries (at most N in every case here); any order of a K-term fp32 sum stays
within gamma_K sum |a b|, and forming dz from a costs at most three roundings against |act'| <= 1.  A column without entries has a zero
bound: only the exact +0.0 passes.

Module level and end to end: the rule of tests/test_gpu_fc_backward.py, max |device - float64| / max |float64| within the larger of
4 x the same error of the float32 CPU graph and train_ref.TOL_UNIT (end to end: train_ref.end_to_end_bound).

The table at the end of the file records the largest fraction of its bound that each tensor used.
"""
import functools

import numpy as np
import pytest
import torch

import fc_bwd_ref as R
import fc_gather_bwd_ref as G
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
TV = 64                               # the vocabulary columns of one tile of the kernel

# (N, Dk, D, activation, values present, layout of dW, pattern).  Layouts: 'dense' rows on a 16-byte aligned base; 'pitch4' a wider
# pitch that keeps the rows 16-byte aligned; 'pitch3' a pitch that breaks it; 'window' a column window at an odd offset of a wider
# buffer.  The 16-byte store variant runs where the layout is 'dense' or 'pitch4' and Dk % 4 == 0, the single-float one elsewhere.
CASES = [
    (1, 1, 4, None, True, 'dense', 'plain'),
    (3, 5, 8, 'tanh', False, 'pitch4', 'holes'),              # an empty row and two empty columns
    (5, 8, 12, 'relu', True, 'pitch4', 'plain'),              # the 16-byte stores through a pitch
    (33, 70, 132, 'relu', True, 'pitch3', 'repeats'),         # repeated indices, ids outside the vocabulary; ragged tiles both ways
    (129, 65, 260, 'sigmoid', False, 'window', 'full'),       # one column hit by all 129 rows
    (17, 129, 8192, None, True, 'dense', 'plain'),
    (64, 1000, 512, 'tanh', False, 'dense', 'zipf'),          # most tiles empty; the 16-byte stores
    (130, 7811, 4096, 'sigmoid', True, 'dense', 'big'),       # sampled
]


def _id(c):
    return 'N%d-Dk%d-D%d-%s-%s-%s-%s' % (c[0], c[1], c[2], c[3], 'values' if c[4] else 'ones', c[5], c[6])


def _rows_of(c, rng):
    """The CSR rows of a case: per row the list of column ids, in the order the CSR holds them."""
    N, Dk, kind = c[0], c[1], c[6]
    if kind == 'holes':
        return [[0, 2], [], [2, 4]]
    per_row = min(Dk, 10)
    if kind == 'zipf':
        return [sorted(set(np.minimum(rng.zipf(2.5, per_row) - 1, Dk - 1).tolist())) for _ in range(N)]
    rows = [sorted(rng.choice(Dk, size=rng.integers(1, per_row + 1), replace=False).tolist()) for _ in range(N)]
    if kind == 'big':
        rows = [sorted(set(r + np.minimum(rng.zipf(1.6, 4) - 1, Dk - 1).tolist())) for r in rows]
    if kind == 'full':
        rows = [sorted(set(r + [7])) for r in rows]
    if kind == 'repeats':
        rows[4] = []
        for n in range(0, N, 3):
            rows[n] = rows[n] + [rows[n][0], 69]               # a word named twice, and the last column
        rows[1] = [-1] + rows[1] + [Dk, Dk + 5]
        rows[7] = rows[7] + [Dk + 5, -1]
    return rows


@functools.lru_cache(maxsize=None)
def _case(c):
    """The pattern, the fp32 operands on the CPU, the float64 reference and the bounds -- computed once, shared, never written."""
    from laff_amd import ops
    N, Dk, D, act, with_values, layout, kind = c
    rng = np.random.default_rng(N * 1000003 + Dk * 1009 + D)
    rows = _rows_of(c, rng)
    crow = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    col = np.array([v for r in rows for v in r], np.int32)
    val = rng.uniform(0.5, 3.0, col.shape[0]).astype(np.float32) if with_values else np.ones(col.shape[0], np.float32)
    csr = torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), size=(N, Dk), check_invariants=False)
    colptr, rws, values = ops.csr_transpose(csr)
    assert int(np.diff(colptr.numpy()).max()) <= N                         # the factor N + 4 covers the longest column
    g = torch.Generator().manual_seed(N * 1000003 + Dk * 1009 + D)
    z = 3.0 * torch.randn(N, D, generator=g)                               # logits x 3: part of A sits in saturation
    a = {None: lambda t: t, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}[act](z)
    da = torch.randn(N, D, generator=g)
    if act == 'relu':
        assert (a == 0).any() and (a > 0).any()
    if act == 'tanh' and N * D >= 1000:
        assert (a.abs() > 0.999).any()
    touched = np.unique(col[(col >= 0) & (col < Dk)])
    out = dict(c=c, csr=csr, csc=(colptr, rws, values if with_values else None), a=a, da=da, touched=touched)
    if kind == 'big':
        # every touched column, and 4,096 elements drawn over the whole matrix (nearly all of them in untouched columns: exact zeros)
        cols = {int(v): G.column(colptr.numpy(), rws.numpy(), values.numpy(), int(v), a.numpy(), da.numpy(), act) for v in touched}
        out.update(cols=cols, sample=(rng.integers(0, D, 4096), rng.integers(0, Dk, 4096)),
                   db=(G.backward(np.zeros((N, 0)), a, da, act)[1], G.bounds(np.zeros((N, 0)), da)[1]))
    else:
        x, mag = G.dense_from_csr(crow, col, val, N, Dk), G.dense_from_csr(crow, col, val, N, Dk, magnitude=True)
        out.update(ref=G.backward(x, a, da, act), bounds=G.bounds(mag, da))
    if kind == 'zipf':
        ptr = colptr.numpy()
        empty = sum(1 for v0 in range(0, Dk, TV) if ptr[min(v0 + TV, Dk)] == ptr[v0])
        assert empty > (Dk + TV - 1) // TV // 2, empty
    return out


@functools.lru_cache(maxsize=None)
def _device_inputs(c):
    cs = _case(c)
    return tuple(None if t is None else t.to(DEV) for t in cs['csc']), cs['a'].to(DEV), cs['da'].to(DEV)


def _launch(c, want=(True, True), layout=None, csc=None):
    """ops.fc_gather_backward into NaN-framed buffers: (dw, db) (None where not wanted) after the frame check."""
    from laff_amd import ops
    N, Dk, D, act = c[:4]
    dcsc, a, da = _device_inputs(c)
    bufs = [TR.pitched(D, Dk, layout or c[5]) if want[0] else None, TR.out_vec(D) if want[1] else None]
    res = ops.fc_gather_backward(csc or dcsc, N, Dk, a, da, act, *want, out=tuple(None if b is None else b[1] for b in bufs))
    torch.cuda.synchronize()
    for name, b, r in zip(('dw', 'db'), bufs, res):
        if b is None:
            assert r is None
            continue
        assert r.data_ptr() == b[1].data_ptr()
        assert TR.untouched_around(*b), '%s: a write outside the output' % name
        assert not r.isnan().any(), '%s: an element was not written' % name
    return res


def _frac(err, bound):
    # a zero bound (a column without entries, a zero row of |dA|) admits only the exact zero
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))


def _check(c, res, label=''):
    cs = _case(c)
    N, Dk, D = c[:3]
    dw, db = res
    if dw is not None:
        # columns without an entry: +0.0, value and sign bit
        untouched = torch.ones(Dk, dtype=torch.bool)
        untouched[torch.from_numpy(cs['touched'].astype(np.int64))] = False
        z = dw[:, untouched.to(DEV)]
        assert not z.any() and not torch.signbit(z).any(), 'a column without entries is not +0.0'
    if c[6] == 'big':
        fr = 0.0
        if dw is not None:
            for v, (ref, bound) in cs['cols'].items():
                fr = max(fr, _frac(np.abs(dw[:, v].cpu().numpy().astype(np.float64) - ref), bound))
            ds, vs = cs['sample']
            got = dw[torch.from_numpy(ds).to(DEV), torch.from_numpy(vs).to(DEV)].cpu().numpy().astype(np.float64)
            for k in range(len(ds)):
                ref, bound = (cs['cols'][int(vs[k])][0][ds[k]], cs['cols'][int(vs[k])][1][ds[k]]) if int(vs[k]) in cs['cols'] else (0.0, 0.0)
                fr = max(fr, _frac(np.abs(got[k:k + 1] - ref), np.asarray([bound])))
        fracs = {'dw': fr if dw is not None else None,
                 'db': None if db is None else _frac(np.abs(db.cpu().numpy().astype(np.float64) - cs['db'][0]), cs['db'][1])}
    else:
        fracs = {}
        for name, got, ref, bound in zip(('dw', 'db'), res, cs['ref'], cs['bounds']):
            if got is None:
                fracs[name] = None
                continue
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            assert err.shape == bound.shape
            fracs[name] = _frac(err, bound)
    for name, f in fracs.items():
        if f is not None:
            print('%s %s%s: largest err / bound %.4f' % (_id(c), name, label, f))
            assert f <= 1.0, (name, f)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_backward_vs_float64(c):
    _check(c, _launch(c))


@pytest.mark.parametrize('c', [CASES[3], CASES[6]], ids=_id)
def test_output_layouts_and_store_variants_give_the_same_bits(c):
    """Every layout of dW against float64, inside its NaN frame; and the bits of the dense one in all of them: Dk = 1000 takes the
    16-byte stores in 'dense' and 'pitch4' and the single-float ones in 'pitch3' and 'window', Dk = 70 the single-float ones throughout."""
    dense = _launch(c, layout='dense')
    _check(c, dense, ' (dense)')
    for layout in ('pitch4', 'pitch3', 'window'):
        res = _launch(c, layout=layout)
        _check(c, res, ' (%s)' % layout)
        assert torch.equal(res[0], dense[0]) and torch.equal(res[1], dense[1]), layout


@pytest.mark.parametrize('c', [CASES[1], CASES[3], CASES[4], CASES[6]], ids=_id)
def test_each_output_alone_and_repeats_are_bit_identical(c):
    full = [t.clone() for t in _launch(c)]
    again = _launch(c)
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])
    dw, none = _launch(c, (True, False))
    assert none is None and torch.equal(dw, full[0])
    none, db = _launch(c, (False, True))
    assert none is None and torch.equal(db, full[1])
    from laff_amd import ops
    dcsc, a, da = _device_inputs(c)
    assert ops.fc_gather_backward(dcsc, c[0], c[1], a, da, c[3], False, False) == (None, None)


def test_empty_batch_and_empty_pattern_write_zeros_and_nothing_else():
    from laff_amd import ops
    Dk, D = 70, 132
    none = (torch.zeros(Dk + 1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None)
    for layout in ('dense', 'pitch3', 'window'):
        # N == 0
        bdw, bdb = TR.pitched(D, Dk, layout), TR.out_vec(D)
        dw, db = ops.fc_gather_backward(none, 0, Dk, torch.empty(0, D, device=DEV), torch.empty(0, D, device=DEV), 'tanh', out=(bdw[1], bdb[1]))
        torch.cuda.synchronize()
        assert not dw.any() and not db.any() and not torch.signbit(dw).any() and TR.untouched_around(*bdw) and TR.untouched_around(*bdb)
        # nnz == 0 with rows: dW is zero, db is the column sum of dZ
        a, da = torch.tanh(torch.randn(5, D, device=DEV)), torch.randn(5, D, device=DEV)
        bdw, bdb = TR.pitched(D, Dk, layout), TR.out_vec(D)
        dw, db = ops.fc_gather_backward(none, 5, Dk, a, da, 'tanh', out=(bdw[1], bdb[1]))
        torch.cuda.synchronize()
        assert not dw.any() and not torch.signbit(dw).any() and TR.untouched_around(*bdw) and TR.untouched_around(*bdb)
        ref = (da.double() * (1.0 - a.double() ** 2)).sum(0)
        assert ((db.double() - ref).abs() <= 9 * G.U * da.double().abs().sum(0)).all()


def test_device_built_csc_equals_the_host_built_one():
    from laff_amd import ops
    for c in (CASES[3], CASES[6]):
        cs = _case(c)
        host = ops.csr_transpose(cs['csr'])
        dev = ops.csr_transpose(cs['csr'].to(DEV))
        for h, d in zip(host, dev):
            assert d.is_cuda and d.dtype == h.dtype and torch.equal(d.cpu(), h)
        if c[4]:
            mine, theirs = _launch(c, csc=dev), _launch(c)
            assert torch.equal(mine[0], theirs[0]) and torch.equal(mine[1], theirs[1])


def test_graph_capture_replays_the_eager_bits():
    from laff_amd import ops
    c = CASES[3]
    N, Dk, D, act = c[:4]
    dcsc, a, da = _device_inputs(c)
    eager = [t.clone() for t in ops.fc_gather_backward(dcsc, N, Dk, a, da, act)]
    outs = (torch.full((D, Dk), NAN, device=DEV), torch.full((D,), NAN, device=DEV))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        ops.fc_gather_backward(dcsc, N, Dk, a, da, act, out=outs)
    gr.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(outs, eager))
    _check(c, outs, ' (graph)')


def test_argument_errors_and_rows_that_are_copied():
    from laff_amd import ops
    c = CASES[3]
    N, Dk, D, act = c[:4]
    dcsc, a, da = _device_inputs(c)
    with pytest.raises(ValueError, match='activation'):
        ops.fc_gather_backward(dcsc, N, Dk, a, da, 'gelu')
    with pytest.raises(ValueError, match='do not fit'):
        ops.fc_gather_backward(dcsc, N, Dk, a, da[:, :128], act)
    with pytest.raises(ValueError, match='colptr'):
        ops.fc_gather_backward(dcsc, N, Dk + 1, a, da, act)
    with pytest.raises(TypeError):
        ops.fc_gather_backward(dcsc, N, Dk, a.double(), da, act)
    with pytest.raises(TypeError):
        ops.fc_gather_backward((dcsc[0].long(), dcsc[1], dcsc[2]), N, Dk, a, da, act)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fc_gather_backward(dcsc, N, Dk, a.cpu(), da, act)
    # the C entry point: shape, pitch, alignment and activation come back as LAFF_E_* before any GPU work
    lib, h = ops._context(a.device)
    p = ops._ptr
    dw = torch.empty(D, Dk, device=DEV)
    args = lambda **k: [k.get(n, d) for n, d in (('h', h), ('colptr', p(dcsc[0])), ('rows', p(dcsc[1])), ('values', p(dcsc[2])),   # noqa: E731
                                                   ('nnz', dcsc[1].numel()), ('N', N), ('Dk', Dk), ('D', D), ('act', 2), ('A', p(a)), ('lda', D),
                                                   ('dA', p(da)), ('ldda', D), ('dW', p(dw)), ('lddw', Dk), ('db', None))]
    call = lib.laff_fc_gather_backward
    assert call(*args(D=130)) == -2 and call(*args(D=8196)) == -2 and call(*args(D=0)) == -2 and call(*args(Dk=0)) == -2
    assert call(*args(lddw=Dk - 1)) == -2 and call(*args(lda=D - 4)) == -2 and call(*args(ldda=D + 2)) == -2
    assert call(*args(act=7)) == -1 and call(*args(colptr=None)) == -1 and call(*args(A=None)) == -1
    assert call(*args(A=a.data_ptr() + 4)) == -3 and call(*args(dW=dw.data_ptr() + 2)) == -3
    assert b'laff_fc_gather_backward' in lib.laff_last_error()
    # rows that are dense but not 16-byte aligned (a column window, a non-unit stride) are copied by the op, not refused
    wide, wide_g = torch.zeros(N, D + 4, device=DEV), torch.zeros(N, 2 * D, device=DEV)
    wide[:, 1:D + 1] = a
    wide_g[:, ::2] = da
    got = ops.fc_gather_backward(dcsc, N, Dk, wide[:, 1:D + 1], wide_g[:, ::2], act)
    want = ops.fc_gather_backward(dcsc, N, Dk, a, da, act)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # 16-byte aligned rows with a pitch are read in place: the same bits
    pitched = torch.zeros(N, D + 8, device=DEV)
    pitched[:, :D] = a
    got = ops.fc_gather_backward(dcsc, N, Dk, pitched[:, :D], da, act)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- TransformNet in training mode on a sparse input ----------------------------------------------------------------------------------
def _bow(N, Dk, seed, per_row=6):
    """A bag-of-words count matrix: (the CSR with int32 indices on the CPU, the same matrix dense)."""
    rng = np.random.default_rng(seed)
    dense = torch.zeros(N, Dk)
    for n in range(N):
        for v in rng.choice(Dk, size=rng.integers(1, per_row + 1), replace=False):
            dense[n, v] = float(rng.integers(1, 4))
    sp = dense.to_sparse_csr()
    return torch.sparse_csr_tensor(sp.crow_indices().to(torch.int32), sp.col_indices().to(torch.int32), sp.values(), size=(N, Dk)), dense


@pytest.mark.parametrize('batch_norm, activation, dropout', [(True, 'tanh', 0.0), (True, 'relu', 0.0), (False, 'sigmoid', 0.0),
                                                             (False, None, 0.0), (False, 'tanh', 0.2)],
                         ids=lambda v: str(v))
def test_transform_net_train_on_a_csr_input(batch_norm, activation, dropout):
    from laff_amd.model.model import TransformNet
    torch.manual_seed(11)
    N = 33
    net = TransformNet((70, 132), batch_norm=batch_norm, activation=activation, dropout=dropout)
    with torch.no_grad():
        net.fc1.bias.normal_(0.0, 0.1)
    W, b = net.fc1.weight.detach().clone(), net.fc1.bias.detach().clone()
    csr, x = _bow(N, 70, 5)
    dE = torch.randn(N, 132)
    net = net.to(DEV).train()
    y = net(csr.to(DEV))
    assert y.requires_grad and tuple(y.shape) == (N, 132)
    y.backward(dE.to(DEV))
    mask = None
    if dropout:
        a64 = R.forward_torch(x.double(), W.double(), b.double(), activation)
        assert (a64 != 0).all() and (R.forward_torch(x, W, b, activation) != 0).all()
        mask = (y.detach() != 0).cpu()
        kept = float(mask.double().mean())
        assert abs(kept - (1.0 - dropout)) <= 5.0 * ((1.0 - dropout) * dropout / mask.numel()) ** 0.5, kept
    ref = TR.layer_graph(torch.float64, W, b, x, dE, activation, batch_norm, mask, dropout)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, activation, batch_norm, mask, dropout)
    got = {'y': y, 'fc1.weight.grad': net.fc1.weight.grad, 'fc1.bias.grad': net.fc1.bias.grad}
    if batch_norm:
        got.update({'bn1.weight.grad': net.bn1.weight.grad, 'bn1.bias.grad': net.bn1.bias.grad, 'running_mean': net.bn1.running_mean,
                    'running_var': net.bn1.running_var})
    TR.compare(got, ref, f32, 'csr')
    gw = net.fc1.weight.grad
    assert gw.is_contiguous() and gw.shape == net.fc1.weight.shape and gw.stride() == net.fc1.weight.stride()
    # plane(): plain and dense, accepted by the training-mode fusion blocks as it is
    pending = []
    src, tile, scale, shift = net.plane(csr.to(DEV), heads=2, pending=pending)
    assert pending == [] and tile is False and scale is None and shift is None and src.requires_grad
    assert dropout or torch.equal(src, y)
    # eval afterwards: today's code path, bit for bit the gather kernel's output with the folded BatchNorm
    from laff_amd import ops
    net.eval()
    with torch.no_grad():
        ye = net(csr.to(DEV))
        scale, shift = net.bn_affine(None)
        want = ops.fc_gather_act_bn(csr.to(DEV), net.weight_t(), net.fc1.bias.detach(), scale, shift, activation)
    assert not ye.requires_grad and torch.equal(ye, want)


def test_adam_steps_the_gather_gradient_as_torch_does_and_the_attached_csc_is_used(monkeypatch):
    from laff_amd import ops, optim, txt2vec
    from laff_amd.model.model import TransformNet
    torch.manual_seed(13)
    words = ['w%d' % i for i in range(70)]
    rng = np.random.default_rng(3)
    captions = [' '.join(rng.choice(words, size=rng.integers(1, 8)).tolist()) for _ in range(33)]
    enc = txt2vec.BoWTxtEncoder(txt2vec.BowVec(words, clean=False), DEV, with_csc=True)
    x = enc({'caption': captions})['text_features']
    plain = txt2vec.BoWTxtEncoder(txt2vec.BowVec(words, clean=False), DEV)({'caption': captions})['text_features']
    assert x.is_cuda and not hasattr(plain, 'laff_csc') and torch.equal(x.to_dense(), plain.to_dense())
    for mine, theirs in zip(x.laff_csc, ops.csr_transpose(plain)):
        assert mine.is_cuda and torch.equal(mine, theirs)
    net = TransformNet((70, 132), batch_norm=False, activation='tanh', dropout=0.0).to(DEV).train()
    dE = torch.randn(33, 132, device=DEV)
    net(plain).backward(dE)                                                  # transposed on the device
    gw, gb = net.fc1.weight.grad.clone(), net.fc1.bias.grad.clone()
    net.zero_grad()
    calls = []
    real = ops.csr_transpose
    monkeypatch.setattr(ops, 'csr_transpose', lambda t: calls.append(1) or real(t))
    net(x).backward(dE)                                                      # the attached arrays: no transposition
    assert calls == [] and torch.equal(net.fc1.weight.grad, gw) and torch.equal(net.fc1.bias.grad, gb)
    # one optimizer step on this gradient, as it is
    lr = 1e-2
    twin = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    for q, p in zip(twin, net.parameters()):
        q.grad = p.grad.clone()
    before = net.fc1.weight.detach().clone()
    optim.Adam(net.parameters(), lr=lr).step()
    torch.optim.Adam(twin, lr=lr).step()
    torch.cuda.synchronize()
    assert not torch.equal(net.fc1.weight, before)
    for p, q in zip(net.parameters(), twin):
        # either side rounds the update (at most lr) a handful of times and the parameter once: 16 u (lr + |p|) between the two
        assert ((p - q).abs() <= 16 * G.U * (lr + q.abs())).all()


# ---- the concat layer in training mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kinds', [('dense', 'csr', 'dense'), ('csr', 'csr'), ('dense', 'dense', 'dense')], ids='-'.join)
@pytest.mark.parametrize('batch_norm, activation', [(True, 'tanh'), (False, 'relu')], ids=str)
def test_concat_train(kinds, batch_norm, activation, monkeypatch):
    from laff_amd import ops
    from laff_amd.model.model import TransformNet
    torch.manual_seed(17)
    N, K, D = 33, 116, 64
    widths = {3: (36, 50, 30), 2: (66, 50)}[len(kinds)]
    net = TransformNet((K, D), batch_norm=batch_norm, activation=activation, dropout=0.0)
    with torch.no_grad():
        net.fc1.bias.normal_(0.0, 0.1)
    W, b = net.fc1.weight.detach().clone(), net.fc1.bias.detach().clone()
    dense, segs = [], []
    for j, (kind, w) in enumerate(zip(kinds, widths)):
        if kind == 'csr':
            csr, x = _bow(N, w, 20 + j)
            segs.append(csr.to(DEV))
        else:
            x = torch.randn(N, w)
            segs.append(x.to(DEV).requires_grad_(j == len(kinds) - 1))       # the last dense segment requires a gradient
        dense.append(x)
    x = torch.cat(dense, 1)
    dE = torch.randn(N, D)
    net = net.to(DEV).train()
    calls, gcalls = [], []
    real, greal = ops.fc_backward, ops.fc_gather_backward
    monkeypatch.setattr(ops, 'fc_backward', lambda *a, **k: calls.append(dict(k)) or real(*a, **k))
    monkeypatch.setattr(ops, 'fc_gather_backward', lambda *a, **k: gcalls.append(dict(k)) or greal(*a, **k))
    y = net.concat_train(segs)
    assert y.requires_grad and tuple(y.shape) == (N, D)
    y.backward(dE.to(DEV))
    ref = TR.layer_graph(torch.float64, W, b, x, dE, activation, batch_norm, None, 0.0)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, activation, batch_norm, None, 0.0)
    got = {'y': y, 'fc1.weight.grad': net.fc1.weight.grad, 'fc1.bias.grad': net.fc1.bias.grad}
    if batch_norm:
        got.update({'bn1.weight.grad': net.bn1.weight.grad, 'bn1.bias.grad': net.bn1.bias.grad, 'running_mean': net.bn1.running_mean,
                    'running_var': net.bn1.running_var})
    col = 0
    for kind, w, s in zip(kinds, widths, segs):
        if kind == 'dense' and s.requires_grad:
            key = 'x.grad[%d:%d]' % (col, col + w)
            got[key], ref[key], f32[key] = s.grad, ref['x.grad'][:, col:col + w], f32['x.grad'][:, col:col + w]
        else:
            assert s.grad is None                                             # no gradient where none is required
        col += w
    TR.compare(got, ref, f32, '-'.join(kinds))
    assert net.fc1.weight.grad.is_contiguous() and net.fc1.weight.grad.shape == (D, K)
    # one call per segment; dx only for the segment that requires it; db formed exactly once, by the first segment's call
    assert len(calls) == kinds.count('dense') and len(gcalls) == kinds.count('csr')
    assert [k['want_dx'] for k in calls] == [s.requires_grad for kind, s in zip(kinds, segs) if kind == 'dense']
    assert sum(bool(k['want_db']) for k in calls + gcalls) == 1 and (calls if kinds[0] == 'dense' else gcalls)[0]['want_db']
    assert all(k['want_dw'] for k in calls + gcalls)


def test_concat_train_refusals():
    from laff_amd.model.model import TransformNet
    net = TransformNet((116, 64), batch_norm=False, activation='tanh', dropout=0.0).to(DEV).train()
    with pytest.raises(ValueError, match='115 columns, fc1 takes 116'):
        net.concat_train([torch.randn(4, 36, device=DEV), _bow(4, 50, 1)[0].to(DEV), torch.randn(4, 29, device=DEV)])
    with pytest.raises(NotImplementedError, match='inference path only'):
        net.concat_problem([torch.randn(4, 116, device=DEV)])


# ---- end to end: a two-tower step whose first text feature is a bag-of-words ------------------------------------------------------------
def test_end_to_end_two_towers_with_a_bow_feature():
    """The graph of test_gpu_fc_backward.py::test_end_to_end_two_towers_margin_loss with the first text feature a CSR bag-of-words through
    TransformNet.train().plane().  Every parameter gradient and every dense input's gradient within train_ref.end_to_end_bound."""
    from laff_amd import loss as laff_loss
    B, H, d, margin = 16, 2, 64, 0.2
    dims = (24, 16, 8)

    def build():
        txt, vis = TR.Side(dims, H * d, H), TR.Side(dims, H * d, H)
        with torch.no_grad():
            for p in list(txt.proj) + list(vis.proj):
                p.fc1.bias.uniform_(-0.2, 0.2)
        z = torch.randn(B, 8)
        csr, bow = _bow(B, dims[0], int(torch.randint(1 << 30, (1,))), per_row=5)
        ft = [bow] + [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims[1:]]
        fv = [z @ torch.randn(8, k) + 0.5 * torch.randn(B, k) for k in dims]
        with torch.no_grad():
            return (txt, vis, csr, ft, fv), TR.side_f64(txt, ft)[0], TR.side_f64(vis, fv)[0]
    txt, vis, csr, ft, fv = TR.hinge_clear_seed(build, margin, 200)
    with torch.no_grad():
        assert TR.hinge_slack(TR.side_f64(txt, ft)[0], TR.side_f64(vis, fv)[0], margin) >= TR.HINGE_CLEAR
    grads = {}
    for dtype in (torch.float64, torch.float32):
        (Et, lt), (Ev, lv) = TR.side_f64(txt, ft, dtype), TR.side_f64(vis, fv, dtype)
        TR.margin_loss_f64(Et, Ev, margin).backward()
        grads[dtype] = ({k: v.grad.double() for k, v in lt.items()}, {k: v.grad.double() for k, v in lv.items()}, Et, Ev)
    absjac = [TR.abs_jacobian(*TR.side_f64((txt, vis)[side], (ft, fv)[side])) for side in (0, 1)]
    txt, vis = txt.to(DEV).train(), vis.to(DEV).train()
    dt = [csr.to(DEV)] + [f.to(DEV).requires_grad_(True) for f in ft[1:]]
    dv = [f.to(DEV).requires_grad_(True) for f in fv]
    Et, Ev = txt(dt), vis(dv)
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    loss = crit(Et, Ev)
    loss.backward()
    torch.cuda.synchronize()
    l64 = float(TR.margin_loss_f64(grads[torch.float64][2].detach(), grads[torch.float64][3].detach(), margin))
    assert abs(loss.item() - l64) <= 2e-5 * max(1.0, abs(l64))
    worst = 0.0
    for side, (mod, feats) in enumerate(((txt, dt), (vis, dv))):
        got = {n: p.grad for n, p in mod.named_parameters()}
        got.update({'feat%d' % i: f.grad for i, f in enumerate(feats) if f.layout == torch.strided})
        for h in range(H):
            assert got.pop('att.attention_layer.%d.global_emb_weight_net.weight' % h) is None
        for n in ('att.layer_norm.weight', 'att.layer_norm.bias'):
            assert got.pop(n) is None
        ref64, ref32 = dict(grads[torch.float64][side]), grads[torch.float32][side]
        if side == 0:
            ref64.pop('feat0')                                               # counts: no gradient
        assert sorted(got) == sorted(ref64)
        for n, g in got.items():
            r = ref64[n]
            if n.endswith('embedding_common.0.bias'):
                assert not g.any(), n
                continue
            bound, e32, top = TR.end_to_end_bound(r, ref32[n], absjac[side][n])
            ratio = float(((g.cpu().double() - r).abs() / bound).max())
            worst = max(worst, ratio)
            print('side %d %-52s max |g| %.3e  fp32 CPU %.2e  worst err / bound %.3f' % (side, n, top, e32, ratio))
            assert ratio <= 1.0, (n, ratio)
    print('end to end with a bow feature: worst err / bound %.3f' % worst)


# MEASURED on the MI355X by test_backward_vs_float64: per case and tensor the largest fraction of its element-by-element bound that the
# device used.  Largest over all cases: dw 0.1436, db 0.1327 -- the short sums, where the bound is a handful of u of the products' magnitudes.
# Module level (CSR input and concat_train, the gather forward with its fused activation): largest error 9.63e-07 of a tensor's largest
# entry (bounds 1.5e-6 .. 3.0e-6).  End to end with a bow feature: the worst element used 0.159 of its bound.
#   case                                               dw        db
#   N1-Dk1-D4-None-values-dense-plain                  0.0576    0.0000
#   N3-Dk5-D8-tanh-ones-pitch4-holes                   0.1436    0.0734
#   N5-Dk8-D12-relu-values-pitch4-plain                0.0857    0.0348
#   N33-Dk70-D132-relu-values-pitch3-repeats           0.0518    0.0219
#   N129-Dk65-D260-sigmoid-ones-window-full            0.0032    0.0010
#   N17-Dk129-D8192-None-values-dense-plain            0.0913    0.1327
#   N64-Dk1000-D512-tanh-ones-dense-zipf               0.0232    0.0078
#   N130-Dk7811-D4096-sigmoid-values-dense-big         0.0057    0.0014
