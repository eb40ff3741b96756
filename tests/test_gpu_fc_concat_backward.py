"""laff_fc_concat_backward and ops.fc_concat_backward on the MI355X: the backward of the concat layer, all dense
segments in one launch per product, the CSR segments through the gather kernel on their windows.

The saved forward output A is an input of the call, so the reference is tests/fc_bwd_ref.backward in float64 on the CONCATENATED input
(the CSR segments densified) and on the very fp32 A, dA, X and W handed to the device.  The bounds are fc_bwd_ref.bounds, derived and
not measured, element by element (u = 2^-24, magnitudes in float64):

    |dW - ref| <= (N + 4) u |dA|^T |X|      |dX - ref| <= (D + 4) u |dA| |W|      |db - ref| <= (N + 4) u sum_n |dA|

They hold for any order of the sums, so for every cut.  A column of a CSR segment without entries has a zero bound: only the exact
zero passes.  At N <= 128 the sums over N are not cut and dW and db are, bit for bit, what the per-segment route writes
(ops.fc_backward / ops.fc_gather_backward on the windows, db by the first segment's call, as model.autograd._FcConcatFn does it).

The table at the end of the file records the largest fraction of its bound that each output used.
"""
import functools

import numpy as np
import pytest
import torch

import fc_bwd_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')

# (N, D, segments (width, 'd' dense | 'c' CSR), activation, segments that get a dX)
CASES = [
    (33, 64, ((36, 'd'), (50, 'c'), (30, 'd')), 'tanh', (2,)),            # the module test's shape; an unaligned window behind a CSR one
    (1, 4, ((1, 'd'), (1, 'd')), None, (0, 1)),                            # the smallest problem
    (37, 132, ((5, 'd'), (130, 'd'), (64, 'd'), (3, 'd')), 'relu', (0, 1, 2, 3)),   # narrower than a tile, spanning tiles, a partial D tile
    (130, 68, ((64, 'd'), (68, 'd')), 'sigmoid', (0,)),                    # the sum over N is cut
    (32, 260, ((128, 'd'), (128, 'd')), 'tanh', (0, 1)),                   # aligned rows but partial tiles (general kernels); dX's sum cut
    (64, 64, ((64, 'd'), (128, 'd')), 'tanh', (0, 1)),                     # whole 64 x 64 tiles, aligned rows: the FAST kernels, dW and dX
    (64, 64, ((64, 'd'), (4, 'd'), (64, 'd')), 'relu', (0, 1, 2)),         # one segment narrower than a tile: the general kernels for all
    (128, 2048, ((1024, 'd'), (1024, 'd')), 'tanh', (0, 1)),               # 128 x 128 tiles, FAST, dW and dX; dX's sum cut 16 ways
    (127, 2048, ((1000, 'd'), (1048, 'd')), 'sigmoid', (0, 1)),            # 128 x 128 tiles, the general kernels
    (16, 8, ((4, 'd'), (8, 'c'), (12, 'd'), (16, 'c'), (20, 'd'), (24, 'd'), (28, 'd'), (32, 'c')), 'tanh', ()),   # 8 segments
    (9, 16, ((66, 'c'), (50, 'c')), 'relu', ()),                           # no dense launch; db from a gather launch
    (0, 8, ((4, 'd'), (4, 'c')), 'tanh', (0,)),                            # N == 0
]


def _id(c):
    return 'N%d-D%d-%s-%s' % (c[0], c[1], '+'.join('%d%s' % (w, 'c' if k == 'c' else '') for w, k in c[2]), c[3])


def _bow(N, Dk, rng, per_row=6):
    dense = torch.zeros(N, Dk)
    for n in range(N):
        for v in rng.choice(Dk, size=rng.integers(1, min(per_row, Dk) + 1), replace=False):
            dense[n, v] = float(rng.integers(1, 4))
    return dense


@functools.lru_cache(maxsize=None)
def _case(c):
    """The fp32 operands on the CPU, the float64 reference and the bounds -- computed once, shared, never written."""
    from laff_amd import ops
    N, D, segs, act, _ = c
    seed = N * 1000003 + D * 1009 + len(segs)
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    xs, cscs = [], []
    for w, kind in segs:
        if kind == 'c':
            x = _bow(N, w, rng)
            sp = x.to_sparse_csr()
            csr = torch.sparse_csr_tensor(sp.crow_indices().to(torch.int32), sp.col_indices().to(torch.int32), sp.values(), size=(N, w))
            cscs.append(ops.csr_transpose(csr))
        else:
            x = torch.randn(N, w, generator=g)
            cscs.append(None)
        xs.append(x)
    K = sum(w for w, _ in segs)
    W = torch.randn(D, K, generator=g) / K ** 0.5
    z = 3.0 * torch.randn(N, D, generator=g)                                # logits x 3: part of A sits in saturation
    a = {None: lambda t: t, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'relu': torch.relu}[act](z)
    da = torch.randn(N, D, generator=g)
    xcat = torch.cat(xs, 1)
    return dict(xs=xs, cscs=cscs, W=W, a=a, da=da, ref=R.backward(xcat, W, a, da, act), bounds=R.bounds(xcat, W, da), K=K)


@functools.lru_cache(maxsize=None)
def _device_inputs(c):
    cs = _case(c)
    segs = [x.to(DEV) if csc is None else tuple(t.to(DEV) for t in csc) for x, csc in zip(cs['xs'], cs['cscs'])]
    return segs, cs['W'].to(DEV), cs['a'].to(DEV), cs['da'].to(DEV)


def _columns(c):
    return np.concatenate([[0], np.cumsum([w for w, _ in c[2]])]).astype(int)


def _launch(c, want_dw=True, want_db=True, want_dx=None, layout='pitch3'):
    """ops.fc_concat_backward into NaN-framed buffers: (dxs, dw, db) after the frame check."""
    from laff_amd import ops
    N, D, segs, act, dx_for = c
    want_dx = [j in dx_for for j in range(len(segs))] if want_dx is None else want_dx
    dsegs, W, a, da = _device_inputs(c)
    K = W.shape[1]
    bdw = TR.pitched(D, K, layout) if want_dw else None
    bdb = TR.out_vec(D) if want_db else None
    bdx = [TR.pitched(N, w, layout) if f else None for (w, _), f in zip(segs, want_dx)]
    dxs, dw, db = ops.fc_concat_backward(dsegs, W, a, da, act, want_dx=want_dx, want_dw=want_dw, want_db=want_db,
                                         out=([None if b is None else b[1] for b in bdx], None if bdw is None else bdw[1],
                                              None if bdb is None else bdb[1]))
    torch.cuda.synchronize()
    for name, b, r in [('dw', bdw, dw), ('db', bdb, db)] + [('dx%d' % j, b, r) for j, (b, r) in enumerate(zip(bdx, dxs))]:
        if b is None:
            assert r is None, name
            continue
        assert r.data_ptr() == b[1].data_ptr()
        assert TR.untouched_around(*b), '%s: a write outside the output' % name
        assert not r.isnan().any(), '%s: an element was not written' % name
    return dxs, dw, db


def _frac(err, bound):
    # a zero bound (a column without entries, a zero row of |dA|) admits only the exact zero
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)), initial=0.0))


def _check(c, res, label=''):
    cs = _case(c)
    dxs, dw, db = res
    rdx, rdw, rdb = cs['ref']
    bdx, bdw, bdb = cs['bounds']
    cols = _columns(c)
    fracs = {}
    if dw is not None:
        fracs['dw'] = _frac(np.abs(dw.cpu().numpy().astype(np.float64) - rdw), bdw)
    if db is not None:
        fracs['db'] = _frac(np.abs(db.cpu().numpy().astype(np.float64) - rdb), bdb)
    got = [(j, dx) for j, dx in enumerate(dxs) if dx is not None]
    if got:
        fracs['dx'] = max(_frac(np.abs(dx.cpu().numpy().astype(np.float64) - rdx[:, cols[j]:cols[j + 1]]), bdx[:, cols[j]:cols[j + 1]])
                          for j, dx in got)
    for name, f in fracs.items():
        print('%s %s%s: largest err / bound %.4f' % (_id(c), name, label, f))
        assert f <= 1.0, (name, f)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_backward_vs_float64(c):
    from laff_amd import ops
    res = _launch(c)
    assert [dx is not None for dx in res[0]] == [j in c[4] for j in range(len(c[2]))]
    _check(c, res)
    if c[0] == 0:
        assert not res[1].any() and not res[2].any() and not torch.signbit(res[1]).any()
    plan = ops.fc_concat_backward_plan(c[0], c[1], _device_inputs(c)[0], [j in c[4] for j in range(len(c[2]))])
    if c[0] == 130:
        assert plan[0] > 1 and plan[1] > 0                                   # the case that is there for the cut over N
    if c[1] == 260:
        assert plan[0] == 1 and plan[2] > 1                                  # ... and the one for the cut over D
    assert plan[3] == (3 if c[1] == 2048 else 0)                             # the cases that are there for the 128 x 128 tiles


def _per_segment_route(c):
    """dW and db as model.autograd._FcConcatFn.backward writes them: one call per segment on the windows, db by the first one's."""
    from laff_amd import ops
    N, D, segs, act, _ = c
    dsegs, W, a, da = _device_inputs(c)
    dw = torch.full_like(W, NAN)
    db = torch.full((D,), NAN, device=DEV)
    cols = _columns(c)
    for j, ((w, kind), x) in enumerate(zip(segs, dsegs)):
        window, first = dw[:, cols[j]:cols[j + 1]], db if j == 0 else None
        if kind == 'c':
            ops.fc_gather_backward(x, N, w, a, da, act, want_dw=True, want_db=first is not None, out=(window, first))
        else:
            ops.fc_backward(x, W[:, cols[j]:cols[j + 1]], a, da, act, want_dx=False, want_dw=True, want_db=first is not None,
                            out=(None, window, first))
    return dw, db


@pytest.mark.parametrize('c', [c for c in CASES if 0 < c[0] <= 128], ids=_id)
def test_dw_and_db_have_the_bits_of_the_per_segment_route(c):
    _, dw, db = _launch(c, layout='dense')
    rdw, rdb = _per_segment_route(c)
    assert torch.equal(dw, rdw), 'dW differs from the per-segment route'
    assert torch.equal(db, rdb), 'db differs from the per-segment route'


@pytest.mark.parametrize('c', [CASES[0], CASES[2], CASES[3], CASES[4], CASES[5], CASES[6]], ids=_id)
def test_output_layouts_give_the_same_bits(c):
    dense = _launch(c, layout='dense')
    for layout in ('pitch4', 'pitch3', 'window'):
        res = _launch(c, layout=layout)
        assert torch.equal(res[1], dense[1]) and torch.equal(res[2], dense[2]), layout
        assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(res[0], dense[0])), layout


FAST = CASES[5]


def test_one_segment_that_breaks_the_alignment_takes_the_whole_launch_off_the_fast_kernels():
    """The FAST kernels load 16 bytes without a guard, so a launch may take them only when EVERY segment has whole tiles and 16-byte
    aligned rows.  The FAST case again with one operand of one segment moved off that -- an X with a pitch of 67 or 129 floats, an X
    4 bytes past a 16-byte boundary, a window of W and dW at an odd column -- has to give the bits of the aligned call (the general
    kernels run the same chains) inside intact NaN frames."""
    from laff_amd import ops
    assert FAST[:2] == (64, 64) and [w for w, _ in FAST[2]] == [64, 128]
    N, D, segs, act, _ = FAST
    dsegs, W, a, da = _device_inputs(FAST)
    want = _launch(FAST, layout='dense')
    _check(FAST, want, ' (fast)')
    for which, layout in ((0, 'pitch3'), (1, 'pitch3'), (1, 'offset')):
        moved = list(dsegs)
        buf, moved[which] = TR.place(_case(FAST)['xs'][which], layout)
        assert torch.equal(moved[which], dsegs[which])
        got = ops.fc_concat_backward(moved, W, a, da, act, want_dx=[True, True])
        torch.cuda.synchronize()
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (which, layout)
        assert all(torch.equal(p, q) for p, q in zip(got[0], want[0])), (which, layout)
    # the windows at columns 1 and 65 of a wider weight: W + col and dW + col are 4 bytes past a 16-byte boundary
    K = 200
    wide = torch.randn(D, K, device=DEV)
    wide[:, 1:65], wide[:, 65:193] = W[:, :64], W[:, 64:]
    buf, dw = TR.pitched(D, K, 'dense')
    got = ops.fc_concat_backward(dsegs, wide, a, da, act, want_dx=[True, True], out=(None, dw, None), columns=[1, 65])
    torch.cuda.synchronize()
    assert TR.untouched_around(buf, dw) and dw[:, :1].isnan().all() and dw[:, 193:].isnan().all()
    assert torch.equal(dw[:, 1:193], want[1]) and torch.equal(got[2], want[2])
    assert all(torch.equal(p, q) for p, q in zip(got[0], want[0]))


def test_windows_that_leave_columns_out_keep_the_rest_of_dw():
    """Two dense windows and a CSR one inside a wider K: the columns between and around them keep their NaNs, the windows hold what the
    same segments give as a full cover of their own weight."""
    from laff_amd import ops
    c = CASES[0]
    N, D, segs, act, _ = c
    dsegs, W, a, da = _device_inputs(c)
    widths = [w for w, _ in segs]
    columns = [3, 45, 101]                                                    # 36 -> [3, 39), 50 -> [45, 95), 30 -> [101, 131); K = 140
    K = 140
    wide = torch.randn(D, K, device=DEV)
    for j, col in enumerate(columns):
        wide[:, col:col + widths[j]] = W[:, _columns(c)[j]:_columns(c)[j + 1]]
    buf, dw = TR.pitched(D, K, 'pitch3')
    bdx = TR.pitched(N, widths[2], 'pitch3')
    dxs, got, db = ops.fc_concat_backward(dsegs, wide, a, da, act, want_dx=[False, False, True], out=([None, None, bdx[1]], dw, None),
                                          columns=columns)
    torch.cuda.synchronize()
    assert TR.untouched_around(buf, dw) and TR.untouched_around(*bdx)
    full = _launch(c, layout='dense')
    inside = torch.zeros(K, dtype=torch.bool, device=DEV)
    for j, col in enumerate(columns):
        inside[col:col + widths[j]] = True
        assert torch.equal(got[:, col:col + widths[j]], full[1][:, _columns(c)[j]:_columns(c)[j + 1]]), j
    assert got[:, ~inside].isnan().all() and not got[:, inside].isnan().any()
    assert torch.equal(db, full[2]) and torch.equal(dxs[2], full[0][2])


@pytest.mark.parametrize('c', [CASES[0], CASES[2], CASES[3], CASES[4], CASES[5], CASES[7], CASES[10]], ids=_id)
def test_each_output_alone_and_repeats_are_bit_identical(c):
    from laff_amd import ops
    n = len(c[2])
    full = _launch(c)
    again = _launch(c)
    assert torch.equal(again[1], full[1]) and torch.equal(again[2], full[2])
    assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(again[0], full[0]))
    dxs, dw, db = _launch(c, True, False, [False] * n)
    assert db is None and dxs == [None] * n and torch.equal(dw, full[1])
    dxs, dw, db = _launch(c, False, True, [False] * n)
    assert dw is None and dxs == [None] * n and torch.equal(db, full[2])
    if c[4]:
        dxs, dw, db = _launch(c, False, False)
        assert dw is None and db is None
        assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(dxs, full[0]))
    dsegs, W, a, da = _device_inputs(c)
    assert ops.fc_concat_backward(dsegs, W, a, da, c[3], want_dw=False, want_db=False) == ([None] * n, None, None)


@pytest.mark.parametrize('c', [CASES[0], CASES[3], CASES[5]], ids=_id)
def test_graph_capture_replays_the_eager_bits(c):
    from laff_amd import ops
    N, D, segs, act, dx_for = c
    dsegs, W, a, da = _device_inputs(c)
    want_dx = [j in dx_for for j in range(len(segs))]
    eager = ops.fc_concat_backward(dsegs, W, a, da, act, want_dx=want_dx)
    eager = ([None if t is None else t.clone() for t in eager[0]], eager[1].clone(), eager[2].clone())
    outs = ([torch.full((N, w), NAN, device=DEV) if f else None for (w, _), f in zip(segs, want_dx)],
            torch.full((D, W.shape[1]), NAN, device=DEV), torch.full((D,), NAN, device=DEV))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        ops.fc_concat_backward(dsegs, W, a, da, act, want_dx=want_dx, out=outs)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[1], eager[1]) and torch.equal(outs[2], eager[2])
    assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(outs[0], eager[0]))
    _check(c, outs, ' (graph)')


def test_argument_errors():
    from laff_amd import ops
    c = CASES[0]
    dsegs, W, a, da = _device_inputs(c)
    with pytest.raises(ValueError, match='activation'):
        ops.fc_concat_backward(dsegs, W, a, da, 'gelu')
    with pytest.raises(ValueError, match='no dx'):
        ops.fc_concat_backward(dsegs, W, a, da, 'tanh', want_dx=[False, True, False])
    with pytest.raises(ValueError, match='do not fit'):
        ops.fc_concat_backward(dsegs[:2], W, a, da, 'tanh')
    with pytest.raises(TypeError):
        ops.fc_concat_backward(dsegs, W.double(), a, da, 'tanh')
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fc_concat_backward(dsegs, W, a.cpu(), da, 'tanh')


# MEASURED on the MI355X by test_backward_vs_float64: per case and output the largest fraction of its element-by-element bound that the
# device used.  Largest over all cases: dw 0.1636 (the smallest problem: the bound is five roundings of one product), db 0.0467, dx 0.0257.
#   case                                          dw        db        dx
#   N33-D64-36+50c+30-tanh                        0.0518    0.0175    0.0150
#   N1-D4-1+1-None                                0.1636    0.0000    0.0091
#   N37-D132-5+130+64+3-relu                      0.0512    0.0213    0.0095
#   N130-D68-64+68-sigmoid                        0.0031    0.0010    0.0071
#   N32-D260-128+128-tanh                         0.0662    0.0180    0.0033
#   N64-D64-64+128-tanh                           0.0209    0.0069    0.0257
#   N64-D64-64+4+64-relu                          0.0243    0.0096    0.0244
#   N128-D2048-1024+1024-tanh                     0.0221    0.0065    0.0001
#   N127-D2048-1000+1048-sigmoid                  0.0067    0.0022    0.0000
#   N16-D8-4+8c+12+16c+20+24+28+32c-tanh          0.0686    0.0142    -
#   N9-D16-66c+50c-relu                           0.0880    0.0467    -
#   N0-D8-4+4c-tanh                               0         0         0
