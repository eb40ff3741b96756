"""The strip form of the FC projection on v_mfma_f32_16x16x32_f16 (laff_amd/csrc/fc_strip16.hip) beside the one on
v_mfma_f32_32x32x16_f16 (fc_strip.hip).  Both sit behind laff_fc_strip_pack / laff_fc_act_bn_strip_grouped; LAFF_FC_STRIP_MFMA,
read when a context is created, picks: 16 (default) or 32.  An image is launched in the mode it was packed in."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layer(g, D):
    W = (g.normal(0, 1, (D, 512)) / np.sqrt(512)).astype(np.float32)
    return W, g.normal(0, 0.1, D).astype(np.float32), g.uniform(0.5, 1.5, D).astype(np.float32), g.normal(0, 0.1, D).astype(np.float32)


def _ref64(x, W, b, sc, sh, act):
    pre = x.astype(np.float64) @ W.astype(np.float64).T + b
    f = {None: lambda v: v, 'tanh': np.tanh, 'relu': lambda v: np.maximum(v, 0)}[act]
    ref = f(pre) * sc + sh
    scale = 1.0 if act == 'tanh' else np.maximum(1.0, np.abs(pre).max(axis=1, keepdims=True))
    return ref, scale


@pytest.fixture
def mfma_mode():
    from laff_amd import ops

    def set_mode(m):
        os.environ['LAFF_FC_STRIP_MFMA'] = str(m)
        ops.reset_contexts()
    yield set_mode
    os.environ.pop('LAFF_FC_STRIP_MFMA', None)
    ops.reset_contexts()


@pytest.mark.parametrize('N,D,act', [(1, 32, 'tanh'), (31, 64, 'tanh'), (129, 512, None), (300, 512, 'relu'), (257, 4096, 'tanh')])
def test_both_mfma_shapes_vs_fp64(mfma_mode, N, D, act):
    """Each kernel against float64 at the FC forms' tolerance (2e-5, scaled by the row's largest pre-activation where the output is
    not bounded), incl. a row beyond the fp16 range, a tiny row and a zero row; on the tanh cases the two agree within 5e-6."""
    from laff_amd import ops
    g = np.random.default_rng(N + D)
    x = g.normal(0, 1, (N, 512)).astype(np.float32)
    x[0] *= 3e4
    if N > 2:
        x[1] *= 1e-6
        x[2] = 0
    W, b, sc, sh = _layer(g, D)
    ref, scale = _ref64(x, W, b, sc, sh, act)
    ys = {}
    for mode in (16, 32):
        mfma_mode(mode)
        sw = ops.fc_strip_pack(dev(W), dev(b), dev(sc), dev(sh), act)
        ys[mode] = ops.fc_act_bn_strip_grouped([dict(x=dev(x), strip=sw)])[0].cpu().numpy()
        err = float(np.max(np.abs(ys[mode] - ref) / scale))
        print('mfma', mode, (N, D, act), 'scaled error vs float64', err)
        assert err <= 2e-5, mode
    if act == 'tanh':
        d = float(np.max(np.abs(ys[16] - ys[32])))
        print('16 vs 32', (N, D, act), d)
        assert d <= 5e-6


@pytest.mark.parametrize('N,D', [(9000, 32), (12800, 64), (6000, 96), (40000, 96), (33000, 160), (12800, 1024)])
def test_every_segment_form(mfma_mode, N, D):
    """launch_fc_strip cuts the ceil(N / 128) * (D / 32) (strip, column block) units into min(#CUs, units) contiguous ranges; a
    segment is the blocks of one strip inside a range.  The first three shapes have fewer units than a 256-CU device has CUs: every
    workgroup runs ONE one-block segment with nothing ahead (a cold strip load, the drain straight behind the first block).  The
    last three have 939, 1,290 and 3,200 units, several per workgroup, and between them reach every other form: segments of 1, 2
    and 3+ blocks, with a successor (the tail copies whose last three bodies carry rounds 0..2 of the next strip's rows, round 3
    into the staging buffer, round 4 in front of the drain) and without, the strip load that finds its first rounds already in
    the ring (the counted waits of its 'pre' branch), an empty plain loop, and both parities of the block behind the plain loop.
    Whole outputs against the fp32-MFMA path, and float64 on the first and last rows."""
    from laff_amd import ops
    mfma_mode(16)
    g = np.random.default_rng(N + D)
    x = g.normal(0, 1, (N, 512)).astype(np.float32)
    W, b, sc, sh = _layer(g, D)
    sw = ops.fc_strip_pack(dev(W), dev(b), dev(sc), dev(sh), 'tanh')
    y = ops.fc_act_bn_strip_grouped([dict(x=dev(x), strip=sw)])[0]
    y32 = ops.fc_act_bn(dev(x), dev(W), dev(b), dev(sc), dev(sh), 'tanh')
    d = float((y - y32).abs().max())
    print((N, D), 'vs fc_act_bn', d)
    assert d <= 2e-5
    rows = np.r_[0:300, N - 300:N]
    ref, _ = _ref64(x[rows], W, b, sc, sh, 'tanh')
    d64 = float(np.max(np.abs(y.cpu().numpy()[rows] - ref)))
    print((N, D), 'vs float64 on 600 rows', d64)
    assert d64 <= 2e-5


@pytest.mark.parametrize('N,D,mode', [pytest.param(300, 96, 16, id='300-96'), pytest.param(300, 96, 32, id='300-96-mfma32'),
                                      pytest.param(33000, 160, 16, id='33000-160')])
def test_layout_detector(mfma_mode, N, D, mode):
    """W[c][k] = an integer pattern of (c, k), X = one-hot rows (row r has its 1 at k_r), no bias, BatchNorm or activation: Y[r][c] =
    W[c][k_r] exactly (integers below 2048 times powers of two are exact in the fp16 hi halves, the lo halves are zero).  A wrong
    lane <-> (row, k, column) mapping anywhere -- the strip read-back, the image, the epilogue -- puts exact integers in the wrong
    place.  (300, 96): one-block segments, cold strip loads, in both MFMA modes (the two image layouts are the two branches of one
    pack kernel).  (33000, 160): five units per workgroup -- segments with a successor, so the strips whose first rounds come early,
    through other buffers and in another order, are read back exactly too.  Input and output rows carry a pitch: nothing outside
    [N, D] is written."""
    from laff_amd import ops
    mfma_mode(mode)
    c, k = np.meshgrid(np.arange(D), np.arange(512), indexing='ij')
    W = dev(((c * 512 + k) % 2039 + 1).astype(np.float32))
    kr = (torch.arange(N, device='cuda') * 37 + 11) % 512
    xb = torch.zeros((N, 520), device='cuda')
    xb[torch.arange(N, device='cuda'), kr] = 1.0
    out_full = torch.full((N, D + 5), -7.0, device='cuda')
    sw = ops.fc_strip_pack(W, None, None, None, None)
    y = ops.fc_act_bn_strip_grouped([dict(x=xb[:, :512], strip=sw, out=out_full[:, :D])])[0]
    want = W[:, kr].T
    bad = torch.nonzero(y != want)
    assert bad.shape[0] == 0, (int(bad.shape[0]), bad[:8].tolist(), float(y[tuple(bad[0])]), float(want[tuple(bad[0])]))
    assert bool((out_full[:, D:] == -7.0).all())


def test_an_image_is_refused_in_the_other_mode(mfma_mode):
    """The two image layouts differ: ops.fc_strip_pack records the mode, ops.fc_act_bn_strip_grouped refuses an image packed under
    the other one, and TransformNet.strip_weights() packs again after the mode has changed."""
    from laff_amd import ops, synth
    mfma_mode(32)
    g = np.random.default_rng(7)
    W, b, sc, sh = _layer(g, 64)
    x = dev(g.normal(0, 1, (40, 512)).astype(np.float32))
    sw = ops.fc_strip_pack(dev(W), dev(b), dev(sc), dev(sh), 'tanh')
    assert sw.mfma == 32
    model = synth.build_model(1, 512, torch.device('cuda'), seed=3)
    net = next(m for m in model.modules() if hasattr(m, 'strip_weights') and getattr(m, 'fc1', None) is not None)
    a = net.strip_weights()
    mfma_mode(16)
    with pytest.raises(ValueError):
        ops.fc_act_bn_strip_grouped([dict(x=x, strip=sw)])
    b16 = net.strip_weights()
    assert a.mfma == 32 and b16.mfma == 16 and b16 is not a
