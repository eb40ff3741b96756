"""The closed form of the frame attention's backward (tests/frame_bwd_ref.py) against float64 autograd of tests/fuse_ref.frame_attention,
the plan and the argument checks of laff_frame_fuse_backward, and what Attention_1.fuse_frames and the FrameLAFF tower refuse in training
mode.  All on the CPU."""
import ctypes as C
import itertools

import pytest
import torch

import frame_bwd_ref as R

FLAGS = [dict(with_ave=a, mul=m) for a, m in itertools.product((False, True), repeat=2)]
SHAPES = [(5, 1, 36), (5, 5, 516), (7, 31, 384), (7, 33, 508), (9, 50, 512)]


def _case(B, Fmax, d, with_lens, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    frames = (0.5 * torch.randn(B, Fmax, d, generator=g, dtype=torch.float64)).float()
    w = (torch.randn(d, generator=g, dtype=torch.float64) / d ** 0.5).float()
    b = (0.1 * torch.randn(1, generator=g, dtype=torch.float64)).float()
    gw = (0.5 + torch.rand(1, generator=g, dtype=torch.float64)).float()
    dV = torch.randn(B, d, generator=g, dtype=torch.float64).float()
    lens = None
    if with_lens:
        lens = torch.randint(1, Fmax + 1, (B,), generator=g).to(torch.int32)
        lens[0], lens[1], lens[2] = 0, 1, Fmax
        frames[torch.arange(Fmax)[None, :] >= lens[:, None]] = float('nan')          # the padded rows are never read
    return frames, w, b, gw, dV, lens


@pytest.mark.parametrize('with_lens', (False, True), ids=('full', 'lens'))
@pytest.mark.parametrize('kw', FLAGS, ids=lambda kw: '+'.join(k for k, v in kw.items() if v) or 'plain')
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_closed_form_agrees_with_float64_autograd(shape, kw, with_lens):
    frames, w, b, gw, dV, lens = _case(*shape, with_lens)
    cf = R.closed_form(frames, w, b, gw, dV, lens=lens, **kw)
    dx, dw, db = R.autograd_grads(frames, w, b, gw, dV, lens=lens, **kw)
    assert cf['dx'].shape == dx.shape == frames.shape and torch.isfinite(cf['dx']).all() and torch.isfinite(dx).all()
    e_dx, e_dw = R.rel_err(cf['dx'], dx), R.rel_err(cf['dw'], dw)
    print('dx %.3g  dw %.3g' % (e_dx, e_dw))
    assert e_dx <= 1e-12 and e_dw <= 1e-12
    assert not db.any() and not cf['db'].any()
    if lens is not None:
        pad = torch.arange(shape[1])[None, :] >= lens[:, None]
        assert not cf['dx'][pad].any() and not dx[pad].any() and not cf['dx'][0].any()       # padded rows, the zero-length video
    if shape[1] == 1:
        assert not cf['dw'].any() and not dw.any()                   # a softmax over one logit is constant
    else:
        assert cf['dw'].any()


def test_float32_autograd_runs_in_float32_and_is_close():
    frames, w, b, gw, dV, lens = _case(7, 33, 508, True)
    kw = dict(with_ave=True, mul=True, lens=lens)
    d64 = R.autograd_grads(frames, w, b, gw, dV, **kw)
    d32 = R.autograd_grads(frames, w, b, gw, dV, dtype=torch.float32, **kw)
    for a, b_ in zip(d32[:2], d64[:2]):
        assert 0.0 < R.rel_err(a, b_) < 1e-5


# ---- the C ABI: the plan and the argument errors need no GPU ------------------------------------------------------------------------
def test_plan_and_argument_errors_do_not_need_a_gpu():
    from laff_amd import _lib, ops
    lib = _lib.load()
    out = (C.c_int * 4)(7, 7, 7, 7)
    # one partial row of dw per (feature, video); the variant is the number of 256-column chunks a lane owns; 8 features a launch
    assert ops.frame_fuse_backward_plan(1, 128, 50, 512) == (128 * 512 * 4, 2, 1, 128)
    assert ops.frame_fuse_backward_plan(9, 7, 5, 36) == (9 * 7 * 36 * 4, 1, 2, 7)
    assert ops.frame_fuse_backward_plan(4, 3000, 32, 1024, want_dw=False) == (0, 4, 1, 0)
    assert [ops.frame_fuse_backward_plan(1, 1, 1, d)[1] for d in (4, 256, 260, 512, 516, 1024)] == [1, 1, 2, 2, 4, 4]
    assert ops.frame_fuse_backward_plan(0, 0, 1, 4) == (0, 1, 0, 0)
    assert lib.laff_frame_fuse_backward_plan(1, 4, 5, 36, 1, None) == -1 and b'null out' in lib.laff_last_error()
    for bad in ((1, 4, 5, 1028), (1, 4, 5, 6), (1, 4, 5, 0), (1, 4, 0, 36), (1, -1, 5, 36), (-1, 4, 5, 36)):
        assert lib.laff_frame_fuse_backward_plan(*bad, 1, out) == -2, bad                          # LAFF_E_SHAPE
        assert b'laff_frame_fuse_backward_plan' in lib.laff_last_error()
    assert tuple(out) == (7, 7, 7, 7)                                                              # untouched by the refusals

    def call(ctx, count, B, Fmax, d, flags, lddv):
        return lib.laff_frame_fuse_backward(ctx, count, None, None, B, Fmax, d, None, None, None, flags, None, lddv, None, None, None,
                                            None, 0)
    assert call(None, 1, 4, 5, 36, 3, 36) == -1                                                    # LAFF_E_ARG: no ctx
    assert b'laff_frame_fuse_backward' in lib.laff_last_error() and b'ctx' in lib.laff_last_error()
    for bad in ((1, 4, 5, 1028), (1, 4, 5, 6), (1, 4, 0, 36)):
        assert call(None, *bad, 3, bad[3]) == -2, bad
    assert call(None, 1, 4, 5, 36, 4, 36) == -1 and b'flags' in lib.laff_last_error()              # L2NORM_EACH_HEAD: not a frame flag
    assert call(None, 1, 4, 5, 36, 1 << 7, 36) == -1 and b'flags' in lib.laff_last_error()
    assert call(None, 1, 4, 5, 36, 3, 32) == -2 and b'lddv' in lib.laff_last_error()               # lddv < d
    assert call(None, 1, 4, 5, 36, 3, 38) == -2 and b'lddv' in lib.laff_last_error()               # not a multiple of 4


def test_abi_version():
    """(The ABI version itself: test_cabi.py, ENTRY_POINTS.)"""
    assert 'frame_fuse_backward' in __import__('laff_amd.ops', fromlist=['x']).__all__
    assert 'frame_fuse_backward_plan' in __import__('laff_amd.ops', fromlist=['x']).__all__


# ---- ops and modules: what they refuse, before anything touches a device -----------------------------------------------------------
def test_ops_frame_fuse_backward_refuses_cpu_and_non_fp32_tensors():
    from laff_amd import ops
    x, w, b, g = torch.zeros(4, 5, 16), torch.zeros(16), torch.zeros(1), torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.frame_fuse_backward([x], None, [(w, b, None)], 0, [g])
    with pytest.raises(TypeError, match='float32'):
        ops.frame_fuse_backward([_FakeDevice(x.double())], None, [(w, b, None)], 0, [g])


def test_fuse_frames_refuses_dtype_and_shape():
    """RuntimeError('no CPU path') for CPU frames, TypeError for non-fp32 frames, ValueError for frames that are not (B, Fmax, d).
    The last two are decided from the tensor's metadata once it is known to be on a device: _FakeDevice stands in for one."""
    from laff_amd.model.Attention import Attention_1
    m = Attention_1(16, with_ave=True, mul=True).train()
    assert m.training
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.fuse_frames(torch.zeros(4, 5, 16))
    with pytest.raises(TypeError, match='float32'):
        m.fuse_frames(_FakeDevice(torch.zeros(4, 5, 16, dtype=torch.float64)))
    for bad in (torch.zeros(4, 16), torch.zeros(4, 5, 12), torch.zeros(2, 4, 5, 16)):
        with pytest.raises(ValueError, match='frames must be'):
            m.fuse_frames(_FakeDevice(bad))


class _FakeDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda with True: lets the checks that follow the device check run without a device."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_tower_in_train_mode_still_raises_from_prepare():
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    for add_fc in (False, True):
        cfg = make_config({}, {'bow': 8}, 64, 2, 'FrameLAFF', frame_feats={'clip_frame': 16}, batch_norm=False,
                          vis_frame_attention='attention_noAveNoAverageMul', vis_frame_addFC=add_fc, frame_feat_with_video_feat=False)
        tower = get_model('FrameLAFF', 'cpu', cfg).vis_net.train()
        assert len(tower.frame_attention['clip_frame']) == (2 if add_fc else 1)
        with pytest.raises(NotImplementedError, match='inference path only'):
            tower.prepare({}, {'clip_frame': torch.zeros(2, 3, 16), 'mask_tensor': torch.ones(2, 3)})
        with pytest.raises(NotImplementedError, match='inference path only'):
            tower({}, {'clip_frame': torch.zeros(2, 3, 16), 'mask_tensor': torch.ones(2, 3)})
