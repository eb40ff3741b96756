"""The closed forms of the fusion's backward (tests/fuse_bwd_ref.py) against float64 autograd of tests/fuse_ref.attention, what the
training-mode attention modules refuse, and the argument checks of laff_fuse_backward.  All on the CPU."""
import ctypes as C
import itertools

import pytest
import torch

import fuse_bwd_ref as R

FLAGS = [dict(with_ave=a, mul=m, l2norm_each_head=n, split_head=s) for a, m, n, s in itertools.product((False, True), repeat=4)]
FLAGS.append(dict(just_average=True))
FLAGS.append(dict(just_average=True, split_head=False))


def _case(kw, N=7, L=4, H=3, d=12, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    Dp = H * d if kw.get('split_head', True) else d
    planes = 0.5 * torch.randn(N, L, Dp, generator=g, dtype=torch.float64)
    w = torch.randn(H, d, generator=g, dtype=torch.float64) / d ** 0.5
    b = 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    gw = 0.5 + torch.rand(H, generator=g, dtype=torch.float64)
    dE = torch.randn(N, H, d, generator=g, dtype=torch.float64)
    return planes, H, d, w, b, gw, dE


@pytest.mark.parametrize('kw', FLAGS, ids=lambda kw: '-'.join(k for k, v in kw.items() if v) or 'plain')
def test_closed_forms_agree_with_float64_autograd(kw):
    args = _case(kw)
    cf = R.closed_form(*args, **kw)
    dx, dw, db = R.autograd_grads(*args, **kw)
    assert float(cf['g_norm'].min()) >= 0.05 and float(cf['raw_norm'].min()) >= 0.05
    assert cf['dx'].shape == dx.shape == args[0].shape
    e_dx, e_dw = R.rel_err(cf['dx'], dx), R.rel_err(cf['dw'], dw)
    print('dx %.3g  dw %.3g  |db| autograd %.3g closed %.3g' % (e_dx, e_dw, float(db.abs().max()), float(cf['db'].abs().max())))
    assert e_dx <= 1e-12 and e_dw <= 1e-12
    # db is identically zero (softmax does not see a shift of its logits): rounding only, in the closed form and in autograd
    N, L = args[0].shape[:2]
    tiny = 1e-12 * float(cf['dz'].abs().max()) * N * L
    assert float(cf['db'].abs().max()) <= tiny and float(db.abs().max()) <= tiny
    if not kw.get('just_average'):
        assert float(cf['dz'].abs().max()) > 0.0


def test_a_single_plane_has_no_parameter_gradient():
    kw = dict(with_ave=True, mul=True)
    args = _case(kw, L=1)
    cf = R.closed_form(*args, **kw)
    dx, dw, db = R.autograd_grads(*args, **kw)
    assert not cf['dw'].any() and not dw.any() and R.rel_err(cf['dx'], dx) <= 1e-12
    assert R.rel_err(torch.zeros(3), torch.zeros(3)) == 0.0 and R.rel_err(torch.ones(3), torch.zeros(3)) == float('inf')


def test_float32_autograd_runs_in_float32_and_is_close():
    kw = dict(with_ave=True, mul=True, l2norm_each_head=True)
    args = _case(kw)
    d64 = R.autograd_grads(*args, **kw)
    d32 = R.autograd_grads(*[a.float() if isinstance(a, torch.Tensor) else a for a in args], dtype=torch.float32, **kw)
    for a, b in zip(d32[:2], d64[:2]):
        assert 0.0 < R.rel_err(a, b) < 1e-5


# ---- the training-mode modules: what they refuse, before anything touches a device ------------------------------------------------
def _modules():
    from laff_amd.model.Attention import Attention_1, JustAverage, Multi_head_MyApply_Attention
    return [Attention_1(16), Multi_head_MyApply_Attention(16, 2, 8), JustAverage()]


@pytest.mark.parametrize('what,plane', [('tiled', lambda x, v: (x[:, :8], True, None, None)),
                                        ('affine', lambda x, v: (x, False, v, v)),
                                        ('activation', lambda x, v: (x, False, None, None, 'tanh'))])
def test_training_mode_refuses_planes_its_backward_does_not_cover(what, plane):
    x, v = torch.zeros(4, 16), torch.ones(16)
    for m in _modules():
        m.train()
        with pytest.raises(NotImplementedError, match=what):
            m.fuse_planes([(x, False, None, None), plane(x, v)])
        with pytest.raises(NotImplementedError, match='row_scale'):
            m.fuse_planes([(x, False, None, None)], l2norm_planes=True)


def test_training_mode_takes_fp32_only_and_has_no_cpu_path():
    for m in _modules():
        m.train()
        with pytest.raises(TypeError, match='fp32'):
            m(torch.zeros(4, 2, 16, dtype=torch.float64))
        with pytest.raises(RuntimeError, match='no CPU path'):
            m(torch.zeros(4, 2, 16))


# ---- the C ABI: argument errors need no GPU -----------------------------------------------------------------------------------------
def test_fuse_backward_argument_errors_do_not_need_a_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    n = C.c_size_t(7)
    assert lib.laff_fuse_backward(None, None, None, 1, 1, 1, 4, None, None, None, 0, None, 4, None, None, None, None, None, 0) == -1
    assert b'laff_fuse_backward' in lib.laff_last_error() and b'ctx' in lib.laff_last_error()
    assert lib.laff_fuse_backward_workspace_bytes(4, 16, 2, 64, 3, None) == -1 and b'null out' in lib.laff_last_error()
    assert lib.laff_fuse_backward_workspace_bytes(4, 16, 2, 64, 1 << 7, C.byref(n)) == -1 and b'flags' in lib.laff_last_error()
    for bad in ((0, 16, 2, 64), (9, 16, 2, 64), (4, -1, 2, 64), (4, 16, 0, 64), (4, 16, 2, 6), (4, 16, 2, 0)):
        assert lib.laff_fuse_backward_workspace_bytes(*bad, 3, C.byref(n)) == -2, bad              # LAFF_E_SHAPE
        assert b'laff_fuse_backward_workspace_bytes' in lib.laff_last_error()
    assert n.value == 7                                                                            # untouched by the refusals
    # one partial row of dw per (head, chunk of rows): 4 rows a block while that fills the device, H d floats each
    assert lib.laff_fuse_backward_workspace_bytes(4, 16, 2, 64, 3, C.byref(n)) == 0 and n.value == 4 * 2 * 64 * 4
    assert lib.laff_fuse_backward_workspace_bytes(4, 0, 2, 64, 3, C.byref(n)) == 0 and n.value == 0
    assert lib.laff_fuse_backward_workspace_bytes(4, 16, 2, 64, 16, C.byref(n)) == 0 and n.value == 0     # just-average: no dw
    # the streaming variant (d > 512) keeps a partial row per wavefront
    assert lib.laff_fuse_backward_workspace_bytes(4, 16, 2, 516, 3, C.byref(n)) == 0 and n.value == 4 * 4 * 2 * 516 * 4


def test_ops_fuse_backward_refuses_cpu_tensors_and_planes_it_does_not_cover():
    from laff_amd import ops
    x = torch.zeros(4, 16)
    with pytest.raises(NotImplementedError, match='tiled'):
        ops.fuse_backward([(x, True, None, None)], 2, 8, None, None, None, 0, x)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.fuse_backward([x], 2, 8, torch.zeros(2, 8), torch.zeros(2), None, 0, x)
