"""Host checks of the tiled training-mode BatchNorm1d: the ABI and the three symbols, the plan, the refusals of the C
entry points (which need no GPU) and of the ops, and TransformNet's no-transform training path: opt-in through device_norm, every
refusal by its name."""
import ctypes as C

import pytest
import torch


def test_header_binding_and_library_agree_on_the_abi_and_the_new_symbols():
    from laff_amd import build, ops
    assert 'tile_bn_train.hip' in build.SOURCES and 'bn_train.hip' in build.SOURCES
    assert any(h.endswith('bn_train_common.h') for h in build.HEADERS)            # a change of the shared arithmetic rebuilds both
    for name in ('tile_bn_train', 'tile_bn_train_backward', 'tile_bn_train_plan'):
        assert callable(getattr(ops, name)) and name in ops.__all__


def test_plan_names_the_shapes_that_are_cut():
    from laff_amd import ops
    chunks, nbytes, launches, rows = ops.tile_bn_train_plan(128, 512, 8)
    assert (chunks, nbytes, launches) == (1, 0, 1) and rows == 256                       # the training batch: one launch, no workspace
    assert ops.tile_bn_train_plan(rows, 512, 8)[:3] == (1, 0, 1)
    assert ops.tile_bn_train_plan(rows + 1, 36, 2)[:3] == (2, 2 * 2 * 2 * 36 * 8, 2)      # the backward's partials: per channel H C
    assert ops.tile_bn_train_plan(512, 512, 8)[:3] == (2, 2 * 2 * 8 * 512 * 8, 2)
    assert ops.tile_bn_train_plan(300, 64, 1)[:3] == ops.dropout_bn_train_plan(300, 64)[:3]
    assert ops.tile_bn_train_plan(0, 5, 1)[:3] == (1, 0, 1)


def test_refusals_need_no_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    E_ARG, E_SHAPE = -1, -2
    vec = (C.c_float * 16)()
    g = C.cast(vec, C.c_void_p)

    def fwd(N=4, Cw=8, H=2, gamma=g, momentum=0.1, eps=1e-5):
        rc = lib.laff_tile_bn_train(None, None, N, Cw, Cw, H, gamma, g, g, g, momentum, eps, None, H * Cw, g, g, None, 0)
        return rc, lib.laff_last_error().decode()

    def bwd(N=4, Cw=8, H=2, gamma=g):
        rc = lib.laff_tile_bn_train_backward(None, None, H * Cw, None, N, Cw, Cw, H, gamma, g, g, None, Cw, None, None, None, 0)
        return rc, lib.laff_last_error().decode()

    for call in (fwd, bwd):
        for kw, code, text in ((dict(H=0), E_SHAPE, 'H>=1'), (dict(Cw=0), E_SHAPE, 'C>=1'), (dict(N=-1), E_SHAPE, 'N>=0'),
                               (dict(H=-3, N=1), E_SHAPE, 'H>=1'),                        # the shape is looked at before the batch
                               (dict(N=1), E_ARG, 'N >= 2'), (dict(N=0), E_ARG, 'N >= 2'), (dict(gamma=None), E_ARG, 'null gamma')):
            rc, msg = call(**kw)
            assert rc == code and text in msg, (call.__name__, kw, rc, msg)
        rc, msg = call()                                   # everything in order: the null ctx is what is left to refuse
        assert rc == E_ARG and 'null ctx' in msg, (call.__name__, rc, msg)
    for kw, text in ((dict(eps=0.0), 'eps'), (dict(eps=-1e-5), 'eps'), (dict(momentum=-0.1), 'momentum'), (dict(momentum=1.5), 'momentum'),
                     (dict(momentum=float('nan')), 'momentum')):
        rc, msg = fwd(**kw)
        assert rc == E_ARG and text in msg, (kw, rc, msg)
    assert 'null ctx' in fwd(momentum=0.0)[1] and 'null ctx' in fwd(momentum=1.0)[1]
    out = (C.c_int * 4)()
    assert lib.laff_tile_bn_train_plan(4, 0, 1, out) == E_SHAPE and lib.laff_tile_bn_train_plan(4, 8, 0, out) == E_SHAPE
    assert lib.laff_tile_bn_train_plan(4, 8, 1, None) == E_ARG


def test_ops_refuse_host_and_non_fp32_tensors():
    from laff_amd import ops
    x, v = torch.randn(4, 8), torch.ones(16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.tile_bn_train(x, 2, v, v, v, v, 0.1, 1e-5)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.tile_bn_train_backward(torch.randn(4, 16), x, 2, v, v[:8], v[:8])


def test_no_transform_training_path_is_opt_in_and_refuses_by_name():
    from laff_amd.model import model
    x = torch.randn(4, 8)
    net = model.TransformNet((8, 16), batch_norm=True, activation=False, fc=False).train()
    assert net.device_norm is False
    # without device_norm: today's refusal, word for word
    with pytest.raises(NotImplementedError) as e:
        net.plane(x, heads=2)
    assert str(e.value) == ('training mode: a TransformNet without fc (fc=False, tiled over 2 heads) has no differentiable path; apply '
                            'its BatchNorm upstream as a torch op')
    with pytest.raises(NotImplementedError, match=r'without fc \(fc=False\) has no differentiable path'):
        net(torch.randn(4, 16))
    # with it: the launch is reached, and there is no CPU path -- both widths
    model.use_device_norm(net)
    with pytest.raises(RuntimeError, match='no CPU path'):
        net.plane(x, heads=2)
    with pytest.raises(RuntimeError, match='no CPU path'):
        net(torch.randn(4, 16))
    assert int(net.bn1.num_batches_tracked) == 0                                   # a refused forward counts nothing
    with pytest.raises(NotImplementedError, match='extra_shift'):
        net.plane(x, heads=2, extra_shift=torch.zeros(16))
    with pytest.raises(ValueError, match='got 6 columns'):
        net.plane(torch.randn(4, 6), heads=2)
    with pytest.raises(TypeError, match='fp32 only'):
        net.plane(x.double(), heads=2)
    for field, value, text in (('momentum', None, 'momentum=None'), ('affine', False, 'affine=False'),
                               ('track_running_stats', False, 'track_running_stats=False')):
        bad = model.TransformNet((8, 16), batch_norm=True, activation=False, fc=False, device_norm=True).train()
        setattr(bad.bn1, field, value)
        with pytest.raises(NotImplementedError, match=text):
            bad.plane(x, heads=2)
    # dropout on a tiled layer: the mask would differ per copy
    drop = model.TransformNet((8, 16), dropout=0.2, batch_norm=True, activation=False, fc=False, device_norm=True).train()
    with pytest.raises(NotImplementedError, match=r'dropout \(p=0.2\).*tiled over 2 heads'):
        drop.plane(x, heads=2)
    with pytest.raises(RuntimeError, match='no CPU path'):                          # its own width: the existing kernel takes the rate
        drop(torch.randn(4, 16))
    with pytest.raises(NotImplementedError, match='without BatchNorm is a plain repeat'):
        model.TransformNet((8, 16), batch_norm=False, activation=False, fc=False, device_norm=True).train().plane(x, heads=2)
    with pytest.raises(NotImplementedError, match='activation without fc'):
        model.TransformNet((8, 16), batch_norm=True, activation='tanh', fc=False, device_norm=True).train().plane(x, heads=2)
