"""Host checks of the training step and the expert stage, none of which needs a GPU: the float64 restatement
(tests/tower_ref.py) against the training-step fixture of the reference, tests/optim_ref.py against the reference's own RMSprop steps,
tests/expert_stage_ref.py against torch autograd, the ABI and the three symbols, and every refusal of the C entry points and of the
model by its message."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import expert_stage_ref
import tower_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rel_err = tower_ref.rel_err


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_restatement_reproduces_the_fixture_in_float64(key):
    tower_ref.check_restatement(*tower_ref.load_case(key))


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_optim_ref_reproduces_the_reference_steps(key):
    """RMSprop(lr, alpha 0.99, eps 1e-8) behind clip_grad_norm_(grad_clip) on the fixture's raw float64 gradients gives the fixture's
    float64 parameters and square_avg after both steps: clip coefficient, eps, alpha and the learning rate are the reference's."""
    arrays, meta = tower_ref.load_case(key)
    assert (meta['optimizer'], meta['alpha'], meta['eps']) == ('rmsprop', 0.99, 1e-8)
    tower_ref.check_replay(arrays, meta)


@pytest.mark.parametrize('expert,l2norm', [(True, False), (False, True), (True, True)])
def test_expert_stage_ref_against_autograd(expert, l2norm):
    g = torch.Generator().manual_seed(5)
    N, L, D = 7, 3, 20
    xs = [torch.randn(N, D, generator=g, dtype=torch.float64, requires_grad=True) for _ in range(L)]
    e = torch.randn(L, D, generator=g, dtype=torch.float64, requires_grad=True) if expert else None
    dY = torch.randn(N, L, D, generator=g, dtype=torch.float64)
    v = torch.stack(xs, 1) + (e[None] if expert else 0)
    Y = v / (v.pow(2).sum(2, keepdim=True).sqrt() + 1e-13 + 1e-14) if l2norm else v
    Y.backward(dY)
    np_xs, np_e = [x.detach().numpy() for x in xs], e.detach().numpy() if expert else None
    Y64, r = expert_stage_ref.forward(np_xs, np_e, l2norm)
    dx, de, mag = expert_stage_ref.backward(np_xs, np_e, l2norm, dY.numpy())
    assert rel_err(Y64, Y.detach()) <= 1e-14 and (r is None) == (not l2norm)
    for l in range(L):
        assert rel_err(dx[:, l], xs[l].grad) <= 1e-13
    if expert:
        assert rel_err(de, e.grad) <= 1e-13
    assert np.all(np.abs(dx) <= mag * (1 + 1e-12))
    # a row of zeros: finite, Y = 0 there, the second term is dropped
    if l2norm and not expert:
        np_xs[1][2] = 0.0
        Y0, _ = expert_stage_ref.forward(np_xs, None, True)
        dx0 = expert_stage_ref.backward(np_xs, None, True, dY.numpy())[0]
        assert not Y0[2, 1].any() and np.isfinite(dx0).all()
        assert np.allclose(dx0[2, 1], dY.numpy()[2, 1] / (1e-13 + 1e-14), rtol=1e-12)


def test_header_binding_and_library_agree_on_the_abi_and_the_new_symbols():
    from laff_amd import build, ops
    assert 'expert_train.hip' in build.SOURCES
    for name in ('expert_stage_train', 'expert_stage_train_backward', 'expert_stage_train_plan'):
        assert callable(getattr(ops, name)) and name in ops.__all__
    from laff_amd.model import autograd, model
    assert model._ExpertStageFn is autograd._ExpertStageFn


def test_plan_counts_blocks_by_rows_alone():
    from laff_amd import ops
    assert ops.expert_stage_train_plan(0, 3, 36) == (0, 0)
    assert ops.expert_stage_train_plan(1, 1, 4) == (1, 16)
    assert ops.expert_stage_train_plan(16, 8, 512) == (1, 8 * 512 * 4)
    assert ops.expert_stage_train_plan(17, 8, 512) == (2, 2 * 8 * 512 * 4)
    assert ops.expert_stage_train_plan(128, 4, 4096) == (8, 8 * 4 * 4096 * 4)


def test_c_refusals_need_no_gpu():
    from laff_amd import _lib
    lib = _lib.load()
    E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3
    header = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    codes = dict(re.findall(r'(LAFF_E_\w+)\s*=\s*(-?\d+)', header))
    assert (int(codes['LAFF_E_ARG']), int(codes['LAFF_E_SHAPE']), int(codes['LAFF_E_ALIGN'])) == (E_ARG, E_SHAPE, E_ALIGN)
    A = 0x10000                                            # an address that is never read: every refusal comes before any GPU work

    def arrays(L, base, ld):
        return (C.c_void_p * 8)(*[base + 0x1000 * l for l in range(8)]), (C.c_int * 8)(*[ld] * 8)

    def fwd(N=4, L=3, D=8, xbase=A, ldx=8, expert=A, lde=8, l2norm=1, Y=A, ldn=24, ldl=8, rnorm=A, x_null=False):
        xs, lds = arrays(L, xbase, ldx)
        rc = lib.laff_expert_stage_train(None, None if x_null else xs, lds, N, L, D, expert, lde, l2norm, Y, ldn, ldl, rnorm)
        return rc, lib.laff_last_error().decode()

    def bwd(N=4, L=3, D=8, xbase=A, ldx=8, expert=A, lde=8, l2norm=1, Y=A, ldn=24, ldl=8, rnorm=A, x_null=False, dxbase=A, lddx=8,
            d_expert=A, ws=A, ws_bytes=1 << 20):
        xs, lds = arrays(L, xbase, ldx)
        dxs, ldds = arrays(L, dxbase, lddx)
        rc = lib.laff_expert_stage_train_backward(None, Y, ldn, ldl, None if x_null else xs, lds, N, L, D, expert, lde, l2norm, rnorm, dxs,
                                                  ldds, d_expert, ws, ws_bytes)
        return rc, lib.laff_last_error().decode()

    shared = ((dict(L=0), E_SHAPE, '1 <= L <= 8'), (dict(L=9), E_SHAPE, '1 <= L <= 8'), (dict(D=6, ldn=24), E_SHAPE, 'D % 4 == 0'),
              (dict(D=0), E_SHAPE, 'D % 4 == 0'), (dict(D=8196, ldx=8196, lde=8196, ldl=8196, ldn=3 * 8196), E_SHAPE, 'D <= 8192'),
              (dict(N=-1), E_SHAPE, 'N >= 0'),
              (dict(expert=None, l2norm=0), E_ARG, 'plain copy'), (dict(x_null=True), E_ARG, 'null x'), (dict(Y=None), E_ARG, 'null x'),
              (dict(rnorm=None), E_ARG, 'l2norm needs rnorm'),
              (dict(ldx=4), E_SHAPE, 'row pitch of x[0] is below D'), (dict(ldx=10), E_ALIGN, 'rows of x[0] must be 16-byte aligned'),
              (dict(xbase=A + 4), E_ALIGN, 'rows of x[0] must be 16-byte aligned'),
              (dict(lde=4), E_SHAPE, 'row pitch of expert is below D'), (dict(lde=9), E_ALIGN, 'rows of expert'),
              (dict(expert=A + 8), E_ALIGN, 'rows of expert'),
              (dict(ldl=4), E_SHAPE, 'without overlap'), (dict(ldn=16), E_SHAPE, 'without overlap'),
              (dict(ldn=26, ldl=8), E_ALIGN, 'row pitch 26'), (dict(Y=A + 4), E_ALIGN, 'must be 16-byte aligned'),
              (dict(rnorm=A + 2), E_ALIGN, 'rnorm must be 4-byte aligned'))
    for call in (fwd, bwd):
        for kw, code, text in shared:
            rc, msg = call(**kw)
            assert rc == code and text in msg, (call.__name__, kw, rc, msg)
        for kw in (dict(), dict(expert=None), dict(l2norm=0, rnorm=None), dict(ldn=8, ldl=32), dict(N=0)):       # plane-major is a layout too
            if call is bwd and kw.get('expert', A) is None:
                kw = dict(kw, d_expert=None)
            rc, msg = call(**kw)
            assert rc == E_ARG and 'null ctx' in msg, (call.__name__, kw, rc, msg)
    for kw, code, text in ((dict(lddx=4), E_SHAPE, 'row pitch of dx[0] is below D'), (dict(lddx=9), E_ALIGN, 'rows of dx[0]'),
                           (dict(dxbase=A + 4), E_ALIGN, 'rows of dx[0]'), (dict(expert=None), E_ARG, 'd_expert without an expert table'),
                           (dict(d_expert=A + 4), E_ALIGN, 'd_expert must be 16-byte aligned'),
                           (dict(ws_bytes=3 * 8 * 4 - 1), E_ARG, 'workspace too small'), (dict(ws=None), E_ARG, 'workspace too small'),
                           (dict(ws=A + 4), E_ALIGN, 'workspace must be 16-byte aligned')):
        rc, msg = bwd(**kw)
        assert rc == code and text in msg, (kw, rc, msg)
    assert 'null ctx' in bwd(d_expert=None, ws=None, ws_bytes=0)[1]              # no d_expert: no workspace
    out = (C.c_int * 2)()
    assert lib.laff_expert_stage_train_plan(4, 0, 8, out) == E_SHAPE and lib.laff_expert_stage_train_plan(4, 3, 10, out) == E_SHAPE
    assert lib.laff_expert_stage_train_plan(4, 3, 8, None) == E_ARG


def test_ops_and_function_refuse_host_and_non_fp32_tensors():
    from laff_amd import ops
    from laff_amd.model.autograd import _ExpertStageFn
    xs = [torch.randn(4, 8) for _ in range(2)]
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.expert_stage_train(xs, torch.randn(2, 8), True)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.expert_stage_train_backward(torch.randn(4, 2, 8), xs, None, True, torch.randn(2, 4), want_d_expert=False)
    with pytest.raises(TypeError, match='fp32 only'):
        _ExpertStageFn.apply(True, None, xs[0].double(), xs[1].double())


def _model(key='a', **overrides):
    return tower_ref.device_model(key, 'cpu', **overrides)


def test_model_refusals_come_before_any_launch():
    from laff_amd.config import make_config
    from laff_amd.model import model as M
    m = _model()
    with pytest.raises(NotImplementedError, match=r'built for inference; call enable_training\(\) first'):
        m({'vis_feats': {}, 'captions': {}})
    for field, value, text in (('negative', True, 'opt.negative'), ('multi_space', False, 'multi_space=False')):
        bad = _model(**{field: value})
        with pytest.raises(NotImplementedError, match=text):
            bad.enable_training()
        with pytest.raises(NotImplementedError, match=text):
            bad({'vis_feats': {}, 'captions': {}})
        assert getattr(bad, 'optimizer', None) is None
    cfg = make_config({'a': 8}, {'bow': 5}, 32, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat')
    with pytest.raises(NotImplementedError, match='concat towers'):
        M.get_model('W2VVPP', 'cpu', cfg).enable_training()
    # the FrameLAFF tower's route opens for the model that armed it only: a tower on its own keeps the inference-only refusal
    cfg = make_config({}, {'bow': 8}, 64, 2, 'FrameLAFF', frame_feats={'clip_frame': 16}, batch_norm=False,
                      vis_frame_attention='attention_noAveNoAverageMul', frame_feat_with_video_feat=False)
    frame = M.get_model('FrameLAFF', 'cpu', cfg).train()
    frames = {'clip_frame': torch.zeros(2, 3, 16), 'mask_tensor': torch.ones(2, 3)}
    with pytest.raises(NotImplementedError, match='inference path only'):
        frame.vis_net.prepare({}, dict(frames))
    frame.enable_training()
    assert frame.vis_net.training_armed
    with pytest.raises(NotImplementedError, match='train on the device only'):
        frame.vis_net.prepare({}, dict(frames))
    keep = M.float16
    try:
        M.float16 = True
        with pytest.raises(NotImplementedError, match='the step is fp32'):
            m.enable_training()
    finally:
        M.float16 = keep


def test_enable_training_builds_the_reference_names_and_allocates_nothing_before():
    from laff_amd import loss, optim
    from laff_amd.model.model import TransformNet
    m = _model('b')
    for name in ('criterion', 'criterion_with_score', 'optimizer', 'lr_schedulers', 'params', 'iters'):
        assert not hasattr(m, name), name
    assert m.enable_training() is m
    assert isinstance(m.criterion, loss.MarginRankingLoss) and (m.criterion.max_violation, m.criterion.direction, m.criterion.margin) == \
        (False, 'bidir', 0.2)
    assert isinstance(m.criterion_with_score, loss.MarginRankingLossWithScore)
    assert isinstance(m.optimizer, optim.RMSprop) and m.optimizer.grad_clip == 2.0 and m.grad_clip == 2 and m.iters == 0
    assert m.learning_rate == [1e-4, 1e-4 / 20] and len(m.lr_schedulers) == 2
    assert len(m.params) == len(list(m.parameters()))
    assert all(t.device_norm for t in m.modules() if isinstance(t, TransformNet))
    m.eval()
    with pytest.raises(RuntimeError, match='eval mode'):
        m({'vis_feats': {}, 'captions': {}})
    assert m.iters == 0
    m.lr_step(0.5)
    assert abs(m.learning_rate[0] - 0.99e-4) < 1e-12
    plain = _model('a').enable_training(device_norm=False)
    assert not any(t.device_norm for t in plain.modules() if isinstance(t, TransformNet))


def test_towers_in_training_mode_want_the_device_and_direct_callers_stay_refused():
    """The towers' prepare no longer refuses training mode as such: a model on the CPU is refused because the routes run on the device
    only.  Direct callers of TransformNet / fuse_planes keep the two refusals of the expert stage."""
    from laff_amd.model.model import TransformNet
    for key in ('a', 'd'):
        m = _model(key).enable_training()
        data = tower_ref.train_data(key, 1, 'cpu')
        with pytest.raises(NotImplementedError, match='train on the device only'):
            m.txt_net(data['captions'])
        with pytest.raises(NotImplementedError, match='train on the device only'):
            m.vis_net(data['vis_feats'])
    m = _model('d')
    with pytest.raises(NotImplementedError, match='the backward of the fusion has no row_scale'):
        m.vis_net.attention_layer.fuse_planes([torch.zeros(2, 512)], 4, l2norm_planes=True)
    with pytest.raises(NotImplementedError, match='extra_shift .the expert embedding. is not differentiable here'):
        TransformNet((8, 16), batch_norm=False, activation='tanh', dropout=0.0).train().plane(torch.zeros(2, 8), extra_shift=torch.zeros(16))
