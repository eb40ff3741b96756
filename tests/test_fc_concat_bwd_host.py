"""What laff_fc_concat_backward and the W2VV++ training route promise without a GPU: the symbols and the ABI, the
refusals by name with the NULL ctx looked at last, the plan as a pure function of the shapes, and the refusals of the towers and of
the training step."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -3


def test_header_library_and_binding_agree_on_the_new_symbols_and_the_abi():
    from laff_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (('laff_fc_concat_backward', 27), ('laff_fc_concat_backward_plan', 7)):
        assert re.search(r'^int %s\(' % name, header, flags=re.M)
        assert hasattr(raw, name) and name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    abi = re.findall(r'^#define LAFF_ABI_VERSION (\d+)$', header, flags=re.M)
    assert len(abi) == 1 and raw.laff_abi_version() == _lib.ABI_VERSION == int(abi[0]) >= 46
    assert 'fc_concat_bwd.hip' in __import__('laff_amd.build', fromlist=['SOURCES']).SOURCES
    assert 'fc_concat_backward' in ops.__all__ and 'fc_concat_backward_plan' in ops.__all__
    # the header is the only declaration: the binding names neither symbol
    assert 'fc_concat_backward' not in open(os.path.join(ROOT, 'laff_amd', '_lib.py')).read()


PTR = 4096                             # a pointer that is never followed: every refusal comes before any GPU work


def _call(spec, nseg=None, N=8, K=16, D=8, lddw=None, ws=None, ws_bytes=0, ctx=None, dW=PTR):
    """spec: (csr, Dk, col, wants dX) per segment, with made-up pointers."""
    from laff_amd import _lib
    lib = _lib.load()
    n = max(len(spec), 1)
    ints = lambda f: (ctypes.c_int * n)(*[f(*g) for g in spec])                               # noqa: E731
    ptrs = lambda f: (ctypes.c_void_p * n)(*[f(*g) for g in spec])                            # noqa: E731
    rc = lib.laff_fc_concat_backward(
        ctx, len(spec) if nseg is None else nseg, ints(lambda c, dk, col, dx: dk), ints(lambda c, dk, col, dx: col),
        ints(lambda c, dk, col, dx: 5 if c else -1), ptrs(lambda c, dk, col, dx: None if c else PTR), ints(lambda c, dk, col, dx: dk),
        ptrs(lambda c, dk, col, dx: PTR if dx else None), ints(lambda c, dk, col, dx: dk), ptrs(lambda c, dk, col, dx: PTR if c else None),
        ptrs(lambda c, dk, col, dx: PTR if c else None), ptrs(lambda c, dk, col, dx: None), N, PTR, K, K, D, 1, PTR, D, PTR, D, dW,
        K if lddw is None else lddw, PTR, ws, ws_bytes)
    return rc, lib.laff_last_error().decode()


def test_refusals_come_back_by_name_without_a_gpu_and_the_null_ctx_last():
    two = [(False, 8, 0, False), (False, 8, 8, False)]
    rc, msg = _call([], nseg=0)
    assert rc == E_ARG and 'nseg' in msg and 'laff_fc_concat_backward' in msg
    rc, msg = _call(two * 4 + two[:1], nseg=9)
    assert rc == E_ARG and 'nseg=9' in msg
    rc, msg = _call([(False, 8, 0, False), (False, 8, 7, False)])
    assert rc == E_SHAPE and 'overlap' in msg
    rc, msg = _call([(False, 8, 0, False), (False, 8, 9, False)])
    assert rc == E_SHAPE and "outside W's K=16" in msg
    rc, msg = _call(two, D=6)
    assert rc == E_SHAPE and 'D=6' in msg
    assert _call(two, D=8196)[0] == E_SHAPE and _call(two, D=0)[0] == E_SHAPE
    rc, msg = _call(two, lddw=15)
    assert rc == E_SHAPE and 'lddw=15 < K=16' in msg
    rc, msg = _call([(False, 8, 0, False), (True, 8, 8, True)])
    assert rc == E_ARG and 'CSR segment has no dX' in msg
    # a short workspace: N = 130 cuts the sum over N, the plan asks for bytes
    from laff_amd import ops
    chunks, nbytes, _, _ = ops.fc_concat_backward_plan(130, 8, [8, 8])
    assert chunks > 1 and nbytes > 0
    rc, msg = _call(two, N=130, ws=PTR, ws_bytes=nbytes - 4)
    assert rc == E_ARG and 'workspace too small' in msg
    rc, msg = _call(two, N=130, ws=None, ws_bytes=nbytes)
    assert rc == E_ARG and 'workspace' in msg
    # everything in order: only now the NULL ctx
    rc, msg = _call(two, N=130, ws=PTR, ws_bytes=nbytes)
    assert rc == E_ARG and 'null ctx' in msg
    rc, msg = _call(two)
    assert rc == E_ARG and 'null ctx' in msg
    rc, msg = _call([(False, 4, 0, False), (True, 4, 4, False)], N=0, K=8)
    assert rc == E_ARG and 'null ctx' in msg


def test_the_plan_is_a_pure_function_of_the_shapes():
    from laff_amd import ops
    # one chunk of the sum over N up to N = 128, whatever the widths
    for widths in ([36, 30], [5, 130, 64, 3], [2048, 2048], [500, 2048]):
        for N in (1, 33, 128):
            assert ops.fc_concat_backward_plan(N, 2048, widths)[0] == 1
            assert ops.fc_concat_backward_plan(N, 64, widths, want_dx=[False] * len(widths))[:2] == (1, 0)
    assert ops.fc_concat_backward_plan(130, 68, [64, 68], [True, False]) == ops.fc_concat_backward_plan(130, 68, [64, 68], [True, False])
    # the cuts do not depend on what is asked for, only the bytes do
    a = ops.fc_concat_backward_plan(130, 260, [64, 68], [True, True])
    b = ops.fc_concat_backward_plan(130, 260, [64, 68], [False, False], want_dw=False)
    assert (a[0], a[2], a[3]) == (b[0], b[2], b[3]) and a[0] > 1 and a[2] > 1 and a[1] > b[1] > 0
    # a CSR segment takes no part in the dense launches' plan
    colptr = torch.zeros(51, dtype=torch.int32)
    csc = (colptr, torch.zeros(0, dtype=torch.int32), None)
    assert ops.fc_concat_backward_plan(130, 68, [64, csc, 68], [True, False, False]) == ops.fc_concat_backward_plan(130, 68, [64, 68], [True, False])
    assert ops.fc_concat_backward_plan(9, 16, [csc, csc]) == (1, 0, 1, 0)
    with pytest.raises(ValueError, match='no dx'):
        ops.fc_concat_backward_plan(9, 16, [csc, 4], [True, False])
    with pytest.raises(RuntimeError, match='nseg'):
        ops.fc_concat_backward_plan(9, 16, [])
    with pytest.raises(RuntimeError, match='D=6'):
        ops.fc_concat_backward_plan(9, 6, [4])


# ---- the fixture of the reference's own steps (tools/gen_golden_train.py) -----------------------------------------------------------
@pytest.mark.parametrize('key', ['i', 'ii'])
def test_concat_tower_ref_reproduces_the_reference_in_float64(key):
    """Embeddings, loss and every gradient of both steps to 1e-12."""
    import tower_ref
    arrays, meta = tower_ref.load_case(key)
    assert meta['model'] == {'i': 'W2VVPP', 'ii': 'w2vpp_mutivis_attention'}[key] and meta['N'] == 12 and meta['D'] == 64
    assert list(meta['vid_dims'].values()) == [96, 48, 40] and list(meta['txt_dims'].values()) == [30, 50, 64]
    assert (meta['optimizer'], meta['max_violation'], meta['direction']) == {'i': ('rmsprop', True, 't2i'), 'ii': ('adam', False, 'bidir')}[key]
    assert tower_ref.REL == 1e-12 and all(rec['none'] == [] for rec in meta['steps'])     # every parameter has a gradient
    tower_ref.check_restatement(arrays, meta)


def test_optim_ref_reproduces_the_reference_optimizers_and_adam_only_with_the_default_eps():
    import tower_ref
    for key in ('i', 'ii'):
        tower_ref.check_replay(*tower_ref.load_case(key))
    arrays, meta = tower_ref.load_case('ii')
    assert meta['eps'] == 1e-8 and meta['betas'] == [0.9, 0.999]
    assert max(tower_ref.replay_steps(arrays, meta, eps=1e-4).values()) > 1e-6      # the multi-head class's eps is not what the base class steps with


# ---- the towers and the step -------------------------------------------------------------------------------------------------------
def _cfg(model='W2VVPP', txt='concat', vis='concat', **kw):
    from laff_amd.config import make_config
    return make_config({'a': 8, 'b': 4}, {'bow': 5, 'w2v': 6}, 32, 1, model, txt_attention=txt, vis_attention=vis, **kw)


def test_step_refusals_are_raised_by_name_before_any_launch():
    from laff_amd.model import model as M
    with pytest.raises(NotImplementedError, match='the concat towers train on the device only'):
        M.get_model('W2VVPP', 'cpu', _cfg()).enable_training()
    with pytest.raises(NotImplementedError, match='the concat towers train on the device only'):
        M.get_model('w2vpp_mutivis_attention', 'cpu', _cfg('w2vpp_mutivis_attention')).enable_training()
    with pytest.raises(NotImplementedError, match=r"key 'LAFF' with the concat towers.*criterion_with_score"):
        M.get_model('LAFF', 'cpu', _cfg('LAFF')).enable_training()
    for txt, vis in (('concat', 'Multi_head_MyApply_Attention'), ('Multi_head_MyApply_Attention', 'concat')):
        for key in ('w2vpp_mutivis_attention', 'LAFF'):
            with pytest.raises(NotImplementedError, match='rank mismatch'):
                M.get_model(key, 'cpu', _cfg(key, txt, vis)).enable_training()
    for field, value, text in (('negative', True, 'opt.negative'), ('multi_space', False, 'multi_space=False')):
        bad = M.get_model('W2VVPP', 'cpu', _cfg(**{field: value}))
        with pytest.raises(NotImplementedError, match=text):
            bad.enable_training()
        assert getattr(bad, 'optimizer', None) is None and not getattr(bad.vis_net, 'training_armed', False)
    m = M.get_model('W2VVPP', 'cpu', _cfg())                               # (get_model sets the module's float16 from the config)
    keep = M.float16
    try:
        M.float16 = True
        with pytest.raises(NotImplementedError, match='the step is fp32'):
            m.enable_training()
    finally:
        M.float16 = keep


def test_an_unarmed_tower_keeps_the_inference_only_refusal():
    from laff_amd.model import model as M
    m = M.get_model('W2VVPP', 'cpu', _cfg()).train()
    assert not getattr(m.vis_net, 'training_armed', False) and not getattr(m.txt_net, 'training_armed', False)
    with pytest.raises(NotImplementedError, match='inference path only'):
        m.vis_net({'a': torch.zeros(2, 8), 'b': torch.zeros(2, 4)})
    with pytest.raises(NotImplementedError, match='inference path only'):
        m.txt_net({'bow_encoding': torch.zeros(2, 5), 'w2v_encoding': torch.zeros(2, 6)})
    with pytest.raises(NotImplementedError, match='inference path only'):
        m.vis_net.concat_problem([torch.zeros(2, 12)])
    # an armed tower on the CPU is refused by name too: the route runs on the device only
    m.vis_net.training_armed = True
    with pytest.raises(NotImplementedError, match='train on the device only'):
        m.vis_net({'a': torch.zeros(2, 8), 'b': torch.zeros(2, 4)})


def test_optimizer_for_keeps_its_eps_and_takes_another():
    from laff_amd import optim
    from laff_amd.model import model as M
    cfg = _cfg(optimizer='adam')
    m = M.get_model('W2VVPP', 'cpu', cfg)
    assert optim.optimizer_for(cfg, m)[0].param_groups[0]['eps'] == 1e-4
    assert optim.optimizer_for(cfg, m, adam_eps=1e-8)[0].param_groups[0]['eps'] == 1e-8
