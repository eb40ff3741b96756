"""The multi-head self-attention fusion block without a GPU: the restatement of the tests (tests/selfattn_ref.py) against the
reference's own class (tests/golden/selfattn.*.npz), the registry, the state_dict, the refusals and the C ABI's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import selfattn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.fixture_cases()
RESULTS = ('E', 'dx', 'dgamma', 'dbeta', 'dw', 'db', 'weights')


def test_fixture_covers_every_output_type_both_ways():
    seen = {(c['type'], c['l2n'], c['shape']) for _, c in CASES}
    shapes = {c['shape'] for _, c in CASES}
    assert shapes == {(5, 1, 1, 4), (5, 3, 2, 8), (5, 8, 4, 36)}
    assert seen == {(t, l2n, s) for t in R.OUTPUT_TYPES for l2n in (False, True) for s in shapes}


@pytest.mark.parametrize('case', [c for _, c in CASES], ids=[i for i, _ in CASES])
def test_restatement_equals_the_reference_in_float64(case):
    N, L, H, d = case['shape']
    mine = R.run(case['x'], H, d, case['gamma'], case['beta'], case['type'], case['l2n'], case['att1'], case['dE'])
    for k in RESULTS:
        if k not in case:
            continue
        # db is zero but for rounding (a softmax does not see a shift of its logits): held absolutely
        err = float(np.abs(mine[k].numpy() - case[k]).max()) if k == 'db' else R.rel_err(mine[k], case[k])
        assert err < 1e-12, (k, err)


def _opt(heads, output_type='mean', dropout=0.0, l2norm=False):
    from laff_amd.config import config
    opt = config()
    opt.multi_head_attention = {'dropout': dropout, 'heads': heads, 'embed_dim_qkv': 0}
    opt.my_self_attention_output_type = output_type
    opt.attention_l2norm = l2norm
    opt.attention_param_each_head = {'with_ave': True, 'mul': False, 'split_head': True}
    return opt


def test_registry_returns_the_class():
    from laff_amd.model.Attention import Multi_head_MyApply_selfAttention
    from laff_amd.model.model import get_attention_layer
    m = get_attention_layer('my_self_attention', 64, 3, _opt(4, 'last', l2norm=True))
    assert type(m) is Multi_head_MyApply_selfAttention
    assert (m.multi_heads, m.dim_per_head, m.output_type, m.l2norm_each_head, m.dropout_rate) == (4, 16, 'last', True, 0.0)
    with pytest.raises(NotImplementedError, match='ablation variant'):
        get_attention_layer('Attention_MMT', 64, 3, _opt(4))


@pytest.mark.parametrize('case', [c for i, c in CASES if not c['l2n']], ids=[i for i, c in CASES if not c['l2n']])
def test_state_dict_keys_and_shapes_equal_the_fixture(case):
    from laff_amd.model.Attention import Multi_head_MyApply_selfAttention
    N, L, H, d = case['shape']
    m = Multi_head_MyApply_selfAttention(H * d, H, d, 0.0, output_type=case['type'], encoder_num=L, opt=_opt(H))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == case['state_dict']
    if case['type'] == 'Attention_1':
        assert 'Attention_list.0.embedding_common.0.weight' in case['state_dict'] and 'layer_norm.bias' in case['state_dict']
        assert m.get_raw_global_emb_weight() == 1.0
        m.change_raw_global_emb_weight(0.25)
        assert [a.get_raw_global_emb_weight() for a in m.Attention_list] == [0.25] * H
    else:
        assert m.get_raw_global_emb_weight() == 0 and m.change_raw_global_emb_weight(0.5) == 0
        with pytest.raises(Exception, match='SelfAttention weights is not applied'):
            m.get_attention_weight()


def test_refusals_come_by_name_before_any_launch():
    from laff_amd.model.Attention import Multi_head_MyApply_selfAttention as SA
    from laff_amd.model.model import get_attention_layer
    for t in ('cls_embedding', 'concat'):
        with pytest.raises(NotImplementedError, match=t):
            get_attention_layer('my_self_attention', 64, 3, _opt(4, t))
    with pytest.raises(NotImplementedError, match='not provided'):
        SA(64, 4, 16, output_type='no_such_type')
    with pytest.raises(ValueError, match='dim_per_head=4 < multi_heads=8'):
        SA(32, 8, 4)
    x = torch.zeros(3, 2, 64)
    with pytest.raises(NotImplementedError, match="'random'"):
        SA(64, 4, 16, output_type='random').train()(x)
    with pytest.raises(NotImplementedError, match='dropout 0.1'):
        get_attention_layer('my_self_attention', 64, 3, _opt(4, dropout=0.1)).train()(x)
    with pytest.raises(NotImplementedError, match='on the device only'):                           # a CPU model in training
        SA(64, 4, 16).train()(x)
    with pytest.raises(NotImplementedError, match='on the device only'):
        SA(64, 4, 16).train().fuse_planes([x[:, 0], x[:, 1]], 4)
    with pytest.raises(RuntimeError, match='no CPU path'):                                         # ... and in eval
        SA(64, 4, 16).eval()(x)


class _FakeDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda with True: lets the checks that follow the device check run without a device."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def test_ops_refuse_cpu_and_non_fp32_tensors():
    from laff_amd import ops
    from laff_amd.model.Attention import _SelfAttnFn
    x, g, b = [torch.zeros(4, 32)] * 2, torch.ones(8), torch.zeros(8)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.selfattn_fuse(x, 4, 8, g, b, 'mean')
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.selfattn_fuse_backward(x, 4, 8, g, b, 'mean', False, torch.zeros(4, 4, 8))
    with pytest.raises(TypeError, match='float32'):
        ops.selfattn_fuse([_FakeDevice(t.double()) for t in x], 4, 8, g, b, 'mean')
    with pytest.raises(TypeError, match='fp32 only'):
        _SelfAttnFn.apply(4, 8, 'mean', False, g, b, None, *[t.double() for t in x])
    with pytest.raises(NotImplementedError, match='cls_embedding'):
        ops.selfattn_mode('cls_embedding', 2)
    K = __import__('laff_amd._lib', fromlist=['K']).K
    assert ops.selfattn_mode('third', 2) == (K['LAFF_SA_PREPEND_NONE'], K['LAFF_SA_POOL_TOKEN'], 0)
    assert ops.selfattn_mode('third', 3) == (K['LAFF_SA_PREPEND_NONE'], K['LAFF_SA_POOL_TOKEN'], 2)
    assert ops.selfattn_mode('last', 5) == (K['LAFF_SA_PREPEND_NONE'], K['LAFF_SA_POOL_TOKEN'], 4)
    assert ops.selfattn_mode('max_embedding', 5) == (K['LAFF_SA_PREPEND_MAX'], K['LAFF_SA_POOL_TOKEN'], 0)
    assert ops.selfattn_mode('random', 5) == ops.selfattn_mode('mean', 5)


@pytest.mark.parametrize('name', ['laff_selfattn_fuse', 'laff_selfattn_fuse_backward', 'laff_selfattn_fuse_backward_plan'])
def test_entry_point_is_exported_and_bound(name):
    from laff_amd import _lib
    assert name in _lib.SIGNATURES and _lib.ABI_VERSION >= 47
    raw = C.CDLL(_lib.LIB_PATH)
    assert getattr(raw, name) is not None
    assert raw.laff_abi_version() == _lib.ABI_VERSION


def test_plan_and_argument_errors_do_not_need_a_gpu():
    from laff_amd import _lib, ops
    lib = _lib.load()
    K = _lib.K
    # groups of 4 per block up to 4096 blocks; one partial row [dgamma | dbeta] per block
    assert ops.selfattn_fuse_backward_plan(0, 8, 64) == (0, 0)
    assert ops.selfattn_fuse_backward_plan(1, 1, 4) == (1 * 2 * 4 * 4, 1)
    assert ops.selfattn_fuse_backward_plan(67, 1, 36) == (17 * 2 * 36 * 4, 17)
    assert ops.selfattn_fuse_backward_plan(128, 8, 512) == (256 * 2 * 512 * 4, 256)
    assert ops.selfattn_fuse_backward_plan(40000, 8, 512)[1] == 4000                   # 80 groups a block
    out = (C.c_int * 2)(7, 7)
    assert lib.laff_selfattn_fuse_backward_plan(4, 2, 8, None) == -1 and b'null out' in lib.laff_last_error()
    for bad in ((-1, 2, 8), (4, 0, 8), (4, 2, 0), (4, 2, 6), (4, 2, 516), (4, 32, 512), (4, 8, 4)):
        assert lib.laff_selfattn_fuse_backward_plan(*bad, out) == -2, bad                          # LAFF_E_SHAPE
        assert b'laff_selfattn_fuse_backward_plan' in lib.laff_last_error()
    assert b'divides by zero' in lib.laff_last_error()                                             # d = 4 < H = 8, by name
    assert tuple(out) == (7, 7)

    mean, tok, al = K['LAFF_SA_POOL_MEAN'], K['LAFF_SA_POOL_TOKEN'], K['LAFF_SA_POOL_ALL']

    def fwd(ctx, L, N, H, d, prepend=0, pool=mean, token=0, flags=0, lde=None, x=None, ldx=None):
        return lib.laff_selfattn_fuse(ctx, x, ldx, L, N, H, d, None, None, prepend, pool, token, flags, None, H * d if lde is None else lde,
                                      None, 0, 0)

    def bwd(ctx, L, N, H, d, prepend=0, pool=mean, token=0, flags=0):
        return lib.laff_selfattn_fuse_backward(ctx, None, None, L, N, H, d, None, None, prepend, pool, token, flags, None, H * d, None, 0, 0,
                                               None, None, None, None, None, 0)
    for call, fn in ((fwd, b'laff_selfattn_fuse'), (bwd, b'laff_selfattn_fuse_backward')):
        for bad in ((0, 4, 2, 8), (9, 4, 2, 8), (2, -1, 2, 8), (2, 4, 0, 8), (2, 4, 2, 6), (2, 4, 2, 516), (2, 4, 32, 512), (2, 4, 8, 4)):
            assert call(None, *bad) == -2, bad
            assert fn in lib.laff_last_error()
        assert call(None, 2, 4, 2, 8, flags=1) == -1 and b'flags' in lib.laff_last_error()         # WITH_AVE: not a flag of this block
        assert call(None, 2, 4, 2, 8, prepend=3) == -1 and b'prepend' in lib.laff_last_error()
        assert call(None, 2, 4, 2, 8, pool=4) == -1 and b'pool' in lib.laff_last_error()
        assert call(None, 2, 4, 2, 8, pool=tok, token=2) == -1 and b'token' in lib.laff_last_error()
        assert call(None, 2, 4, 2, 8, prepend=1, pool=tok, token=2) == -1 and b'null x' in lib.laff_last_error()   # T = 3: token 2 exists
        assert call(None, 2, 4, 2, 8, prepend=1, pool=al) == -1 and b'no prepended token' in lib.laff_last_error()
        assert call(None, 2, 4, 2, 8) == -1 and b'null x' in lib.laff_last_error()
        assert call(None, 2, 0, 2, 8) == -1 and b'ctx' in lib.laff_last_error()                    # N = 0: nothing but the ctx is looked at
    # pointers, pitches and alignment, still without a device: host arrays of made-up addresses that are never dereferenced
    x, ldx = (C.c_void_p * 2)(4096, 8192), (C.c_int * 2)(16, 16)

    def full(E=4096, lde=16, gamma=4096, ldx=ldx, x=x, pool=mean, O=None, ldon=0, ldol=0):
        return lib.laff_selfattn_fuse(None, x, ldx, 2, 4, 2, 8, C.c_void_p(gamma), C.c_void_p(4096), 0, pool, 0, 4, C.c_void_p(E) if E else None,
                                      lde, C.c_void_p(O) if O else None, ldon, ldol)
    assert full() == -1 and b'ctx' in lib.laff_last_error()                                        # all is well: the NULL ctx comes last
    assert full(ldx=(C.c_int * 2)(16, 12)) == -2 and b'plane 1' in lib.laff_last_error()
    assert full(ldx=(C.c_int * 2)(18, 16)) == -2 and b'plane 0' in lib.laff_last_error()
    assert full(x=(C.c_void_p * 2)(4096, 8196)) == -3 and b'plane 1' in lib.laff_last_error()      # LAFF_E_ALIGN
    assert full(gamma=4100) == -3 and b'gamma' in lib.laff_last_error()
    assert full(E=0) == -1 and b'null E' in lib.laff_last_error()
    assert full(lde=12) == -2 and b'lde' in lib.laff_last_error()
    assert full(E=4100) == -3
    assert full(pool=al, E=0) == -1 and b'null O' in lib.laff_last_error()
    assert full(pool=al, E=0, O=4096, ldon=32, ldol=16) == -1 and b'ctx' in lib.laff_last_error()
    assert full(pool=al, E=0, O=4096, ldon=16, ldol=64) == -1 and b'ctx' in lib.laff_last_error()  # plane-major
    assert full(pool=al, E=0, O=4096, ldon=16, ldol=16) == -2 and b'overlap' in lib.laff_last_error()
    assert full(pool=al, E=0, O=4096, ldon=34, ldol=16) == -3


# ---- the model cases of the fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['sa_mean', 'sa_att1'])
def test_tower_restatement_and_optimizer_replay_reproduce_the_model_fixture(key):
    """tests/tower_ref.py with the fusion of tests/selfattn_tower.py reproduces both steps of the reference's float64 run to 1e-12
    (embeddings, loss, gradients, running statistics, every hinge decision HINGE_CLEAR from flipping), tests/optim_ref.py its
    parameters and RMSprop state."""
    import selfattn_tower
    import tower_ref
    arrays, meta = tower_ref.load_case(key)
    assert meta['attention'] == 'my_self_attention' and meta['output_type'] == selfattn_tower.CASES[key] and meta['model'] == 'LAFF'
    assert (meta['loss'], meta['optimizer'], meta['max_violation'], meta['direction']) == ('mrl', 'rmsprop', True, 't2i')
    tower_ref.check_restatement(arrays, meta)
    tower_ref.check_replay(arrays, meta)
    cfg = tower_ref.make_cfg(meta)
    assert cfg.vis_attention == cfg.txt_attention == 'my_self_attention' and cfg.my_self_attention_output_type == meta['output_type']
    # the cases the harness had before are built as before
    _, meta_a = tower_ref.load_case('a')
    assert tower_ref.make_cfg(meta_a).vis_attention == 'Multi_head_MyApply_Attention'
