"""The 'LAFF' model's training step on the MI355X against the training-step fixture of the reference
(tests/golden/train_step.<case>.<n>.npz: two RMSprop steps of the reference in float64 and float32, tools/gen_golden_train.py).

Rules, all of tests/train_ref.py, constants unchanged:
    embeddings, loss     max |device - float64| <= max(4 e32, TOL_UNIT) max |float64|, e32 the fixture's recorded error of the
                         reference's own float32 run for that tensor
    raw gradients        element by element under end_to_end_bound: max(4 e32, TOL_UNIT) max |r64| + GRAD_ABS sum_j |d r / d E_j|, the
                         absolute Jacobian from the float64 restatement tests/tower_ref.py (once per session)
    total norm           | |g| - |g64| | <= |g - g64| <= sqrt(sum of the squared element bounds), plus TOL_UNIT |g64| for the sum itself
    the step             parameters and square_avg against tests/optim_ref.py applied to this model's OWN device gradients, under the
                         bounds of tests/test_gpu_optim.py -- no element-wise comparison of stepped parameters with the fixture:
                         RMSprop's first update is +-10 lr whatever |g|, so an element whose gradient lies inside its bound may take
                         the other sign (tests/test_train_step_host.py ties the optimizer to the reference instead)
    running statistics   max(4 e32, TOL_UNIT) as the dropout-BN test, e32 from the restatement in float32
The embedding_common.0.bias gradients are exact zeros here and rounding noise in the reference (softmax ignores a shift): they are
asserted to be zero and left out of every comparison with the reference.
"""
import functools

import numpy as np
import pytest
import torch

import fuse_bwd_ref
import optim_ref
import tower_ref
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BIAS = 'embedding_common.0.bias'
rel_err = fuse_bwd_ref.rel_err


@functools.lru_cache(maxsize=None)
def _refs(key, step):
    """The float64 graph of a fixture step, its absolute Jacobian (tower_ref.abs_jacobian) and the float32 graph's batch statistics --
    computed once per session, shared."""
    g64 = tower_ref.step_graph(key, step)
    absjac = {k: v.numpy() for k, v in tower_ref.abs_jacobian(g64).items()}
    return g64, absjac, tower_ref.step_graph(key, step, torch.float32)


def _state_before(key, step):
    arrays, _ = tower_ref.load_case(key)
    return tower_ref.sub(arrays, 'sd0/') if step == 1 else tower_ref.sub(arrays, 's%d/sd/' % (step - 1))


def _model(key, step=1, **overrides):
    """The model in the state the fixture's run had before `step`, enable_training() called; for step 2 the optimizer state of the
    fixture's step 1 is loaded through optimizer.load_state_dict."""
    arrays, meta = tower_ref.load_case(key)
    model = tower_ref.device_model(key, DEV, sd=_state_before(key, step), **overrides).enable_training()
    if step == 2:
        sq = tower_ref.sub(arrays, 's1/sq/')
        state = model.optimizer.state_dict()
        names = [k for k, _ in model.named_parameters()]
        assert state['param_groups'][0]['params'] == list(range(len(names)))
        state['state'] = {i: {'step': torch.tensor(float(meta['steps'][0]['opt_step'])),
                              'square_avg': torch.as_tensor(sq[k]).float().to(DEV)} for i, k in enumerate(names) if k in sq}
        model.optimizer.load_state_dict(state)
    return model


def _grad_bounds(key, step):
    """{name: (float64 gradient, element bound)} for every compared gradient of a fixture step."""
    arrays, meta = tower_ref.load_case(key)
    _, absjac, _ = _refs(key, step)
    e32 = meta['steps'][step - 1]['e32']
    out = {}
    for name, r64 in tower_ref.sub(arrays, 's%d/grad/' % step).items():
        if name.endswith(BIAS):
            continue
        # train_ref.end_to_end_bound takes the float32 CPU gradient to form e32 = max |r32 - r64| / max |r64|; the fixture keeps that
        # figure of the reference's float32 run, not the tensor, so the rule is handed a tensor with exactly that error: r64 with its
        # largest element moved by e32 max |r64|
        r64_t = torch.as_tensor(r64)
        r32_t = r64_t.clone()
        top = r64_t.abs().max()
        r32_t.view(-1)[r64_t.abs().argmax()] += e32['grad/' + name] * top
        bound, e, _ = TR.end_to_end_bound(r64_t, r32_t, torch.as_tensor(absjac[name]))
        assert abs(e - e32['grad/' + name]) <= 1e-6 * e32['grad/' + name] + 1e-300
        out[name] = (r64, bound.numpy())
    return out


def _check_step(key, step):
    arrays, meta = tower_ref.load_case(key)
    rec, pre = meta['steps'][step - 1], 's%d/' % step
    e32 = rec['e32']
    # ---- embeddings, on a model of their own (a training-mode forward moves the running statistics)
    probe = _model(key, step)
    data = tower_ref.train_data(key, step, DEV)
    txt = probe.txt_net(data['captions'])
    vis = probe.vis_net(data['vis_feats'], vis_frame_feat_dict_input=data['vis_frame_feat_dict'] or None)
    assert txt.requires_grad and vis.requires_grad
    for name, got in (('txt_emb', txt), ('vis_emb', vis)):
        err, bound = rel_err(got.detach().cpu(), arrays[pre + name]), max(4.0 * e32[name], TR.TOL_UNIT)
        print('case %s step %d %-8s device %.2e  reference fp32 %.2e  bound %.2e' % (key, step, name, err, e32[name], bound))
        assert err <= bound, (name, err, bound)
    # ---- loss and raw gradients: cal_foward + backward
    model = _model(key, step)
    loss, items = model.cal_foward(tower_ref.train_data(key, step, DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert items['triplet_loss'] is loss
    bound = max(4.0 * e32['loss'], TR.TOL_UNIT) * abs(rec['loss'])
    print('case %s step %d loss     device %.9g  float64 %.9g  bound %.2e' % (key, step, float(loss.detach()), rec['loss'], bound))
    assert abs(float(loss.detach()) - rec['loss']) <= bound
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert sorted(k for k, g in grads.items() if g is None) == rec['none']
    worst, sq_bound = 0.0, 0.0
    for name, (r64, b) in _grad_bounds(key, step).items():
        err = np.abs(grads[name].cpu().double().numpy() - r64)
        worst = max(worst, float((err / b).max()))
        sq_bound += float((b * b).sum())
        assert np.all(err <= b), (name, float((err / b).max()))
    for name, g in grads.items():
        if name.endswith(BIAS):
            assert not g.any(), name                       # exact zeros: softmax ignores a shift
    print('case %s step %d: %d gradients, worst err / bound %.3f' % (key, step, len(grads), worst))
    if meta['expert']:
        assert grads['vis_net.expert_embedding.weight'].abs().max() > 0 and grads['txt_net.expert_embedding.weight'].abs().max() > 0
    # ---- the step itself, on a fresh model
    stepped = _model(key, step)
    before = {k: p.detach().cpu().double().numpy().copy() for k, p in stepped.named_parameters()}
    sq0 = {k: stepped.optimizer.state[p]['square_avg'].cpu().double().numpy().copy() if p in stepped.optimizer.state else None
           for k, p in stepped.named_parameters()}
    items = stepped(tower_ref.train_data(key, step, DEV))
    torch.cuda.synchronize()
    assert stepped.iters == 1 and abs(float(items['triplet_loss'].detach()) - float(loss.detach())) == 0.0
    own = {k: p.grad for k, p in stepped.named_parameters() if p.grad is not None}
    assert all(torch.equal(own[k], grads[k]) for k in own) and sorted(own) == sorted(k for k, g in grads.items() if g is not None)
    total = float(stepped.optimizer.total_norm)
    tol = np.sqrt(sq_bound) + TR.TOL_UNIT * rec['total_norm']
    print('case %s step %d total norm device %.9g  float64 %.9g  bound %.2e' % (key, step, total, rec['total_norm'], tol))
    assert abs(total - rec['total_norm']) <= tol
    names = sorted(own)
    g_own = [own[k].cpu().double().numpy() for k in names]
    norm = optim_ref.total_norm(g_own)
    assert abs(total - norm) <= 2.0 ** -23 * norm and norm > meta['grad_clip']           # .grad is unclipped: its norm is the total norm
    c = optim_ref.clip_coef(norm, meta['grad_clip'])
    p0 = [before[k] for k in names]
    s0 = [sq0[k] if sq0[k] is not None else np.zeros_like(before[k]) for k in names]
    G = optim_ref.gmag(p0, g_own, c, 0.0)
    _, s_ref = optim_ref.rmsprop(p0, g_own, s0, meta['lr'], meta['alpha'], meta['eps'], 0.0, c)
    s_dev = [stepped.optimizer.state[dict(stepped.named_parameters())[k]]['square_avg'].cpu().numpy() for k in names]
    p_dev = [dict(stepped.named_parameters())[k].detach().cpu().numpy() for k in names]
    p_ref = optim_ref.rmsprop_param(p0, optim_ref.clipped(g_own, c), s_dev, meta['lr'], meta['eps'])
    for k, sd_, sr, sb, pd, pr, pb in zip(names, s_dev, s_ref, optim_ref.bound_v(s0, G, meta['alpha']), p_dev, p_ref,
                                          optim_ref.bound_p_rmsprop(p_ref, G, s_dev, meta['lr'], meta['eps'])):
        assert np.all(np.abs(sd_.astype(np.float64) - sr) <= sb), ('square_avg', k)
        assert np.all(np.abs(pd.astype(np.float64) - pr) <= pb), ('parameter', k)
    for k in rec['none']:
        assert np.array_equal(dict(stepped.named_parameters())[k].detach().cpu().double().numpy(), before[k])
    # ---- BatchNorm statistics after the step
    g64, _, g32 = _refs(key, step)
    sd_before, sd_after, sd_dev = _state_before(key, step), tower_ref.sub(arrays, pre + 'sd/'), stepped.state_dict()
    for prefix, (m64, v64) in g64['stats'].items():
        bn = prefix + 'bn1.'
        m32, v32 = g32['stats'][prefix]
        for stat, s64, s32 in (('running_mean', m64, m32), ('running_var', v64, v32)):
            old = torch.as_tensor(sd_before[bn + stat]).double()
            want = torch.as_tensor(sd_after[bn + stat]).double()
            bound = max(4.0 * rel_err(0.9 * old + 0.1 * s32.double(), want), TR.TOL_UNIT)
            err = rel_err(sd_dev[bn + stat].cpu(), want)
            assert err <= bound, (bn + stat, err, bound)
        assert int(sd_dev[bn + 'num_batches_tracked']) == int(sd_after[bn + 'num_batches_tracked'])
    return stepped, sq_bound


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_step_one_against_the_fixture(key):
    _check_step(key, 1)


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_teacher_forced_step_two(key):
    """From the fixture's parameters and optimizer state after step 1 (rounded to fp32), on the step-2 inputs."""
    _check_step(key, 2)


def test_free_running_step_two():
    """After our own step 1 the step-2 loss stays within the loss rule plus 20 lr sum of the step-1 element bounds: the first-order
    effect of every element whose update may have taken the other sign (+-10 lr each way)."""
    key = 'a'
    arrays, meta = tower_ref.load_case(key)
    model, _ = _check_step(key, 1)
    slack = sum(float(b.sum()) for _, b in _grad_bounds(key, 1).values())
    loss, _ = model.cal_foward(tower_ref.train_data(key, 2, DEV))
    rec = meta['steps'][1]
    bound = max(4.0 * rec['e32']['loss'], TR.TOL_UNIT) * abs(rec['loss']) + 20.0 * meta['lr'] * slack
    print('free-running step 2: loss %.9g  float64 %.9g  bound %.2e' % (float(loss.detach()), rec['loss'], bound))
    assert abs(float(loss.detach()) - rec['loss']) <= bound


def test_direct_callers_of_the_expert_stage_pieces_stay_refused():
    from laff_amd.model.model import TransformNet
    model = _model('d')
    x = torch.zeros(4, 40, device=DEV)
    with pytest.raises(NotImplementedError, match='extra_shift .the expert embedding. is not differentiable here'):
        model.vis_net.VisMutiTransformNet.X3D_L.plane(x, extra_shift=torch.zeros(512, device=DEV))
    with pytest.raises(NotImplementedError, match='the backward of the fusion has no row_scale'):
        model.vis_net.attention_layer.fuse_planes([torch.zeros(4, 512, device=DEV)], 4, l2norm_planes=True)
    assert isinstance(model.vis_net.VisMutiTransformNet.X3D_L, TransformNet)


def _one_step(key, seed=None, **overrides):
    model = _model(key, **overrides)
    if seed is not None:
        torch.manual_seed(seed)
    loss, _ = model.cal_foward(tower_ref.train_data(key, 1, DEV))
    loss.backward()
    model.optimizer.step()
    torch.cuda.synchronize()
    return model, loss.detach()


def test_dropout_follows_the_seed():
    a, la = _one_step('a', 11, dropout=0.2)
    b, lb = _one_step('a', 11, dropout=0.2)
    c, lc = _one_step('a', 12, dropout=0.2)
    assert torch.equal(la, lb) and not torch.equal(la, lc)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k


@pytest.mark.parametrize('key', ['a', 'd', 'e'])
def test_two_runs_of_a_step_give_identical_bits(key):
    a, la = _one_step(key)
    b, lb = _one_step(key)
    assert torch.equal(la, lb)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k


@pytest.mark.parametrize('key', ['a', 'd'])
def test_back_to_inference_after_a_step(key):
    """After one step and .eval() the embeddings are, bit for bit, those of a fresh model loaded with this one's state_dict(): no stale
    bn_affine, weight_t or strip cache survives the step."""
    from laff_amd.model.model import get_model
    arrays, meta = tower_ref.load_case(key)
    model = _model(key)
    with torch.no_grad():                                  # fill the eval-mode caches first
        model.eval()
        data = tower_ref.train_data(key, 2, DEV)
        stale_t, stale_v = model.txt_net(data['captions']), model.vis_net(data['vis_feats'])
        model.train()
    model(tower_ref.train_data(key, 1, DEV))
    model.eval()
    fresh = get_model('LAFF', DEV, tower_ref.make_cfg(meta)).eval()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        got = [model.txt_net(tower_ref.train_data(key, 2, DEV)['captions']), model.vis_net(tower_ref.train_data(key, 2, DEV)['vis_feats'])]
        want = [fresh.txt_net(tower_ref.train_data(key, 2, DEV)['captions']), fresh.vis_net(tower_ref.train_data(key, 2, DEV)['vis_feats'])]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], stale_t) and not torch.equal(got[1], stale_v)


def test_real_encoders_train_through_the_step():
    """A LAFF model fed CSR counts through BoWTxtEncoder and token ids through GruTxtEncoder(differentiable=True): one step runs;
    we.weight, every rnn.* and the bag-of-words fc1.weight receive finite gradients and change; the loss equals that of the same model
    fed the densified counts within TOL_UNIT relative."""
    from laff_amd import txt2vec as T
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    words = ['w%d' % i for i in range(30)]
    rng = np.random.default_rng(5)
    N = 12
    captions = [' '.join(rng.choice(words, size=rng.integers(1, 8)).tolist()) for _ in range(N)]
    vocab = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + words:
        vocab.add(w)
    cfg = make_config({'clip': 128, 'X3D_L': 40}, {'rnn': 32, 'bow': 30, 'CLIP': 128}, 512, 4, 'LAFF', vis_no_transform=['clip'],
                      txt_no_transform=['CLIP_encoder'], batch_norm=True, with_ave=True, dropout=0)
    torch.manual_seed(3)
    model = get_model('LAFF', DEV, cfg)
    model.txt_net.encoder.rnn_encoder = T.GruTxtEncoder(T.IdxVec(vocab), 12, 32, device=DEV, differentiable=True)
    model.txt_net.encoder.bow_encoder = T.BoWTxtEncoder(T.BowVec(words, clean=False), DEV, with_csc=True)
    model.train().enable_training()
    g = torch.Generator().manual_seed(9)
    feats = {'clip': torch.randn(N, 128, generator=g), 'X3D_L': torch.randn(N, 40, generator=g)}
    clip = torch.randn(N, 128, generator=g)

    def data():
        return {'vis_feats': {k: v.clone().to(DEV) for k, v in feats.items()}, 'captions': {'caption': captions, 'CLIP_encoding': clip.to(DEV)},
                'vis_frame_feat_dict': {}}
    bow = model.txt_net.encoder.bow_encoder
    counts = bow({'caption': captions})['text_features'].to_dense()

    class Dense(torch.nn.Module):
        def forward(self, caption_feat_dict, task3=False):
            return {'text_features': counts}
    model.txt_net.encoder.bow_encoder = Dense()            # the same model fed the densified counts: the loss before any step
    loss_dense = model.cal_foward(data())[0].detach()
    model.txt_net.encoder.bow_encoder = bow
    watched = {k: p for k, p in model.named_parameters()
               if k.startswith('txt_net.encoder.rnn_encoder.') or k == 'txt_net.transform_layer.bow_encoder_transform.fc1.weight'}
    assert any(k.endswith('we.weight') for k in watched) and sum('.rnn.' in k for k in watched) == 4 and len(watched) == 6
    before = {k: p.detach().clone() for k, p in watched.items()}
    items = model(data())
    torch.cuda.synchronize()
    loss = float(items['triplet_loss'])
    assert np.isfinite(loss) and abs(loss - float(loss_dense)) <= TR.TOL_UNIT * abs(float(loss_dense))
    for k, p in watched.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().max() > 0, k
        assert not torch.equal(p.detach(), before[k]), k
