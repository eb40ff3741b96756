"""The W2VV++ concat towers in training mode and the model's training step on the MI355X, against float64 and against
the fixture of the reference's own steps (tests/golden/train_step_w2vvpp.<case>.<n>.npz, tools/gen_golden_train_w2vvpp.py).

Rules, all of tests/train_ref.py and tests/test_gpu_train_step.py, constants unchanged:
    module level         train_ref.compare: max |device - float64| / max |float64| within max(4 x the float32 CPU graph's, TOL_UNIT)
    embeddings, loss     max |device - float64| <= max(4 e32, TOL_UNIT) max |float64|, e32 the fixture's recorded error of the
                         reference's own float32 run for that tensor
    raw gradients        element by element under end_to_end_bound, the absolute Jacobian from tests/concat_tower_ref.py
    the step             parameters and optimizer state against tests/optim_ref.py applied to this model's OWN device gradients, under
                         the bounds of tests/test_gpu_optim.py; not compared with the fixture element by element (the
                         first update is +-lr-sized whatever |g|; tests/test_fc_concat_bwd_host.py ties the optimizer to the reference)
"""
import copy
import functools

import numpy as np
import pytest
import torch

import concat_tower_ref as CT
import fuse_bwd_ref
import optim_ref
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
rel_err = fuse_bwd_ref.rel_err
sub = CT.tower_ref.sub


# ---- the armed towers against float64 and against the per-segment route -------------------------------------------------------------
N, WIDTHS, D = 33, (36, 50, 30), 64          # dense + CSR + dense -> 64, as tests/test_gpu_fc_gather_backward.py::test_concat_train


def _bow(n, dk, seed, per_row=6):
    rng = np.random.default_rng(seed)
    dense = torch.zeros(n, dk)
    for r in range(n):
        for v in rng.choice(dk, size=rng.integers(1, per_row + 1), replace=False):
            dense[r, v] = float(rng.integers(1, 4))
    sp = dense.to_sparse_csr()
    return torch.sparse_csr_tensor(sp.crow_indices().to(torch.int32), sp.col_indices().to(torch.int32), sp.values(), size=(n, dk)), dense


def _towers(batch_norm):
    """A 'W2VVPP' model whose two towers both see dense 36 + CSR 50 + dense 30, armed, in training mode: (model, the video tower and
    how to feed it, the text tower and how to feed it)."""
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    cfg = make_config(dict(zip('abc', WIDTHS)), {'rnn': WIDTHS[0], 'bow': WIDTHS[1], 'w2v': WIDTHS[2]}, D, 1, 'W2VVPP',
                      txt_attention='concat', vis_attention='concat', batch_norm=batch_norm, dropout=0)
    model = get_model('W2VVPP', DEV, cfg).train()
    assert model.txt_net.encoder.encoder_name_list == ['rnn_encoder', 'bow_encoder', 'w2v_encoder']
    feed_vis = lambda segs: model.vis_net(dict(zip('abc', segs)))                                              # noqa: E731
    feed_txt = lambda segs: model.txt_net(dict(zip(('rnn_encoding', 'bow_encoding', 'w2v_encoding'), segs)))   # noqa: E731
    return model, (model.vis_net, model.vis_net, feed_vis), (model.txt_net, model.txt_net.transformer, feed_txt)


@pytest.mark.parametrize('side', ['vis', 'txt'])
@pytest.mark.parametrize('batch_norm', [True, False], ids=['bn', 'nobn'])
def test_armed_tower_against_float64_and_the_per_segment_route(side, batch_norm, monkeypatch):
    from laff_amd import ops
    torch.manual_seed(23)
    model, vis, txt = _towers(batch_norm)
    tower, layer, feed = vis if side == 'vis' else txt
    with torch.no_grad():
        layer.fc1.bias.normal_(0.0, 0.1)
    W, b = layer.fc1.weight.detach().cpu().clone(), layer.fc1.bias.detach().cpu().clone()
    csr, bow = _bow(N, WIDTHS[1], 21)
    dense = [torch.randn(N, WIDTHS[0]), bow, torch.randn(N, WIDTHS[2])]
    dE = torch.randn(N, D)

    def segments():
        return [dense[0].to(DEV), csr.to(DEV), dense[2].to(DEV).requires_grad_(True)]      # the last dense segment requires a gradient
    # unarmed: today's refusal; armed by hand here (enable_training() does it for a whole model: the step tests below)
    with pytest.raises(NotImplementedError, match='inference path only'):
        feed(segments())
    tower.training_armed = True
    old_route = copy.deepcopy(layer)                      # the same layer through TransformNet.concat_train, the per-segment route
    calls = {'fc_concat_backward': 0, 'fc_backward': 0, 'fc_gather_backward': 0}
    for name in calls:
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: calls.__setitem__(_n, calls[_n] + 1) or _r(*a, **k))
    segs = segments()
    y = feed(segs)
    assert y.requires_grad and tuple(y.shape) == (N, D)
    y.backward(dE.to(DEV))
    torch.cuda.synchronize()
    # the video tower: one library call for the whole backward of the layer, none of the per-segment ones.  The text tower keeps the
    # per-segment calls (the grouped call measured slower at its nominal mix of segments)
    own = {'fc_concat_backward': 1, 'fc_backward': 0, 'fc_gather_backward': 0} if side == 'vis' else \
        {'fc_concat_backward': 0, 'fc_backward': 2, 'fc_gather_backward': 1}
    assert calls == own, calls
    x = torch.cat(dense, 1)
    ref = TR.layer_graph(torch.float64, W, b, x, dE, 'tanh', batch_norm, None, 0.0)
    f32 = TR.layer_graph(torch.float32, W, b, x, dE, 'tanh', batch_norm, None, 0.0)
    got = {'y': y, 'fc1.weight.grad': layer.fc1.weight.grad, 'fc1.bias.grad': layer.fc1.bias.grad}
    if batch_norm:
        got.update({'bn1.weight.grad': layer.bn1.weight.grad, 'bn1.bias.grad': layer.bn1.bias.grad, 'running_mean': layer.bn1.running_mean,
                    'running_var': layer.bn1.running_var})
    lo = WIDTHS[0] + WIDTHS[1]
    key = 'x.grad[%d:%d]' % (lo, lo + WIDTHS[2])
    got[key], ref[key], f32[key] = segs[2].grad, ref['x.grad'][:, lo:], f32['x.grad'][:, lo:]
    assert segs[0].grad is None
    TR.compare(got, ref, f32, '%s tower, %s' % (side, 'bn' if batch_norm else 'no bn'))
    assert layer.fc1.weight.grad.is_contiguous() and layer.fc1.weight.grad.shape == (D, sum(WIDTHS))
    # the per-segment route on the same inputs: the parameter gradients and the segment's have its bits
    old_route.device_norm = layer.device_norm
    segs2 = segments()
    old_route.train().concat_train(segs2).backward(dE.to(DEV))
    torch.cuda.synchronize()
    assert calls == {k: v + {'fc_concat_backward': 0, 'fc_backward': 2, 'fc_gather_backward': 1}[k] for k, v in own.items()}, calls
    for (k, p), q in zip(layer.named_parameters(), old_route.parameters()):
        assert torch.equal(p.grad, q.grad), k
    assert torch.equal(segs[2].grad, segs2[2].grad)
    # ... and so has the grouped Function on the text tower's layer, which the tower itself does not take
    if side == 'txt':
        third = copy.deepcopy(old_route)
        third.zero_grad(set_to_none=True)
        segs3 = segments()
        third.train().concat_train(segs3, grouped=True).backward(dE.to(DEV))
        torch.cuda.synchronize()
        assert calls['fc_concat_backward'] == 1
        for (k, p), q in zip(layer.named_parameters(), third.parameters()):
            assert torch.equal(p.grad, q.grad), k
        assert torch.equal(segs[2].grad, segs3[2].grad)


# ---- both fixture cases on the device ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs(key, step):
    g64 = CT.step_graph(key, step)
    absjac = {k: v.numpy() for k, v in CT.abs_jacobian(g64).items()}
    return g64, absjac, CT.step_graph(key, step, torch.float32)


def _state_before(key, step):
    arrays, _ = CT.load_case(key)
    return sub(arrays, 'sd0/') if step == 1 else sub(arrays, 's%d/sd/' % (step - 1))


def _state_names(meta):
    return ('square_avg',) if meta['optimizer'] == 'rmsprop' else ('exp_avg', 'exp_avg_sq')


def _model(key, step=1, **overrides):
    """The model in the state the fixture's run had before `step`, enable_training() called; for step 2 the optimizer state of the
    fixture's step 1 is loaded through optimizer.load_state_dict."""
    arrays, meta = CT.load_case(key)
    model = CT.device_model(key, DEV, sd=_state_before(key, step), **overrides).enable_training()
    assert model.vis_net.training_armed and model.txt_net.training_armed
    assert model.optimizer.param_groups[0]['eps'] == 1e-8                    # both cases: the base class's optimizers, torch's default eps
    if step == 2:
        state = model.optimizer.state_dict()
        names = [k for k, _ in model.named_parameters()]
        assert state['param_groups'][0]['params'] == list(range(len(names)))
        state['state'] = {i: dict({'step': torch.tensor(float(meta['steps'][0]['opt_step']))},
                                  **{n: torch.as_tensor(arrays['s1/state/%s/%s' % (n, k)]).float().to(DEV) for n in _state_names(meta)})
                          for i, k in enumerate(names)}
        model.optimizer.load_state_dict(state)
    return model


def _grad_bounds(key, step):
    """{name: (float64 gradient, element bound)} for every gradient of a fixture step (the rule of test_gpu_train_step.py)."""
    arrays, meta = CT.load_case(key)
    _, absjac, _ = _refs(key, step)
    e32 = meta['steps'][step - 1]['e32']
    out = {}
    for name, r64 in sub(arrays, 's%d/grad/' % step).items():
        # end_to_end_bound takes the float32 CPU gradient to form e32; the fixture keeps that figure of the reference's float32 run, not
        # the tensor, so the rule is handed a tensor with exactly that error: r64 with its largest element moved by e32 max |r64|
        r64_t = torch.as_tensor(r64)
        r32_t = r64_t.clone()
        r32_t.view(-1)[r64_t.abs().argmax()] += e32['grad/' + name] * r64_t.abs().max()
        bound, e, _ = TR.end_to_end_bound(r64_t, r32_t, torch.as_tensor(absjac[name]))
        assert abs(e - e32['grad/' + name]) <= 1e-6 * e32['grad/' + name] + 1e-300
        out[name] = (r64, bound.numpy())
    return out


def _check_step(key, step):
    arrays, meta = CT.load_case(key)
    rec, pre = meta['steps'][step - 1], 's%d/' % step
    e32 = rec['e32']
    # ---- embeddings, on a model of their own (a training-mode forward moves the running statistics)
    probe = _model(key, step)
    data = CT.train_data(key, step, DEV)
    txt, vis = probe.txt_net(data['captions']), probe.vis_net(data['vis_feats'])
    assert txt.requires_grad and vis.requires_grad and txt.dim() == vis.dim() == 2
    for name, got in (('txt_emb', txt), ('vis_emb', vis)):
        err, bound = rel_err(got.detach().cpu(), arrays[pre + name]), max(4.0 * e32[name], TR.TOL_UNIT)
        print('case %s step %d %-8s device %.2e  reference fp32 %.2e  bound %.2e' % (key, step, name, err, e32[name], bound))
        assert err <= bound, (name, err, bound)
    # ---- loss and raw gradients: cal_foward + backward
    model = _model(key, step)
    loss, items = model.cal_foward(CT.train_data(key, step, DEV))
    loss.backward()
    torch.cuda.synchronize()
    bound = max(4.0 * e32['loss'], TR.TOL_UNIT) * abs(rec['loss'])
    print('case %s step %d loss     device %.9g  float64 %.9g  bound %.2e' % (key, step, float(loss.detach()), rec['loss'], bound))
    assert abs(float(loss.detach()) - rec['loss']) <= bound
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None for g in grads.values()) and sorted(grads) == sorted(sub(arrays, pre + 'grad/'))
    worst = 0.0
    for name, (r64, b) in _grad_bounds(key, step).items():
        err = np.abs(grads[name].cpu().double().numpy() - r64)
        worst = max(worst, float((err / b).max()))
        assert np.all(err <= b), (name, float((err / b).max()))
    print('case %s step %d: %d gradients, worst err / bound %.3f' % (key, step, len(grads), worst))
    # ---- the step itself, on a fresh model: optim_ref on the device's own gradients, the bounds of test_gpu_optim.py
    stepped = _model(key, step)
    params = dict(stepped.named_parameters())
    names = sorted(params)
    before = {k: p.detach().cpu().double().numpy().copy() for k, p in params.items()}
    old = {n: [stepped.optimizer.state[params[k]][n].cpu().double().numpy().copy() if params[k] in stepped.optimizer.state
               else np.zeros_like(before[k]) for k in names] for n in _state_names(meta)}
    items = stepped(CT.train_data(key, step, DEV))
    torch.cuda.synchronize()
    assert stepped.iters == 1 and float(items['triplet_loss'].detach()) == float(loss.detach())
    assert all(torch.equal(params[k].grad, grads[k]) for k in names)
    g_own = [params[k].grad.cpu().double().numpy() for k in names]
    norm = optim_ref.total_norm(g_own)
    total = float(stepped.optimizer.total_norm)
    assert abs(total - norm) <= 2.0 ** -23 * norm
    # | |g| - |g64| | <= |g - g64| <= sqrt(sum of the squared element bounds), plus TOL_UNIT |g64| for the sum itself
    tol = float(np.sqrt(sum(float((b * b).sum()) for _, b in _grad_bounds(key, step).values()))) + TR.TOL_UNIT * rec['total_norm']
    assert abs(total - rec['total_norm']) <= tol, (total, rec['total_norm'], tol)
    c = optim_ref.clip_coef(norm, meta['grad_clip'])
    p0 = [before[k] for k in names]
    G = optim_ref.gmag(p0, g_own, c, 0.0)
    new = {n: [stepped.optimizer.state[params[k]][n].cpu().numpy() for k in names] for n in _state_names(meta)}
    p_dev = [params[k].detach().cpu().numpy() for k in names]
    lr, eps = meta['lr'], meta['eps']
    if meta['optimizer'] == 'rmsprop':
        _, s_ref = optim_ref.rmsprop(p0, g_own, old['square_avg'], lr, meta['alpha'], eps, 0.0, c)
        checks = [('square_avg', new['square_avg'], s_ref, optim_ref.bound_v(old['square_avg'], G, meta['alpha']))]
        p_ref = optim_ref.rmsprop_param(p0, optim_ref.clipped(g_own, c), new['square_avg'], lr, eps)
        checks.append(('parameter', p_dev, p_ref, optim_ref.bound_p_rmsprop(p_ref, G, new['square_avg'], lr, eps)))
    else:
        b1, b2 = meta['betas']
        t = step                                           # the fixture's optimizer is at step 1 before step 2
        _, m_ref, v_ref = optim_ref.adam(p0, g_own, old['exp_avg'], old['exp_avg_sq'], lr, b1, b2, eps, 0.0, t, c)
        checks = [('exp_avg', new['exp_avg'], m_ref, optim_ref.bound_m(old['exp_avg'], G, b1)),
                  ('exp_avg_sq', new['exp_avg_sq'], v_ref, optim_ref.bound_v(old['exp_avg_sq'], G, b2))]
        p_ref = optim_ref.adam_param(p0, new['exp_avg'], new['exp_avg_sq'], lr, b1, b2, eps, t)
        checks.append(('parameter', p_dev, p_ref, optim_ref.bound_p_adam(p_ref, new['exp_avg'], new['exp_avg_sq'], lr, b1, b2, eps, t)))
    for what, dev, ref, bounds in checks:
        for k, a, r, bd in zip(names, dev, ref, bounds):
            assert np.all(np.abs(a.astype(np.float64) - r) <= bd), (what, k)
    assert any(not np.array_equal(a.astype(np.float64), before[k]) for k, a in zip(names, p_dev))
    # ---- BatchNorm statistics after the step
    g64, _, g32 = _refs(key, step)
    sd_before, sd_after, sd_dev = _state_before(key, step), sub(arrays, pre + 'sd/'), stepped.state_dict()
    for prefix, (m64, v64) in g64['stats'].items():
        bn = prefix + 'bn1.'
        m32, v32 = g32['stats'][prefix]
        for stat, s32 in (('running_mean', m32), ('running_var', v32)):
            prev = torch.as_tensor(sd_before[bn + stat]).double()
            want = torch.as_tensor(sd_after[bn + stat]).double()
            bound = max(4.0 * rel_err(0.9 * prev + 0.1 * s32.double(), want), TR.TOL_UNIT)
            err = rel_err(sd_dev[bn + stat].cpu(), want)
            assert err <= bound, (bn + stat, err, bound)
        assert int(sd_dev[bn + 'num_batches_tracked']) == int(sd_after[bn + 'num_batches_tracked'])
    return stepped


@pytest.mark.parametrize('key', CT.CASES)
def test_step_one_against_the_fixture(key):
    _check_step(key, 1)


@pytest.mark.parametrize('key', CT.CASES)
def test_teacher_forced_step_two(key):
    """From the fixture's parameters and optimizer state after step 1 (rounded to fp32), on the step-2 inputs."""
    _check_step(key, 2)


@pytest.mark.parametrize('key', CT.CASES)
def test_back_to_inference_after_a_step(key):
    """After one step and .eval() the embeddings change and are, bit for bit, those of a fresh model loaded with this one's
    state_dict(): no stale weight_t_block or bn_affine survives the step; eval mode runs the one-launch forward as before."""
    from laff_amd.model.model import get_model
    arrays, meta = CT.load_case(key)
    model = _model(key)
    with torch.no_grad():                                  # fill the eval-mode caches first
        model.eval()
        data = CT.train_data(key, 2, DEV)
        stale_t, stale_v = model.txt_net(data['captions']), model.vis_net(data['vis_feats'])
        model.train()
    model(CT.train_data(key, 1, DEV))
    model.eval()
    fresh = get_model(meta['model'], DEV, CT.make_cfg(meta)).eval()
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        got = [model.txt_net(CT.train_data(key, 2, DEV)['captions']), model.vis_net(CT.train_data(key, 2, DEV)['vis_feats'])]
        want = [fresh.txt_net(CT.train_data(key, 2, DEV)['captions']), fresh.vis_net(CT.train_data(key, 2, DEV)['vis_feats'])]
    assert not got[0].requires_grad and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], stale_t) and not torch.equal(got[1], stale_v)


def test_step_refusals_on_the_device():
    from laff_amd.model.model import get_model
    _, meta = CT.load_case('i')
    with pytest.raises(NotImplementedError, match="key 'LAFF' with the concat towers"):
        get_model('LAFF', DEV, CT.make_cfg(dict(meta, model='LAFF'))).enable_training()
    for field, value, text in (('negative', True, 'opt.negative'), ('multi_space', False, 'multi_space=False')):
        with pytest.raises(NotImplementedError, match=text):
            CT.device_model('i', DEV, **{field: value}).enable_training()
    # the per-head Adam keeps its eps where the towers are not concat: nothing changes for the models that trained before
    import tower_ref
    assert tower_ref.device_model('a', DEV, optimizer='adam').enable_training().optimizer.param_groups[0]['eps'] == 1e-4


# ---- a W2VV++ text tower as data.pair_provider feeds it -----------------------------------------------------------------------------
def test_two_steps_from_prepared_inputs_and_from_the_strings(tmp_path):
    """'W2VVPP' with the text tower bigru (differentiable) + bag of words (CSR with its laff_csc) + word2vec, on a tiny corpus: two steps
    fed by the provider's prepared inputs and two fed the strings give the same loss, .grad and parameter bits; the GRU's embedding
    table and recurrent weights receive nonzero gradients through the tower's dense segment."""
    import pair_ref
    import test_gpu_pair_provider as PP
    from laff_amd import data
    from laff_amd import txt2vec as T
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    B, H = 12, 32
    shape = dict(N=B, vid_dims={'a': 24, 'b': 16}, txt_dims={'bow': len(PP.WORDS), 'w2v': 20})
    ds = PP._training_set(shape, 2 * B, np.random.default_rng(31), real_text=True)
    sampler = [int(i) for i in np.random.default_rng(8).permutation(2 * B)]

    def model():
        cfg = make_config(shape['vid_dims'], dict(shape['txt_dims'], rnn=H), 64, 1, 'W2VVPP', txt_attention='concat', vis_attention='concat',
                          batch_norm=True, dropout=0)
        cfg.text_encoding['rnn_encoding']['name'] = 'bigru_mean'
        torch.manual_seed(5)
        m = get_model('W2VVPP', DEV, cfg)
        assert m.txt_net.encoder.encoder_name_list == ['rnn_encoder', 'bow_encoder', 'w2v_encoder']
        assert m.txt_net.transformer.fc1.in_features == 2 * H + len(PP.WORDS) + 20
        vocab = T.Vocabulary('gru')
        for w in ['<pad>', '<start>', '<end>', '<unk>'] + PP.WORDS:
            vocab.add(w)
        w2v = T.W2Vec(PP.WORDS[:25], np.random.default_rng(6).standard_normal((25, 20)).astype(np.float32))
        enc = {'rnn_encoder': T.GruTxtEncoder(T.IdxVec(vocab), 12, H, bidirectional=True, device=DEV, differentiable=True),
               'bow_encoder': T.BoWTxtEncoder(T.BowVec(PP.WORDS), DEV, with_csc=True), 'w2v_encoder': T.W2VTxtEncoder(w2v, DEV)}
        for name, e in enc.items():
            setattr(m.txt_net.encoder.encoder, name, e)
        return m.train().enable_training(), enc
    fed, enc = model()
    provider = data.pair_provider(pair_ref.write_dataset(ds, tmp_path, batch_size=B, sampler=sampler, device=DEV, encoders=enc))
    host, _ = model()
    losses = []
    for step, batch in enumerate(provider):
        assert T.PREPARED_KEY in batch['captions']
        a = fed(batch)
        b = host(PP._to_device(pair_ref.collate(ds, sampler[step * B:(step + 1) * B])))
        torch.cuda.synchronize()
        la, lb = a['triplet_loss'].detach(), b['triplet_loss'].detach()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
        losses.append(float(la))
        for (k, p), q in zip(fed.named_parameters(), host.parameters()):
            assert p.grad is not None and q.grad is not None and torch.equal(p.grad, q.grad), (step, k)
            assert torch.equal(p.detach(), q.detach()), (step, k)
    assert step == 1 and fed.iters == host.iters == 2 and losses[0] != losses[1]
    grads = {k: p.grad for k, p in fed.named_parameters()}
    watched = [k for k in grads if k.startswith('txt_net.encoder.encoder.rnn_encoder.')]
    assert any(k.endswith('we.weight') for k in watched) and sum('.rnn.' in k for k in watched) >= 4
    for k in watched + ['txt_net.transformer.fc1.weight']:
        assert bool(torch.isfinite(grads[k]).all()) and grads[k].abs().max() > 0, k
