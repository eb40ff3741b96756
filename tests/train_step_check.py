"""One training step of a model on the MI355X against a case of the training-step fixture (tests/tower_ref.py: cases a-e 'LAFF' and
'FrameLAFF', i and ii the W2VV++ concat towers; two steps of the reference in float64 and float32, tools/gen_golden_train.py).  What
tests/test_gpu_train_step.py and tests/test_gpu_w2vvpp_train.py share.

Rules, all of tests/train_ref.py, constants unchanged:
    embeddings, loss     max |device - float64| <= max(4 e32, TOL_UNIT) max |float64|, e32 the fixture's recorded error of the
                         reference's own float32 run for that tensor
    raw gradients        element by element under end_to_end_bound: max(4 e32, TOL_UNIT) max |r64| + GRAD_ABS sum_j |d r / d E_j|, the
                         absolute Jacobian from the float64 restatement tests/tower_ref.py (once per session)
    total norm           | |g| - |g64| | <= |g - g64| <= sqrt(sum of the squared element bounds), plus TOL_UNIT |g64| for the sum itself
    the step             parameters and optimizer state (RMSprop: square_avg; Adam: exp_avg, exp_avg_sq) against tests/optim_ref.py
                         applied to this model's OWN device gradients, under the bounds of tests/test_gpu_optim.py -- no element-wise
                         comparison of stepped parameters with the fixture: the first update is +-lr-sized whatever |g| (RMSprop's is
                         +-10 lr), so an element whose gradient lies inside its bound may take the other sign
                         (tower_ref.replay_steps ties the optimizer to the reference instead, on the host)
    running statistics   max(4 e32, TOL_UNIT) as the dropout-BN test, e32 from the restatement in float32
The embedding_common.0.bias gradients are exact zeros here and rounding noise in the reference (softmax ignores a shift): they are
asserted to be zero and left out of every comparison with the reference.
"""
import functools

import numpy as np
import torch

import optim_ref
import tower_ref
import train_ref as TR

DEV = 'cuda'
BIAS = 'embedding_common.0.bias'
rel_err = tower_ref.rel_err
sub = tower_ref.sub


@functools.lru_cache(maxsize=None)
def refs(key, step):
    """The float64 graph of a fixture step, its absolute Jacobian (tower_ref.abs_jacobian) and the float32 graph's batch statistics --
    computed once per session, shared."""
    g64 = tower_ref.step_graph(key, step)
    absjac = {k: v.numpy() for k, v in tower_ref.abs_jacobian(g64).items()}
    return g64, absjac, tower_ref.step_graph(key, step, torch.float32)


def model(key, step=1, **overrides):
    """The model in the state the fixture's run had before `step`, enable_training() called; for step 2 the optimizer state of the
    fixture's step 1 is loaded through optimizer.load_state_dict."""
    arrays, meta = tower_ref.load_case(key)
    net = tower_ref.device_model(key, DEV, sd=tower_ref.state_before(arrays, step), **overrides).enable_training()
    if meta['attention'] == 'concat':
        assert net.vis_net.training_armed and net.txt_net.training_armed
    if 'optimizer' not in overrides:                       # (the concat cases: the base class's optimizers, torch's default eps)
        assert net.optimizer.param_groups[0]['eps'] == meta['eps'] == 1e-8
    if step == 2:
        old = {n: sub(arrays, 's1/state/%s/' % n) for n in tower_ref.STATE_NAMES[meta['optimizer']]}
        state = net.optimizer.state_dict()
        names = [k for k, _ in net.named_parameters()]
        assert state['param_groups'][0]['params'] == list(range(len(names)))
        state['state'] = {i: dict({'step': torch.tensor(float(meta['steps'][0]['opt_step']))},
                                  **{n: torch.as_tensor(v[k]).float().to(DEV) for n, v in old.items()})
                          for i, k in enumerate(names) if all(k in v for v in old.values())}
        net.optimizer.load_state_dict(state)
    return net


def grad_bounds(key, step):
    """{name: (float64 gradient, element bound)} for every compared gradient of a fixture step."""
    arrays, meta = tower_ref.load_case(key)
    _, absjac, _ = refs(key, step)
    e32 = meta['steps'][step - 1]['e32']
    out = {}
    for name, r64 in sub(arrays, 's%d/grad/' % step).items():
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


def check_step(key, step):
    """Step `step` (1 or 2) of a case on the device under the rules above; returns the stepped model."""
    arrays, meta = tower_ref.load_case(key)
    rec, pre = meta['steps'][step - 1], 's%d/' % step
    e32 = rec['e32']
    # ---- embeddings, on a model of their own (a training-mode forward moves the running statistics)
    probe = model(key, step)
    data = tower_ref.train_data(key, step, DEV)
    txt = probe.txt_net(data['captions'])
    vis = probe.vis_net(data['vis_feats'], vis_frame_feat_dict_input=data['vis_frame_feat_dict'] or None)
    assert txt.requires_grad and vis.requires_grad
    if meta['attention'] == 'concat':
        assert txt.dim() == vis.dim() == 2
    for name, got in (('txt_emb', txt), ('vis_emb', vis)):
        err, bound = rel_err(got.detach().cpu(), arrays[pre + name]), max(4.0 * e32[name], TR.TOL_UNIT)
        print('case %s step %d %-8s device %.2e  reference fp32 %.2e  bound %.2e' % (key, step, name, err, e32[name], bound))
        assert err <= bound, (name, err, bound)
    # ---- loss and raw gradients: cal_foward + backward
    net = model(key, step)
    loss, items = net.cal_foward(tower_ref.train_data(key, step, DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert items['triplet_loss'] is loss
    bound = max(4.0 * e32['loss'], TR.TOL_UNIT) * abs(rec['loss'])
    print('case %s step %d loss     device %.9g  float64 %.9g  bound %.2e' % (key, step, float(loss.detach()), rec['loss'], bound))
    assert abs(float(loss.detach()) - rec['loss']) <= bound
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert sorted(k for k, g in grads.items() if g is None) == rec['none']
    assert sorted(k for k, g in grads.items() if g is not None) == sorted(sub(arrays, pre + 'grad/'))
    worst, sq_bound = 0.0, 0.0
    for name, (r64, b) in grad_bounds(key, step).items():
        err = np.abs(grads[name].cpu().double().numpy() - r64)
        worst = max(worst, float((err / b).max()))
        sq_bound += float((b * b).sum())
        assert np.all(err <= b), (name, float((err / b).max()))
    for name, g in grads.items():
        if name.endswith(BIAS):
            assert not g.any(), name                       # exact zeros: softmax ignores a shift
    print('case %s step %d: %d gradients, worst err / bound %.3f' % (key, step, len(grads), worst))
    if meta.get('expert'):
        assert grads['vis_net.expert_embedding.weight'].abs().max() > 0 and grads['txt_net.expert_embedding.weight'].abs().max() > 0
    # ---- the step itself, on a fresh model: optim_ref on the device's own gradients, the bounds of test_gpu_optim.py
    stepped = model(key, step)
    params = dict(stepped.named_parameters())
    before = {k: p.detach().cpu().double().numpy().copy() for k, p in params.items()}
    kept = tower_ref.STATE_NAMES[meta['optimizer']]
    old = {n: {k: stepped.optimizer.state[p][n].cpu().double().numpy().copy() if p in stepped.optimizer.state else np.zeros_like(before[k])
               for k, p in params.items()} for n in kept}
    items = stepped(tower_ref.train_data(key, step, DEV))
    torch.cuda.synchronize()
    assert stepped.iters == 1 and abs(float(items['triplet_loss'].detach()) - float(loss.detach())) == 0.0
    own = {k: p.grad for k, p in params.items() if p.grad is not None}
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
    old = {n: [v[k] for k in names] for n, v in old.items()}
    G = optim_ref.gmag(p0, g_own, c, 0.0)
    new = {n: [stepped.optimizer.state[params[k]][n].cpu().numpy() for k in names] for n in kept}
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
    for k in rec['none']:
        assert np.array_equal(params[k].detach().cpu().double().numpy(), before[k])
    assert any(not np.array_equal(a.astype(np.float64), before[k]) for k, a in zip(names, p_dev))
    # ---- BatchNorm statistics after the step
    g64, _, g32 = refs(key, step)
    sd_before, sd_after, sd_dev = tower_ref.state_before(arrays, step), sub(arrays, pre + 'sd/'), stepped.state_dict()
    for prefix in g64['stats']:
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


def back_to_inference_after_a_step(key):
    """After one step and .eval() the embeddings change and are, bit for bit, those of a fresh model loaded with this one's
    state_dict(): no stale bn_affine, weight_t, weight_t_block or strip cache survives the step."""
    from laff_amd.model.model import get_model
    _, meta = tower_ref.load_case(key)
    net = model(key)
    with torch.no_grad():                                  # fill the eval-mode caches first
        net.eval()
        data = tower_ref.train_data(key, 2, DEV)
        stale_t, stale_v = net.txt_net(data['captions']), net.vis_net(data['vis_feats'])
        net.train()
    net(tower_ref.train_data(key, 1, DEV))
    net.eval()
    fresh = get_model(meta['model'], DEV, tower_ref.make_cfg(meta)).eval()
    fresh.load_state_dict(net.state_dict())
    with torch.no_grad():
        got = [net.txt_net(tower_ref.train_data(key, 2, DEV)['captions']), net.vis_net(tower_ref.train_data(key, 2, DEV)['vis_feats'])]
        want = [fresh.txt_net(tower_ref.train_data(key, 2, DEV)['captions']), fresh.vis_net(tower_ref.train_data(key, 2, DEV)['vis_feats'])]
    assert not got[0].requires_grad and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], stale_t) and not torch.equal(got[1], stale_v)
