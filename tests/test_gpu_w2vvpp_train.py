"""The W2VV++ concat towers in training mode and the model's training step on the MI355X, against float64 and against
the fixture of the reference's own steps (tests/golden/train_step_w2vvpp.<case>.<n>.npz, tools/gen_golden_train.py).

Rules, all of tests/train_ref.py, constants unchanged:
    module level         train_ref.compare: max |device - float64| / max |float64| within max(4 x the float32 CPU graph's, TOL_UNIT)
    the step             tests/train_step_check.py, shared with tests/test_gpu_train_step.py: embeddings, loss, raw gradients, total
                         norm, the optimizer on the device's own gradients, running statistics
"""
import copy

import numpy as np
import pytest
import torch

import tower_ref
import train_ref as TR
import train_step_check as SC

pytestmark = pytest.mark.gpu

DEV = SC.DEV


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
@pytest.mark.parametrize('key', tower_ref.CONCAT_CASES)
def test_step_one_against_the_fixture(key):
    SC.check_step(key, 1)


@pytest.mark.parametrize('key', tower_ref.CONCAT_CASES)
def test_teacher_forced_step_two(key):
    """From the fixture's parameters and optimizer state after step 1 (rounded to fp32), on the step-2 inputs."""
    SC.check_step(key, 2)


@pytest.mark.parametrize('key', tower_ref.CONCAT_CASES)
def test_back_to_inference_after_a_step(key):
    """After one step and .eval() the embeddings change and are, bit for bit, those of a fresh model loaded with this one's
    state_dict(): no stale weight_t_block or bn_affine survives the step; eval mode runs the one-launch forward as before."""
    SC.back_to_inference_after_a_step(key)


def test_step_refusals_on_the_device():
    from laff_amd.model.model import get_model
    _, meta = tower_ref.load_case('i')
    with pytest.raises(NotImplementedError, match="key 'LAFF' with the concat towers"):
        get_model('LAFF', DEV, tower_ref.make_cfg(dict(meta, model='LAFF'))).enable_training()
    for field, value, text in (('negative', True, 'opt.negative'), ('multi_space', False, 'multi_space=False')):
        with pytest.raises(NotImplementedError, match=text):
            tower_ref.device_model('i', DEV, **{field: value}).enable_training()
    # the per-head Adam keeps its eps where the towers are not concat: nothing changes for the models that trained before
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
