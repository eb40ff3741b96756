"""The 'LAFF' and 'FrameLAFF' models' training step on the MI355X against the training-step fixture of the reference
(tests/golden/train_step.<case>.<n>.npz: two RMSprop steps of the reference in float64 and float32, tools/gen_golden_train.py).  The
step check itself and its rules are tests/train_step_check.py's, shared with tests/test_gpu_w2vvpp_train.py; what only these models
have is here: the free-running second step, the expert stage's refusals, dropout, identical bits, real text encoders."""
import numpy as np
import pytest
import torch

import tower_ref
import train_ref as TR
import train_step_check as SC

pytestmark = pytest.mark.gpu

DEV = SC.DEV
_model = SC.model


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_step_one_against_the_fixture(key):
    SC.check_step(key, 1)


@pytest.mark.parametrize('key', tower_ref.CASES)
def test_teacher_forced_step_two(key):
    """From the fixture's parameters and optimizer state after step 1 (rounded to fp32), on the step-2 inputs."""
    SC.check_step(key, 2)


def test_free_running_step_two():
    """After our own step 1 the step-2 loss stays within the loss rule plus 20 lr sum of the step-1 element bounds: the first-order
    effect of every element whose update may have taken the other sign (+-10 lr each way)."""
    key = 'a'
    arrays, meta = tower_ref.load_case(key)
    model = SC.check_step(key, 1)
    slack = sum(float(b.sum()) for _, b in SC.grad_bounds(key, 1).values())
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
    SC.back_to_inference_after_a_step(key)


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
