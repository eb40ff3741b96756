"""laff_gru_encode_train, laff_gru_backward and the differentiable GruTxtEncoder on a real MI355X.

Reference: a CPU torch.nn.GRU in float64 loaded from the encoder's own state dict, with pack_padded_sequence and the reference's pooling,
under autograd (tests/gru_bwd_ref.autograd_grads; CPU nn.GRU does not involve MIOpen).

Rule (the project's own, tests/test_gpu_fuse_backward.py): for the output and for each gradient tensor,
    max |device - f64| / max |f64|  <=  max(4 x the same error of the float32 CPU graph, 1.5e-6).

Kernel-level cases: vocabulary 50 (tokens repeat; ids 45..49 are never drawn: their rows of d_we must be exactly zero), we_dim 20,
H in {32, 96, 256} (K split that leaves waves without a chunk / uneven / even), N in {1, 15, 17, 65} with lengths 1..40 drawn per row, a
row of length 1 and three rows of the maximum length, every pooling mode; and, from laff_gru_backward_plan, the smallest N at which the
64 x 32 tile of the saving forward and of the backward is taken (lengths 2..4).  Reserve, workspace and every output sit in NaN frames.

MEASURED: test_against_float64 prints, per case and tensor, the float32 CPU error, the device error and the fraction of the bound used;
the table at the end of this file lists the largest fraction per tensor as measured on the MI355X.
"""
import functools

import numpy as np
import pytest
import torch

import gru_bwd_ref as R
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL_UNIT = TR.TOL_UNIT
V, V_DRAWN, WE = 50, 45, 20
MODES = [('gru', 'mean'), ('gru', 'last'), ('gru', 'mean_last'), ('bigru', 'mean'), ('bigru', 'last')]
PAD = 64                                             # floats of NaN frame on either side of a buffer


def _big_n(H, ndirs):
    """The smallest N whose first step takes the 64 x 32 tile: 512 tiles of 64 rows x 32 units over the directions of a launch."""
    return (512 // ((H // 32) * ndirs) - 1) * 64 + 1


# (H, N, net, pooling, longest caption)
CASES = [(H, N, net, pooling, 40) for H in (32, 96, 256) for N in (1, 15, 17, 65) for net, pooling in MODES]
BIG = [(32, _big_n(32, 1), 'gru', 'mean_last', 4), (32, _big_n(32, 2), 'bigru', 'mean', 4)]


def _case_id(c):
    return 'H%d-N%d-%s_%s' % c[:4]


def _ndirs(net, pooling):
    return 2 if net == 'bigru' and pooling == 'mean' else 1


def _width(H, net, pooling):
    return H if pooling == 'last' else 2 * H if (pooling == 'mean_last' or net == 'bigru') else H


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs (fp32 values, CPU), the float64 reference and the float32 yardstick of one case: computed once, shared, never written to."""
    H, N, net, pooling, top = c
    bi = net == 'bigru'
    g = np.random.default_rng(1000 * H + 10 * N + MODES.index((net, pooling)))
    lo = 2 if top < 40 else 1
    lens = g.integers(lo, top + 1, N)
    if N > 1:
        lens[0] = lo                                 # top == 40: a row whose first and last step coincide
    if N >= 4:
        lens[-3:] = top                              # several rows share the maximum length
    if N == 1 and H == 32:
        lens[0] = 1
    ids = [g.integers(0, V_DRAWN, L) for L in lens]
    k = 1.0 / H ** 0.5
    sd = {'we.weight': g.normal(0, 1, (V, WE)).astype(np.float32)}
    for sfx in ('_l0', '_l0_reverse') if bi else ('_l0',):
        for name, shape in (('weight_ih', (3 * H, WE)), ('weight_hh', (3 * H, H)), ('bias_ih', (3 * H,)), ('bias_hh', (3 * H,))):
            sd['rnn.%s%s' % (name, sfx)] = g.uniform(-k, k, shape).astype(np.float32)
    dout = g.normal(0, 1, (N, _width(H, net, pooling))).astype(np.float32)
    out64, ref = R.autograd_grads(ids, sd, pooling, bi, dout)
    out32, f32 = R.autograd_grads(ids, sd, pooling, bi, dout, dtype=torch.float32)
    e32 = {k_: R.rel_err(f32[k_], ref[k_]) for k_ in ref}
    e32['out'] = R.rel_err(out32, out64)
    ref = dict(ref, out=out64)
    return dict(H=H, N=N, bi=bi, pooling=pooling, ndirs=_ndirs(net, pooling), ids=ids, sd=sd, dout=dout, ref=ref, e32=e32,
                bound={k_: max(4.0 * e32[k_], TOL_UNIT) for k_ in ref})


def _batch(ids):
    """IdxVec.batch over token ids instead of captions, and the arrays the differentiable encoder adds, on the device."""
    from laff_amd import txt2vec as T
    lens = np.array([len(v) for v in ids], dtype=np.int64)
    perm = np.argsort(-lens, kind='stable').astype(np.int32)
    Tm = int(lens.max())
    tokens = np.zeros((Tm, len(ids)), dtype=np.int32)
    for j, i in enumerate(perm):
        tokens[:lens[i], j] = ids[i]
    slens = lens[perm].astype(np.int32)
    bs = [int((slens > t).sum()) for t in range(Tm)]
    dev = [torch.from_numpy(a).to(DEV) for a in (tokens, slens, perm) + tuple(T.gru_train_arrays(tokens, bs))]
    return T.GruTrainBatch(dev[0], dev[1], dev[2], bs, *dev[3:])


def _device(cs, want_dwe=True, frames=None):
    """The training forward and the backward through ops, as _GruEncodeFn runs them: {'out', state-dict key: gradient} on the device."""
    from laff_amd import ops
    H, bi, pooling, ndirs = cs['H'], cs['bi'], cs['pooling'], cs['ndirs']
    b = cs.get('batch') or _batch(cs['ids'])
    p = cs.get('params') or {k: torch.from_numpy(v).to(DEV) for k, v in cs['sd'].items()}
    dout = cs['dout_dev'] if 'dout_dev' in cs else torch.from_numpy(cs['dout']).to(DEV)
    sfxs = ('_l0', '_l0_reverse')[:ndirs]
    N, M = len(cs['ids']), b.flat.numel()
    new = frames.floats if frames else (lambda *s: torch.empty(*s, device=DEV))
    raw = frames.bytes if frames else (lambda n: torch.empty(max(n, 16), dtype=torch.uint8, device=DEV))
    x = ops.gru_gather_rows(p['we.weight'], b.flat, out=new(M, WE))
    sets = [(ops.fc_act_bn(x, p['rnn.weight_ih' + s], p['rnn.bias_ih' + s]), ops.gru_pack_whh(p['rnn.weight_hh' + s]),
             p['rnn.bias_hh' + s]) for s in sfxs]
    rev = sets[1] if ndirs == 2 else None
    out, reserve = ops.gru_encode_train(b.pos, b.lengths, b.perm, b.batch_sizes, sets[0], rev, pooling,
                                        out=new(N, _width(H, 'bigru' if bi else 'gru', pooling)),
                                        workspace=raw(ops.gru_workspace_bytes(N, H, 1, ndirs == 2, pooling)),
                                        reserve=raw(ops.gru_train_reserve_bytes(M, H, 1, ndirs == 2, pooling)))
    dirs = [(p['rnn.weight_ih' + s], ops.gru_pack_whh_t(p['rnn.weight_hh' + s])) for s in sfxs]
    shapes = ((3 * H, WE), (3 * H, H), (3 * H,), (3 * H,))
    bufs = {'fwd': [new(*s) for s in shapes]}
    if ndirs == 2:
        bufs['rev'] = [new(*s) for s in shapes]
    if want_dwe:
        bufs['d_we'] = new(V, WE)
    ws = raw(ops.gru_backward_workspace_bytes(b.batch_sizes, N, H, WE, 1, ndirs == 2, pooling, want_dwe))
    d_we, gf, gr = ops.gru_backward(dout, b.lengths, b.perm, b.batch_sizes, reserve, x, dirs[0],
                                    dirs[1] if ndirs == 2 else None, pooling,
                                    segments=(b.seg_off, b.seg_tok, b.seg_pos) if want_dwe else None, vocab=V, out=bufs, workspace=ws)
    res = {'out': out, 'we.weight': d_we, 'reserve': reserve}
    for d, s in enumerate(sfxs):
        for k, name in enumerate(('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')):
            res['rnn.%s%s' % (name, s)] = (gf, gr)[d][k]
    return res


def _staged(c):
    """A case with its batch, parameters and dout already on the device: nothing is copied there by a later _device call."""
    cs = dict(_case(c))
    cs['batch'] = _batch(cs['ids'])
    cs['params'] = {k: torch.from_numpy(v).to(DEV) for k, v in cs['sd'].items()}
    cs['dout_dev'] = torch.from_numpy(cs['dout']).to(DEV)
    return cs


WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    print('\nlargest fraction of the bound per tensor:', {k: round(v, 3) for k, v in sorted(WORST.items())})


def _hold(cs, got, label):
    """The error rule on every tensor of a case; prints the figures before it asserts."""
    bad = []
    for k, want in cs['ref'].items():
        if k.endswith('_reverse') and cs['ndirs'] == 1:
            assert k not in got and not np.any(want)          # bigru + last: no gradient here, zeros in torch
            continue
        err = R.rel_err(got[k].cpu().numpy(), want)
        frac = err / cs['bound'][k]
        name = k.replace('_reverse', '').replace('_l0', '')
        WORST[name] = max(WORST.get(name, 0.0), frac)
        print('%s %-24s f32 %.2e  device %.2e  bound %.2e  fraction %.2f' % (label, k, cs['e32'][k], err, cs['bound'][k], frac))
        if not frac <= 1.0:
            bad.append((k, err, cs['bound'][k]))
    assert not bad, bad


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_against_float64(c):
    cs = _case(c)
    fr = TR.Frames(PAD)
    got = _device(cs, frames=fr)
    torch.cuda.synchronize()
    assert fr.intact()
    _hold(cs, got, _case_id(c))
    assert not got['we.weight'][V_DRAWN:].any()                # tokens that no caption used: exactly zero
    unused = np.setdiff1d(np.arange(V), np.concatenate(cs['ids']))
    assert not got['we.weight'][torch.from_numpy(unused).to(DEV)].any()


@pytest.mark.parametrize('c', BIG, ids=_case_id)
def test_large_tile_against_float64(c):
    """The smallest N at which the first launch of the saving forward and the last of the backward take the 64 x 32 tile; a gru's later,
    shorter steps in the same call still take the 16 x 16 one."""
    from laff_amd import ops
    H, N, net, pooling, _ = c
    cs = _staged(c)
    bs = cs['batch'].batch_sizes
    fwd, bwd = ops.gru_backward_plan(bs, H, net == 'bigru', pooling)
    # a bigru launch pairs step i with step T - 1 - i, so every launch has the N rows of one of them; a gru's later steps are shorter
    assert (set(fwd), set(bwd)) == (({1}, {1}) if net == 'bigru' else ({0, 1}, {0, 1})), (fwd, bwd)
    assert fwd[0] == 1 and bwd[-1] == 1
    fewer = ops.gru_backward_plan([min(x, N - 1) for x in bs], H, net == 'bigru', pooling)      # one row less: no launch takes it
    assert set(fewer[0]) == {0} and set(fewer[1]) == {0}
    fr = TR.Frames(PAD)
    got = _device(cs, frames=fr)
    torch.cuda.synchronize()
    assert fr.intact()
    _hold(cs, got, _case_id(c))
    assert not got['we.weight'][V_DRAWN:].any()


def test_every_tile_variant_was_planned():
    from laff_amd import ops
    seen_f, seen_b = set(), set()
    for c in CASES[:1] + BIG:
        H, N, net, pooling, _ = c
        lens = sorted((len(v) for v in _case(c)['ids']), reverse=True)
        bs = [sum(1 for L in lens if L > t) for t in range(lens[0])]
        f, b = ops.gru_backward_plan(bs, H, net == 'bigru', pooling)
        seen_f |= set(f)
        seen_b |= set(b)
    assert seen_f == {0, 1} and seen_b == {0, 1}


PROPERTY_CASES = [(96, 17, net, pooling, 40) for net, pooling in MODES]


@pytest.mark.parametrize('c', PROPERTY_CASES, ids=_case_id)
def test_two_runs_are_bit_identical_and_without_d_we_the_rest_is_the_same_bits(c):
    from laff_amd import ops
    cs = _staged(c)
    a, b = _device(cs), _device(cs)
    fr = TR.Frames(PAD)
    no = _device(cs, want_dwe=False, frames=fr)                # its workspace has no room for dX: none is formed
    torch.cuda.synchronize()
    assert fr.intact()
    N, H, bs = cs['N'], cs['H'], cs['batch'].batch_sizes
    M = sum(bs)
    assert (ops.gru_backward_workspace_bytes(bs, N, H, WE, 1, cs['ndirs'] == 2, cs['pooling'], True) -
            ops.gru_backward_workspace_bytes(bs, N, H, WE, 1, cs['ndirs'] == 2, cs['pooling'], False)) >= cs['ndirs'] * M * WE * 4
    assert no['we.weight'] is None
    for k in a:
        assert torch.equal(a[k], b[k]), k
        if k != 'we.weight':
            assert torch.equal(a[k], no[k]), k


@pytest.mark.parametrize('c', PROPERTY_CASES, ids=_case_id)
def test_training_forward_is_bit_equal_to_the_inference_encode(c):
    from laff_amd import ops
    cs = _staged(c)
    b, p = cs['batch'], cs['params']
    sets = [(ops.fc_act_bn(p['we.weight'], p['rnn.weight_ih' + s], p['rnn.bias_ih' + s]), ops.gru_pack_whh(p['rnn.weight_hh' + s]),
             p['rnn.bias_hh' + s]) for s in ('_l0', '_l0_reverse')[:cs['ndirs']]]
    want = ops.gru_encode(b.tokens, b.lengths, b.perm, b.batch_sizes, sets[0], sets[1] if cs['ndirs'] == 2 else None, cs['pooling'])
    assert torch.equal(_device(cs)['out'], want)


@pytest.mark.parametrize('c', [PROPERTY_CASES[2], PROPERTY_CASES[3]], ids=_case_id)
def test_graph_replay_gives_the_eager_bits(c):
    cs = _staged(c)
    eager = {k: v.clone() for k, v in _device(cs).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _device(cs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _device(cs)
    for v in held.values():
        v.fill_(float('nan')) if v.dtype == torch.float32 else v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(held[k], eager[k]), k


# ---- module level: GruTxtEncoder(differentiable=True) inside a training step made of this library's differentiable pieces ---------
def _vocab(n_words=40):
    from laff_amd import txt2vec as T
    v = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + ['w%d' % i for i in range(n_words)]:
        v.add(w)
    return v


def _captions(g, n, n_words=40, longest=9):
    lens = g.integers(1, longest + 1, n)
    lens[0], lens[-1] = 1, longest
    return [' '.join('w%d' % i for i in g.integers(0, n_words, L)) for L in lens]


class _TextSide(torch.nn.Module):
    """Captions -> GruTxtEncoder -> two TransformNet projections (fc1 + tanh) -> Attention_1 over the two planes."""

    def __init__(self, H, D, bidirectional=False, pooling='mean'):
        super().__init__()
        from laff_amd import txt2vec as T
        from laff_amd.model.Attention import Attention_1
        from laff_amd.model.model import TransformNet
        self.enc = T.GruTxtEncoder(T.IdxVec(_vocab()), 12, H, bidirectional=bidirectional, pooling=pooling, device=DEV,
                                   differentiable=True)
        width = _width(H, 'bigru' if bidirectional else 'gru', pooling)
        self.proj = torch.nn.ModuleList([TransformNet((width, D), batch_norm=False, activation='tanh', dropout=0.0) for _ in range(2)])
        self.att = Attention_1(D, with_ave=True, mul=True)

    def forward(self, caps):
        feat = self.enc({'caption': caps})['text_features']
        return self.att.fuse_planes([p.plane(feat) for p in self.proj])


def _text_side_f64(side, caps, dtype=torch.float64):
    """The same graph on the CPU in `dtype`: (E (B, D), its leaves by parameter name)."""
    import fuse_bwd_ref as FR
    import fuse_ref
    enc = side.enc
    ids = [enc.t2v_idx.encoding(c) for c in caps]
    sd = {k: v.detach().cpu().numpy() for k, v in enc.state_dict().items()}
    feat, leaves = R.torch_encoder(ids, sd, enc.pooling, enc.bigru, dtype)
    leaves = {'enc.' + k: v for k, v in leaves.items()}

    def leaf(name, t):
        leaves[name] = t.detach().cpu().to(dtype).requires_grad_(True)
        return leaves[name]
    planes = torch.stack([torch.tanh(feat @ leaf('proj.%d.fc1.weight' % i, p.fc1.weight).T + leaf('proj.%d.fc1.bias' % i, p.fc1.bias))
                          for i, p in enumerate(side.proj)], 1)
    lin = side.att.embedding_common[0]
    w, b = leaf('att.embedding_common.0.weight', lin.weight), leaf('att.embedding_common.0.bias', lin.bias)
    gw = side.att.global_emb_weight_net.weight.detach().cpu().to(dtype).reshape(1)
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        E = fuse_ref.attention(FR.heads_of(planes, 1, planes.shape[2], True), w.reshape(1, -1), b.reshape(1), gw, with_ave=True, mul=True)[0]
    finally:
        fuse_ref.F64 = keep
    return E.reshape(E.shape[0], -1), leaves


def test_module_training_step_against_float64():
    """16 captions -> GruTxtEncoder(differentiable=True).train() at H = 64 -> TransformNet.train().plane() x 2 -> Attention_1.train()
    .fuse_planes -> loss.MarginRankingLoss against fixed video embeddings -> backward.  Every parameter gradient against the same
    graph in float64 (CPU nn.GRU), element by element, under the bound of tests/test_gpu_fc_backward.py's
    test_end_to_end_two_towers_margin_loss:   max(4 e32, 1.5e-6) max |T|  +  GRAD_ABS sum_j |dT / dE_j|   (tests/train_ref.py).
    Then one laff_amd.optim.Adam step on the encoder's parameters changes them and the next forward sees the new weights."""
    from laff_amd import loss as laff_loss
    from laff_amd import optim as laff_optim
    B, H, D, margin = 16, 64, 32, 0.2
    g = np.random.default_rng(11)
    caps = _captions(g, B)

    def build():
        side = _TextSide(H, D)
        with torch.no_grad():
            for p in side.proj:
                p.fc1.bias.uniform_(-0.2, 0.2)
        vis = torch.randn(B, D)
        with torch.no_grad():
            return (side, vis), _text_side_f64(side, caps)[0], vis
    side, vis = TR.hinge_clear_seed(build, margin, 300)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        E, leaves = _text_side_f64(side, caps, dtype)
        TR.margin_loss_f64(E, vis.to(dtype), margin).backward()
        grads[dtype] = ({k: v.grad.double() for k, v in leaves.items()}, E.detach())
    # sum_j |dT / dE_j| from the float64 graph, one backward per unit vector of E
    absjac = TR.abs_jacobian(*_text_side_f64(side, caps), batched=False)
    # the device
    side.to(DEV).train()
    Ed = side(caps)
    assert Ed.shape == (B, D) and Ed.grad_fn is not None
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    loss = crit(Ed, vis.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    l64 = float(TR.margin_loss_f64(grads[torch.float64][1], vis.double(), margin))
    assert abs(loss.item() - l64) <= 2e-5 * max(1.0, abs(l64))
    got = {n: p.grad for n, p in side.named_parameters()}
    assert got.pop('att.global_emb_weight_net.weight') is None
    ref64, ref32 = grads[torch.float64][0], grads[torch.float32][0]
    assert sorted(got) == sorted(ref64)
    worst = {}
    for n, gt in got.items():
        r = ref64[n]
        if n == 'att.embedding_common.0.bias':
            assert not gt.any()                                          # db of the fusion: exactly zero
            continue
        bound, e32, _ = TR.end_to_end_bound(r, ref32[n], absjac[n])
        ratio = float(((gt.cpu().double() - r).abs() / bound).max())
        worst[n] = ratio
        print('module %-32s e32 %.2e  worst fraction of the bound %.3f' % (n, e32, ratio))
    assert max(worst.values()) <= 1.0, worst
    # one optimizer step on the encoder's parameters, and the next forward sees them
    before = {n: p.detach().clone() for n, p in side.enc.named_parameters()}
    opt = laff_optim.Adam(list(side.enc.parameters()), lr=1e-2)
    opt.step()
    assert all(not torch.equal(p, before[n]) for n, p in side.enc.named_parameters())
    with torch.no_grad():
        side.enc.eval()
        new = side.enc({'caption': caps})['text_features']
        ids = [side.enc.t2v_idx.encoding(c) for c in caps]
        want = R.torch_encoder(ids, {k: v.detach().cpu().numpy() for k, v in side.enc.state_dict().items()}, 'mean', False)[0]
    assert R.rel_err(new.cpu().numpy(), want.detach().numpy()) <= TOL_UNIT
    side.enc.train()
    again = side.enc({'caption': caps})['text_features']
    assert again.grad_fn is not None and torch.equal(again.detach(), new)      # the training forward: same bits, new weights


def test_module_switch_and_what_gets_a_gradient():
    from laff_amd import ops
    from laff_amd import txt2vec as T
    g = np.random.default_rng(3)
    caps = _captions(g, 5)
    # off by default, train mode or not: no graph
    torch.manual_seed(1)
    off = T.GruTxtEncoder(T.IdxVec(_vocab()), 12, 32, device=DEV)
    assert off.training and off({'caption': caps})['text_features'].grad_fn is None
    # bigru + last: the output is the forward half only, and the reverse parameters get no gradient
    torch.manual_seed(1)
    enc = T.GruTxtEncoder(T.IdxVec(_vocab()), 12, 32, bidirectional=True, pooling='last', device=DEV, differentiable=True).train()
    out = enc({'caption': caps})['text_features']
    assert out.shape == (5, 32) and out.grad_fn is not None
    out.square().sum().backward()
    for n, p in enc.named_parameters():
        assert (p.grad is None) == n.endswith('_reverse'), n
    # a frozen embedding: the same bits for the others, and no dX is formed
    real, calls = ops.gru_backward, []

    def spy(*a, **k):
        calls.append(k.get('segments'))
        return real(*a, **k)
    keep = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    enc.zero_grad(set_to_none=True)
    enc.we.weight.requires_grad_(False)
    ops.gru_backward = spy
    try:
        enc({'caption': caps})['text_features'].square().sum().backward()
    finally:
        ops.gru_backward = real
    assert calls == [None] and enc.we.weight.grad is None
    assert all(torch.equal(p.grad, keep[n]) for n, p in enc.named_parameters() if n in keep and n != 'we.weight')
    # eval() or no_grad(): the inference path, bit-equal to the training forward
    with torch.no_grad():
        assert torch.equal(enc({'caption': caps})['text_features'], out)
    assert enc.eval()({'caption': caps})['text_features'].grad_fn is None
    # double backward is refused
    enc.train()
    enc.we.weight.requires_grad_(True)
    o = enc({'caption': caps})['text_features']
    gr, = torch.autograd.grad(o.sum(), enc.rnn.weight_hh_l0, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable|differentiated twice|does not require grad'):
        gr.sum().backward()


# MEASURED on the MI355X (test_against_float64 and test_large_tile_against_float64, 62 cases; errors are max |x - f64| / max |f64|):
#
#   tensor            float32 CPU error      device error           largest fraction of the bound
#   out               8.7e-8 .. 2.4e-7       7.6e-8 .. 2.3e-7       0.15  (H32-N65-gru_mean_last)
#   we.weight         7.2e-8 .. 1.4e-6       7.0e-8 .. 1.3e-6       0.26  (H256-N1-bigru_mean)
#   rnn.weight_ih     6.2e-8 .. 5.5e-6       6.1e-8 .. 6.3e-7       0.31  (H32-N15-bigru_mean)
#   rnn.weight_hh     0 .. 4.0e-7            0 .. 5.2e-7            0.34  (H32-N16321-bigru_mean)
#   rnn.bias_ih       3.8e-8 .. 1.9e-7       4.2e-8 .. 4.3e-7       0.28  (H32-N16321-bigru_mean, reverse)
#   rnn.bias_hh       6.0e-8 .. 3.7e-7       4.6e-8 .. 7.9e-7       0.53  (H32-N16321-bigru_mean: 7.9e-7 against 1.5e-6)
#
# Both arms of the rule are live: the float32 arm decides e.g. rnn.weight_ih at the large-tile cases (4 x 5.5e-6), the 1.5e-6 arm most
# others.  Module level (test_module_training_step_against_float64): largest fraction of the end-to-end bound 0.16 (proj.1.fc1.weight),
# the encoder's own parameters 0.07 .. 0.11.  tools/gru_backward_time.py at N = 128, H = 1024: 0.67 (gru) and 0.81 (bigru) of the bound.
