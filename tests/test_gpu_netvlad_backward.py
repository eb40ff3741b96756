"""laff_netvlad_encode_train, laff_netvlad_backward and the differentiable NetVLADTxtEncoder on a real MI355X.

Reference: tests/netvlad_bwd_ref.netvlad_backward in float64 (itself held to the reference module's CPU autograd at 1e-12 by
tests/test_netvlad_bwd_ref.py).

Rule (the project's own, tests/train_ref.compare): for the output and for each gradient tensor,
    max |device - f64| / max |f64|  <=  max(4 x the same error of the float32 CPU graph, 1.5e-6),
the float32 CPU graph being the reference module restated in torch (netvlad_bwd_ref.torch_module_grads: the module's own bits).

Kernel-level cases: a table of 50 rows (ids repeat across captions; ids 45..49 are never drawn; row 7 is a zero row), every pairing of
K in {1, 5, 32, 64} (no full cluster quad, a ragged quad, the reference's size, the limit) with D in {4, 20, 500, 1024} (one float4,
under a wave of float4s, a partial second wave, four float4s per lane), N in {1, 3, 65} (65: five caption chunks and more than one
chunk of token rows in the parameter stage), caption lengths 1, 8, 9, 17, 40 (under, exactly one and several LDS chunks), captions of
1 and 3 all-zero rows and empty captions.  Reserve, workspace and every output sit in NaN frames.

MEASURED: test_against_float64 prints, per case and tensor, the float32 CPU error, the device error and the fraction of the bound used;
the table at the end of this file lists the largest fraction per tensor as measured on the MI355X.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import netvlad_bwd_ref as B
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL_UNIT = TR.TOL_UNIT
V, V_DRAWN = 50, 45
PAD = 64                                             # floats of NaN frame on either side of a buffer
TENSORS = ('out', 'fc1.weight', 'centeroids')


def _lens65(seed):
    """65 captions: the special lengths, captions of 1 and 3 zero rows (-1, -3), an empty one (0), the rest 1..17 rows."""
    g = np.random.default_rng(seed)
    return (1, 8, 9, 17, 40, -1, -3, 0) + tuple(int(x) for x in g.integers(1, 18, 57))


# (K, D, per caption: rows > 0, 0 = empty, -Z = Z all-zero rows)
CASES = [
    (1, 4, (1,)), (1, 20, (8, -1, 9)), (1, 500, (40, -1, 8)), (1, 1024, (1, 0, 9)),
    (5, 4, (17, 0, 40)), (5, 20, _lens65(1)), (5, 20, (17,)), (5, 500, (9, 1, -3)), (5, 1024, (8,)),
    (32, 4, (40, 17, 1)), (32, 20, (9,)), (32, 500, _lens65(2)), (32, 500, (0, -1, 40)), (32, 1024, (17, 8, 0)),
    (64, 4, (9, -3, 1)), (64, 20, _lens65(3)), (64, 500, (40,)), (64, 1024, (40, 1, 17)), (64, 1024, (-3,)),
]


def _case_id(c):
    return 'K%d-D%d-N%d%s' % (c[0], c[1], len(c[2]), '' if len(c[2]) > 3 else '-' + '_'.join(str(x).replace('-', 'z') for x in c[2]))


@functools.lru_cache(maxsize=None)
def _table(D):
    t = np.random.default_rng(D).normal(0, 1, (V, D)).astype(np.float32)
    t[7] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def _case(c, zero_centroids=()):
    """Inputs (fp32 values, CPU), the float64 reference and the float32 yardstick of one case: computed once, shared, never written to."""
    K, D, lens = c
    g = np.random.default_rng(1000 * K + D + len(lens))
    table = _table(D)
    ids = [g.integers(0, V_DRAWN, max(L, 0)).astype(np.int32) for L in lens]
    zero_rows = np.array([-L if L < 0 else 0 for L in lens], np.int32)
    fc1 = g.normal(0, 1.0 / np.sqrt(D), (K, D)).astype(np.float32)
    cent = g.normal(0, 1.0 / np.sqrt(D), (K, D)).astype(np.float32)
    cent[list(zero_centroids)] = 0.0
    dout = g.normal(0, 1, (len(lens), K * D)).astype(np.float32)
    caps = [table[i] if len(i) else np.zeros((z, D), np.float32) for i, z in zip(ids, zero_rows)]
    out, d_fc1, d_cent = B.netvlad_backward(caps, fc1, cent, dout)
    ref = {'out': out, 'fc1.weight': d_fc1, 'centeroids': d_cent}
    f32 = B.torch_module_grads(caps, fc1, cent, dout, torch.float32)
    e32 = {k: B.rel_err(f32[k], ref[k]) for k in ref}
    return dict(K=K, D=D, N=len(lens), table=table, ids=ids, zero_rows=zero_rows, fc1=fc1, cent=cent, dout=dout, ref=ref, e32=e32,
                bound={k: max(4.0 * e32[k], TOL_UNIT) for k in ref})


def _staged(cs):
    """The case's arrays on the device, as ops takes them: (table, ids, row_off, row_off_host, zero_rows, fc1, cent), dout."""
    row_off = np.concatenate([[0], np.cumsum([len(i) for i in cs['ids']])]).astype(np.int32)
    ids = np.concatenate(cs['ids']) if cs['ids'] else np.zeros(0, np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (t(cs['table']), t(ids.astype(np.int32)), t(row_off), row_off, t(cs['zero_rows']), t(cs['fc1']), t(cs['cent'])), t(cs['dout'])


def _device(cs, want=(True, True), frames=None, staged=None):
    """The saving forward and the backward through ops, as _NetvladEncodeFn runs them, every buffer passed in."""
    from laff_amd import ops
    args, dout = staged or _staged(cs)
    K, D, N, R = cs['K'], cs['D'], cs['N'], args[1].numel()
    new = frames.floats if frames else (lambda *s: torch.full(s, float('nan'), device=DEV))
    raw = frames.bytes if frames else (lambda n: torch.empty(max(n, 16), dtype=torch.uint8, device=DEV))
    out, reserve = ops.netvlad_encode_train(*args, out=new(N, K * D), reserve=raw(ops.netvlad_train_reserve_bytes(N, R, K)))
    bufs = [new(K, D), new(K, D)]
    d_fc1, d_cent = ops.netvlad_backward(dout, out, reserve, *args, want=want, d_fc1=bufs[0], d_centroids=bufs[1],
                                         workspace=raw(ops.netvlad_backward_workspace_bytes(N, R, K, D)))
    assert (d_fc1 is bufs[0]) == bool(want[0]) and (d_cent is bufs[1]) == bool(want[1])
    return {'out': out, 'fc1.weight': bufs[0], 'centeroids': bufs[1]}


WORST = {}


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
    yield
    print('\nlargest fraction of the bound per tensor:', {k: (round(v[0], 3), v[1]) for k, v in sorted(WORST.items())})


def _hold(cs, got, label, tensors=TENSORS):
    """The error rule on every tensor of a case; prints the figures before it asserts."""
    bad = []
    for k in tensors:
        err = B.rel_err(got[k].cpu().numpy(), cs['ref'][k])
        frac = err / cs['bound'][k]
        if frac > WORST.get(k, (0.0, ''))[0]:
            WORST[k] = (frac, label)
        print('%s %-12s f32 %.2e  device %.2e  bound %.2e  fraction %.2f' % (label, k, cs['e32'][k], err, cs['bound'][k], frac))
        if not frac <= 1.0:
            bad.append((k, err, cs['bound'][k]))
    assert not bad, bad


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_against_float64(c):
    from laff_amd import ops
    cs = _case(c)
    fr = TR.Frames(PAD)
    staged = _staged(cs)
    got = _device(cs, frames=fr, staged=staged)
    torch.cuda.synchronize()
    assert fr.intact()
    _hold(cs, got, _case_id(c))
    # the saving forward gives the inference forward's bits
    assert torch.equal(got['out'], ops.netvlad_encode(*staged[0]))
    # and two runs of forward + backward give the same bits
    again = _device(cs, staged=staged)
    for k in TENSORS:
        assert torch.equal(got[k], again[k]), k


def test_fixture_parity(golden):
    """The reference module's own autograd results (tests/golden/netvlad_train.npz) under the same rule, its float32 run the yardstick;
    the rows themselves are the table."""
    z = golden('netvlad_train')
    for c in range(4):
        p = 'c%d/' % c
        lens, zero = z[p + 'lens'], z[p + 'zero']
        off = np.concatenate([[0], np.cumsum(lens)])
        ids = [np.zeros(0, np.int32) if zr else np.arange(off[i], off[i + 1], dtype=np.int32) for i, zr in enumerate(zero)]
        ref, f32 = z.sub(p + 'f64/'), z.sub(p + 'f32/')
        e32 = {k: B.rel_err(f32[k], ref[k]) for k in ref}
        cs = dict(K=z[p + 'fc1'].shape[0], D=z[p + 'fc1'].shape[1], N=len(lens), table=z[p + 'rows'], ids=ids,
                  zero_rows=np.where(zero, lens, 0).astype(np.int32), fc1=z[p + 'fc1'], cent=z[p + 'cent'], dout=z[p + 'dout'], ref=ref,
                  e32=e32, bound={k: max(4.0 * e32[k], TOL_UNIT) for k in ref})
        fr = TR.Frames(PAD)
        got = _device(cs, frames=fr)
        torch.cuda.synchronize()
        assert fr.intact()
        _hold(cs, got, 'fixture-%d' % c)


def test_exact_zeros():
    """An all-empty batch: both gradients exactly zero.  Only zero-row captions: d_fc1 exactly zero, d_centroids the float64 one.
    Empty captions inside a batch add exactly nothing: the bits of the batch without them."""
    got = _device(_case((5, 20, (0, 0, 0))))
    assert not got['out'].any() and not got['fc1.weight'].any() and not got['centeroids'].any()
    cs = _case((5, 20, (-1, -3, -2)))
    got = _device(cs)
    assert not got['fc1.weight'].any() and bool(got['centeroids'].any())
    _hold(cs, got, 'zero-rows-only')
    cs = dict(_case((32, 500, (9, 0, 17, 0))))
    full = _device(cs)
    keep = [0, 2]
    part = dict(cs, N=2, ids=[cs['ids'][i] for i in keep], zero_rows=cs['zero_rows'][keep], dout=cs['dout'][keep])
    sub = _device(part)
    assert not full['out'][1].any() and torch.equal(full['out'][keep], sub['out'])
    assert torch.equal(full['fc1.weight'], sub['fc1.weight']) and torch.equal(full['centeroids'], sub['centeroids'])


def test_no_rows_and_no_captions_give_zeros():
    """R = 0 and N = 0 are legal calls: the gradients come back as zeros."""
    got = _device(_case((5, 20, (0,))))
    assert not got['fc1.weight'].any() and not got['centeroids'].any()
    got = _device(_case((5, 20, ())))
    assert got['out'].shape == (0, 100) and not got['fc1.weight'].any() and not got['centeroids'].any()
    assert not got['fc1.weight'].isnan().any() and not got['centeroids'].isnan().any()


@pytest.mark.parametrize('zero_centroids', [(2,), (0, 1, 2, 3, 4)], ids=['one-row', 'all-rows'])
def test_clamped_branch_against_float64(zero_centroids):
    """A zero centroid row against a caption of all-zero rows: u_k = 0, the norm is clamped and the derivative is dv / eps (with every
    centroid zero, |v| is clamped as well).  d_centroids then holds entries of the order 1e12 and more; the rule is the same."""
    cs = _case((5, 20, (9, -3, 1)), zero_centroids)
    fr = TR.Frames(PAD)
    got = _device(cs, frames=fr)
    torch.cuda.synchronize()
    assert fr.intact()
    assert not got['out'][1].reshape(5, 20)[list(zero_centroids)].any()
    assert float(got['centeroids'][list(zero_centroids)].abs().max()) > 1e9
    _hold(cs, got, 'clamped-%d' % len(zero_centroids))


def test_graph_replay_gives_the_eager_bits():
    cs = _case(CASES[11])                                       # K = 32, D = 500, N = 65
    staged = _staged(cs)
    eager = {k: v.clone() for k, v in _device(cs, staged=staged).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _device(cs, staged=staged)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _device(cs, staged=staged)
    for v in held.values():
        v.fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(held[k], eager[k]), k


@pytest.mark.parametrize('want', [(True, False), (False, True)], ids=['fc1-only', 'centroids-only'])
def test_want_flags(want):
    """Only one gradient requested: the other buffer is not touched, the requested one keeps the bits of the full call."""
    cs = _case(CASES[7])                                        # K = 5, D = 500
    staged = _staged(cs)
    full = _device(cs, staged=staged)
    fr = TR.Frames(PAD)
    got = _device(cs, want=want, frames=fr, staged=staged)
    torch.cuda.synchronize()
    assert fr.intact()
    for flag, k in zip(want, TENSORS[1:]):
        assert torch.equal(got[k], full[k]) if flag else bool(got[k].isnan().all()), k


def test_out_of_table_id_poisons_the_gradients_and_reads_nothing_past_the_table():
    cs = dict(_case(CASES[7]))
    cs['ids'] = [i.copy() for i in cs['ids']]
    cs['ids'][1][0] = V + 5
    cs['ids'][0][3] = -1
    fr = TR.Frames(PAD)
    got = _device(cs, frames=fr)
    torch.cuda.synchronize()
    assert fr.intact()
    assert bool(got['out'][:2].isnan().all()) and bool(torch.isfinite(got['out'][2]).all())
    assert bool(got['fc1.weight'].isnan().all()) and bool(got['centeroids'].isnan().all())


def test_refusals_launch_nothing():
    """K = 65, D = 6, a short reserve and a short workspace on real device buffers, fp16 parameters and a CPU encoder: an error by name,
    and every output keeps its sentinel."""
    from laff_amd import ops
    from laff_amd import txt2vec as T
    cs = _case(CASES[7])
    K, D, N = cs['K'], cs['D'], cs['N']
    (table, ids, ro, roh, zr, fc1, cent), dout = _staged(cs)
    R = ids.numel()
    out = torch.full((N, K * D), 7.0, device=DEV)
    grads = torch.full((2, K, D), 7.0, device=DEV)
    reserve = torch.zeros(ops.netvlad_train_reserve_bytes(N, R, K), dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.netvlad_backward_workspace_bytes(N, R, K, D), dtype=torch.uint8, device=DEV)
    lib, h = ops._context(table.device)
    P = ops._ptr
    r = (C.c_int * len(roh))(*roh)

    def enc(K_=K, D_=D, reserve_bytes=reserve.numel()):
        return lib.laff_netvlad_encode_train(h, P(table), V, D_, P(ids), P(ro), r, P(zr), N, R, P(fc1), P(cent), K_, P(out), K * D,
                                             P(reserve), reserve_bytes, None, 0)

    def bwd(K_=K, D_=D, reserve_bytes=reserve.numel(), ws_bytes=ws.numel(), ldg=K * D):
        return lib.laff_netvlad_backward(h, P(table), V, D_, P(ids), P(ro), r, P(zr), N, R, P(fc1), P(cent), K_, P(out), K * D, P(dout),
                                         ldg, P(reserve), reserve_bytes, P(grads[0]), P(grads[1]), P(ws), ws_bytes)
    assert enc(K_=65) == -5 and enc(D_=6) == -5
    assert enc(reserve_bytes=reserve.numel() - 256) == -1 and b'reserve too small' in lib.laff_last_error()
    assert bwd(K_=65) == -5 and bwd(D_=6) == -5 and bwd(ldg=K * D + 2) == -2
    assert bwd(reserve_bytes=reserve.numel() - 256) == -1 and b'reserve too small' in lib.laff_last_error()
    assert bwd(ws_bytes=ws.numel() - 256) == -1 and b'workspace too small' in lib.laff_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((grads == 7.0).all()) and not reserve.any()
    assert enc() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any()) and not bool((grads == 7.0).any())
    with pytest.raises(ValueError, match='reserve has'):
        ops.netvlad_backward(dout, out, reserve[:64], table, ids, ro, roh, zr, fc1, cent)
    with pytest.raises(ValueError, match='workspace has'):
        ops.netvlad_backward(dout, out, reserve, table, ids, ro, roh, zr, fc1, cent, workspace=ws[:64])
    with pytest.raises(TypeError, match='fc1_weight must be torch.float32'):
        ops.netvlad_encode_train(table, ids, ro, roh, zr, fc1.half(), cent)
    w2v = T.W2Vec(['w%d' % i for i in range(V)], cs['table'])
    half = T.NetVLADTxtEncoder(w2v, num_clusters=K, device=DEV, differentiable=True).half().train()
    with pytest.raises(TypeError, match='fp32 only, netvlad.fc1.weight is torch.float16'):
        half({'caption': ['w1 w2']})
    cpu = T.NetVLADTxtEncoder(w2v, num_clusters=K, device='cpu', differentiable=True).train()
    with pytest.raises(RuntimeError, match='netvlad.fc1.weight is a CPU tensor'):
        cpu({'caption': ['w1 w2']})


# ---- module level: NetVLADTxtEncoder(differentiable=True) inside a training step made of this library's differentiable pieces ------
WORDS = ['w%d' % i for i in range(40)]


def _w2v(Dw, seed=0):
    from laff_amd import txt2vec as T
    table = np.random.default_rng(seed).normal(0, 1, (len(WORDS), Dw)).astype(np.float32)
    return T.W2Vec(WORDS, table, stopwords=('the',))


def _captions(g, n, longest=12):
    caps = [' '.join(str(w) for w in g.choice(WORDS[:36], int(L))) for L in g.integers(1, longest + 1, n)]
    caps[1] = 'zebra the quokka'                                 # no known word: two zero rows
    return caps


def _rows_of(w2v, caps):
    """Each caption's rows as the reference's raw_encoding gives them."""
    table = w2v.table.numpy()
    return [table[ids] if len(ids) else np.zeros((n, table.shape[1]), np.float32) for ids, n in (w2v.raw_ids(c) for c in caps)]


class _TextSide(torch.nn.Module):
    """Captions -> NetVLADTxtEncoder -> one TransformNet projection (fc1 + tanh, no dropout, no BatchNorm)."""

    def __init__(self, K, Dw, D):
        super().__init__()
        from laff_amd import txt2vec as T
        from laff_amd.model.model import TransformNet
        self.enc = T.NetVLADTxtEncoder(_w2v(Dw), num_clusters=K, device=DEV, differentiable=True)
        self.proj = TransformNet((K * Dw, D), batch_norm=False, activation='tanh', dropout=0.0)

    def forward(self, caps):
        return self.proj(self.enc({'caption': caps})['text_features'])


def _text_side_cpu(side, caps, dtype=torch.float64):
    """The same graph on the CPU in `dtype`: (E (B, D), its leaves by parameter name)."""
    v = side.enc.netvlad
    feat, leaves = B.torch_encoder(_rows_of(side.enc.t2v_w2v, caps), v.fc1.weight.detach().cpu().numpy(),
                                   v.centeroids.detach().cpu().numpy(), dtype)
    leaves = {'enc.netvlad.' + k: t for k, t in leaves.items()}
    for name, p in (('proj.fc1.weight', side.proj.fc1.weight), ('proj.fc1.bias', side.proj.fc1.bias)):
        leaves[name] = p.detach().cpu().to(dtype).requires_grad_(True)
    return torch.tanh(feat @ leaves['proj.fc1.weight'].T + leaves['proj.fc1.bias']), leaves


def test_module_training_step_against_float64():
    """12 captions -> NetVLADTxtEncoder(differentiable=True).train() -> TransformNet.train() -> loss.MarginRankingLoss against a random
    video side -> backward.  Every gradient, the two NetVLAD parameters among them, against the same graph in float64 on the CPU, element
    by element, under   max(4 e32, 1.5e-6) max |T|  +  GRAD_ABS sum_j |dT / dE_j|   (tests/train_ref.py)."""
    from laff_amd import loss as laff_loss
    Bn, K, Dw, D, margin = 12, 5, 20, 16, 0.2
    caps = _captions(np.random.default_rng(11), Bn)

    def build():
        side = _TextSide(K, Dw, D)
        with torch.no_grad():
            side.proj.fc1.bias.uniform_(-0.2, 0.2)
        vis = torch.randn(Bn, D)
        with torch.no_grad():
            return (side, vis), _text_side_cpu(side, caps)[0], vis
    side, vis = TR.hinge_clear_seed(build, margin, 500)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        E, leaves = _text_side_cpu(side, caps, dtype)
        TR.margin_loss_f64(E, vis.to(dtype), margin).backward()
        grads[dtype] = ({k: v.grad.double() for k, v in leaves.items()}, E.detach())
    absjac = TR.abs_jacobian(*_text_side_cpu(side, caps), batched=False)
    side.to(DEV).train()
    Ed = side(caps)
    assert Ed.shape == (Bn, D) and Ed.grad_fn is not None
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    loss = crit(Ed, vis.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    l64 = float(TR.margin_loss_f64(grads[torch.float64][1], vis.double(), margin))
    assert abs(loss.item() - l64) <= 2e-5 * max(1.0, abs(l64))
    got = {n: p.grad for n, p in side.named_parameters()}
    ref64, ref32 = grads[torch.float64][0], grads[torch.float32][0]
    assert sorted(got) == sorted(ref64)
    worst = {}
    for n, gt in got.items():
        bound, e32, _ = TR.end_to_end_bound(ref64[n], ref32[n], absjac[n])
        worst[n] = float(((gt.cpu().double() - ref64[n]).abs() / bound).max())
        print('module %-28s e32 %.2e  worst fraction of the bound %.3f' % (n, e32, worst[n]))
    assert max(worst.values()) <= 1.0, worst
    # eval() or no_grad(): the inference path, bit-equal to the training forward; .train() without the switch: no graph
    feat = side.enc({'caption': caps})['text_features']
    assert feat.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(side.enc({'caption': caps})['text_features'], feat)
    assert side.enc.eval()({'caption': caps})['text_features'].grad_fn is None
    side.enc.train().differentiable = False
    assert side.enc({'caption': caps})['text_features'].grad_fn is None


def _laff_model(differentiable, seed=3):
    from laff_amd import txt2vec as T
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    K, Dw = 5, 20
    cfg = make_config({'clip': 128, 'X3D_L': 40}, {'w2v': Dw, 'CLIP': 128, 'NetVLAD': K}, 512, 4, 'LAFF', vis_no_transform=['clip'],
                      txt_no_transform=['CLIP_encoder'], batch_norm=True, with_ave=True, dropout=0)
    torch.manual_seed(seed)
    model = get_model('LAFF', DEV, cfg)
    w2v = _w2v(Dw)
    model.txt_net.encoder.w2v_encoder = T.W2VTxtEncoder(w2v, DEV)
    model.txt_net.encoder.NetVLAD_encoder = T.NetVLADTxtEncoder(w2v, num_clusters=K, device=DEV, differentiable=differentiable)
    return model.train().enable_training()


def _two_steps(model):
    N = 12
    caps = _captions(np.random.default_rng(5), N, longest=8)
    g = torch.Generator().manual_seed(9)
    feats = {'clip': torch.randn(N, 128, generator=g), 'X3D_L': torch.randn(N, 40, generator=g)}
    clip = torch.randn(N, 128, generator=g)
    losses = []
    for _ in range(2):
        items = model({'vis_feats': {k: v.clone().to(DEV) for k, v in feats.items()},
                       'captions': {'caption': caps, 'CLIP_encoding': clip.to(DEV)}, 'vis_frame_feat_dict': {}})
        losses.append(float(items['triplet_loss'].detach()))
    torch.cuda.synchronize()
    return losses


def test_laff_model_trains_its_netvlad_layer():
    """A small 'LAFF' model whose text side includes NetVLAD_encoding, the encoder plugged in: two steps change both NetVLAD parameters,
    the optimizer holds state for them, a second model from the same seed reaches the same bits; with differentiable=False the two
    parameters stay where they were (what every model did before the switch existed)."""
    names = ('txt_net.encoder.NetVLAD_encoder.netvlad.fc1.weight', 'txt_net.encoder.NetVLAD_encoder.netvlad.centeroids')
    model = _laff_model(True)
    params = dict(model.named_parameters())
    assert model.txt_net.encoder_name_list == ['w2v_encoder', 'CLIP_encoder', 'NetVLAD_encoder'] and all(n in params for n in names)
    in_optimizer = {id(p) for gr in model.optimizer.param_groups for p in gr['params']}
    assert all(id(params[n]) in in_optimizer for n in names)
    before = {n: params[n].detach().clone() for n in names}
    losses = _two_steps(model)
    assert all(np.isfinite(x) for x in losses)
    for n in names:
        p = params[n]
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]), n
        assert len(model.optimizer.state[p]) > 0, n
    twin = _laff_model(True)
    assert _two_steps(twin) == losses
    for n, p in twin.named_parameters():
        assert torch.equal(p, params[n]), n
    frozen = _laff_model(False)
    fp = dict(frozen.named_parameters())
    assert all(torch.equal(fp[n], before[n]) for n in names)
    _two_steps(frozen)
    for n in names:
        assert fp[n].grad is None and torch.equal(fp[n], before[n]), n


# MEASURED on the MI355X (test_against_float64, 19 cases; errors are max |x - f64| / max |f64|):
#
#   tensor            float32 CPU error      device error           largest fraction of the bound
#   out               1.3e-8 .. 5.0e-7       6.6e-8 .. 2.7e-7       0.18  (K32-D4-N3-40_17_1)
#   fc1.weight        0 .. 8.1e-7            0 .. 7.7e-7            0.38  (K32-D4-N3-40_17_1)
#   centeroids        6.0e-8 .. 4.7e-7       6.0e-8 .. 2.8e-7       0.18  (K32-D4-N3-40_17_1)
#
# The zeros are the K = 1 cases: with one cluster the softmax is constant and d_fc1 is exactly zero on both sides.  Both arms of the rule
# are live: the float32 arm decides fc1.weight at five cases (e.g. K64-D4: 4 x 8.1e-7), the 1.5e-6 arm the others.  Fixture parity:
# at most 0.30 (fc1.weight); the clamped branches 0.13; module level (test_module_training_step_against_float64): largest fraction of
# the end-to-end bound 0.12 (proj.fc1.weight), the two NetVLAD parameters 0.09 and 0.11.
