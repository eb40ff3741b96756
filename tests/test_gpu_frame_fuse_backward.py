"""laff_frame_fuse_backward, ops.frame_fuse_backward, Attention_1.fuse_frames and the FrameLAFF tower's frame_vector in training mode on a
real MI355X, element by element against float64 autograd of tests/fuse_ref.frame_attention on the very fp32 inputs (tests/frame_bwd_ref.py).

Error of a tensor = max |device - float64| / max |float64| (frame_bwd_ref.rel_err; a float64 tensor that is zero throughout, dw at
Fmax = 1, admits only zeros).  Bound of a case = the larger of
  (i)  4 x the same error of float32 CPU autograd of the restatement on that case, and
  (ii) 1.5e-6, the floor of tests/test_gpu_fuse_backward.py.
db is exactly zero, rows at or past a video's length are exactly zero, a zero-length video gets zero rows.  Before each launch the float64
reference asserts min |g| >= 0.05 over the videos with a frame: it stays clear of the 1 / r singularity by itself.  Inputs come from the
first seed of a case's fixed seed range that clears it, found on the CPU: no case is skipped.

MEASURED: test_backward_vs_float64 prints, per case, the float32 CPU error (i) and the device error of dx and dw; the table at the end of
this file lists them as measured on the MI355X.  Largest device error: dx 5.4e-7 (the std-12 case, bound 1.9e-6), dw 4.5e-7; closest to
a bound: dw at (37, 33, 36) with lens, 4.5e-7 of 1.5e-6 (0.30 x).
"""
import ctypes as C
import functools
import itertools

import pytest
import torch

import frame_bwd_ref as R
import fuse_bwd_ref as FR
import fuse_ref
import train_ref as TR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL_UNIT = TR.TOL_UNIT
NAN = float('nan')
BOTH = (True, True)           # (with_ave, mul): every term of the backward is present
GUARD = 64                    # floats of NaN on either side of every output buffer

# (B, Fmax, d, (with_ave, mul), mode, count, logit scale): the smallest shapes at which each piece can go wrong
_SHAPES = []
_SHAPES += [(37, F, 36, BOTH, 1, None) for F in (1, 3, 4, 5, 32, 33, 65)]     # NCH = 1 requests 8 frames a wave and trip: a wave with no
#                                                                              frame, a partial batch, a whole trip, a second trip
_SHAPES += [(5, 9, d, BOTH, 1, None) for d in (4, 252, 256, 260, 508, 512, 516, 1024)]      # NCH 1 / 2 / 4, partial and whole chunks
_SHAPES += [(3, 200, 1024, BOTH, 1, None)]                                      # the limit of the interface
_SHAPES += [(5, 33, 260, (a, m), 1, None) for a, m in itertools.product((False, True), repeat=2)]
_SHAPES += [(1030, 2, 4, BOTH, 1, None)]                                        # many partial rows in the dw sum
_SHAPES += [(7, 5, 36, BOTH, n, None) for n in (1, 3, 9)]                       # several features a launch; 9: two launches
_SHAPES += [(1, 9, 260, BOTH, 1, None)]
CASES = [(B, F, d, fl, mode, n, sc) for B, F, d, fl, n, sc in dict.fromkeys(_SHAPES) for mode in ('lens', 'full')]
CASES += [(9, 8, 128, BOTH, 'full', 1, 3.0),                                    # peaked softmax: logits of standard deviation 3 in a video
          (9, 8, 128, BOTH, 'full', 1, 12.0)]                                   # near one-hot


def _case_id(c):
    B, F, d, (a, m), mode, n, sc = c
    fl = '+'.join(k for k, v in (('with_ave', a), ('mul', m)) if v) or 'plain'
    return 'B%d-F%d-d%d-%s-%s%s%s' % (B, F, d, fl, mode, '-x%d' % n if n > 1 else '', '' if sc is None else '-std%g' % sc)


def _lens(B, Fmax, g):
    """Lengths 0, 1 and Fmax in one batch where the batch has room for them, anything in [1, Fmax] elsewhere."""
    lens = torch.randint(1, Fmax + 1, (B,), generator=g).to(torch.int32)
    if B == 1:
        lens[0] = (Fmax + 1) // 2
        return lens
    for i, v in enumerate((0, 1, Fmax)[:B]):
        lens[i] = v
    return lens


def _logits(frames, w, mul):
    x = frames.double()
    ws = w.double()[None] * x.sum(1) / x.shape[1] if mul else w.double()[None].expand(x.shape[0], -1)
    return torch.einsum('bfd,bd->bf', x, ws)


def _inputs(B, Fmax, d, flags, mode, scale, seed, lens=None):
    g = torch.Generator().manual_seed(seed)
    frames = (0.5 * torch.randn(B, Fmax, d, generator=g, dtype=torch.float64)).float()
    w = (torch.randn(d, generator=g, dtype=torch.float64) / d ** 0.5).float()
    b = (0.1 * torch.randn(1, generator=g, dtype=torch.float64)).float()
    gw = (0.5 + torch.rand(1, generator=g, dtype=torch.float64)).float()
    dV = torch.randn(B, d, generator=g, dtype=torch.float64).float()              # random: not orthogonal to V
    if lens is None and mode == 'lens':
        lens = _lens(B, Fmax, g)
    if lens is not None:
        frames[torch.arange(Fmax)[None, :] >= lens[:, None]] = NAN                # the buffer past a video's length is never read
    if scale is not None:
        lg = _logits(frames, w, flags[1])
        w = (w.double() * (scale / float((lg - lg.mean(1, keepdim=True)).pow(2).mean().sqrt()))).float()
    return frames, w, b, gw, dV, lens


@functools.lru_cache(maxsize=None)
def _case(c):
    """Inputs (fp32, CPU), the float64 autograd reference and the bounds of one case, per feature: computed once, shared, never written."""
    B, Fmax, d, flags, mode, count, scale = c
    kw = dict(with_ave=flags[0], mul=flags[1])
    feats = []
    base = 7919 * (B + 31 * Fmax) + d + 13 * (flags[0] + 2 * flags[1]) + (5 if mode == 'lens' else 0)
    for k in range(count):
        for seed in range(base + 100 * k, base + 100 * k + 20):
            # (one lens for the features of a launch)
            frames, w, b, gw, dV, lens = _inputs(B, Fmax, d, flags, mode, scale, seed, feats[0]['lens'] if k else None)
            cf = R.closed_form(frames, w, b, gw, dV, lens=lens, **kw)
            live = torch.ones(B, dtype=torch.bool) if lens is None else lens > 0
            if float(cf['g_norm'][live].min()) >= 0.05:
                break
        assert float(cf['g_norm'][live].min()) >= 0.05, c                         # the reference alone stays clear of 1 / r
        ref = R.autograd_grads(frames, w, b, gw, dV, lens=lens, **kw)
        f32 = R.autograd_grads(frames, w, b, gw, dV, lens=lens, dtype=torch.float32, **kw)
        assert R.rel_err(cf['dx'], ref[0]) <= 1e-12 and R.rel_err(cf['dw'], ref[1]) <= 1e-12
        e32 = (R.rel_err(f32[0], ref[0]), R.rel_err(f32[1], ref[1]))
        feats.append(dict(frames=frames, w=w, b=b, gw=gw, dV=dV, lens=lens, ref=ref, e32=e32, top=float(cf['a'].max(1).values.min()),
                          bound=(max(4.0 * e32[0], TOL_UNIT), max(4.0 * e32[1], TOL_UNIT))))
    return dict(B=B, Fmax=Fmax, d=d, kw=kw, lens=feats[0]['lens'], feats=feats)


def _flags(kw):
    from laff_amd import ops
    return ops.attention_flags(kw['with_ave'], kw['mul'])


def _table(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class _Launch:
    """One laff_frame_fuse_backward call through the C ABI on the case's inputs; every output sits in a NaN-filled frame."""

    def __init__(self, cs, want_dw=True, pitch=None):
        from laff_amd import ops
        self.cs, self.want_dw = cs, want_dw
        B, Fmax, d, n = cs['B'], cs['Fmax'], cs['d'], len(cs['feats'])
        self.n = n
        self.frames = [f['frames'].to(DEV) for f in cs['feats']]
        self.params = [(f['w'].to(DEV), f['b'].to(DEV), f['gw'].to(DEV)) for f in cs['feats']]
        self.lens = None if cs['lens'] is None else cs['lens'].to(DEV)
        self.lddv = d if pitch is None else pitch
        self.grads = []
        for f in cs['feats']:
            g = torch.full((B, self.lddv), NAN, device=DEV)
            g[:, :d] = f['dV'].to(DEV)
            self.grads.append(g)
        self.fr = TR.Frames(GUARD)
        self.df = [self.fr.floats(B * Fmax * d) for _ in range(n)]
        self.dw = [self.fr.floats(d) for _ in range(n)]
        self.db = [self.fr.floats(4) for _ in range(n)]                           # (db is its first float; the rest stays NaN)
        self.nbytes = ops.frame_fuse_backward_plan(n, B, Fmax, d, want_dw)[0]
        self.ws = self.fr.floats(max(self.nbytes // 4, 4))
        self.tables = (_table(self.frames), _table([p[0] for p in self.params]), _table([p[1] for p in self.params]),
                       _table([p[2] for p in self.params]), _table(self.grads), _table(self.df), _table(self.dw), _table(self.db))

    def run(self):
        from laff_amd import ops
        cs = self.cs
        lib, h = ops._context(torch.device(DEV, torch.cuda.current_device()))
        F, W, Bb, G, DV, DF, DW, DB = self.tables
        ops.check(lib.laff_frame_fuse_backward(h, self.n, F, ops._ptr(self.lens), cs['B'], cs['Fmax'], cs['d'], W, Bb, G, _flags(cs['kw']),
                                               DV, self.lddv, DF, DW if self.want_dw else None, DB if self.want_dw else None,
                                               ops._ptr(self.ws), self.nbytes))
        return self

    def outputs(self):
        torch.cuda.synchronize()
        cs = self.cs
        return ([v.view(cs['B'], cs['Fmax'], cs['d']) for v in self.df], list(self.dw), [v[:1] for v in self.db])

    def guards_intact(self):
        torch.cuda.synchronize()
        return self.fr.intact() and all(bool(torch.isnan(v[1:]).all()) for v in self.db)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check(cs, dfs, dws, dbs, label):
    B, Fmax = cs['B'], cs['Fmax']
    pad = torch.zeros(B, Fmax, dtype=torch.bool) if cs['lens'] is None else torch.arange(Fmax)[None, :] >= cs['lens'][:, None]
    worst = 0.0
    for k, f in enumerate(cs['feats']):
        dx, dw, db = dfs[k].cpu(), dws[k].cpu(), dbs[k].cpu()
        assert torch.isfinite(dx).all() and torch.isfinite(dw).all(), label
        assert not dx[pad].any(), label                                  # padded rows and zero-length videos: exactly zero
        assert tuple(db.shape) == (1,) and not db.any(), label           # exactly zero
        if Fmax == 1:
            assert not dw.any(), label                                   # a softmax over one logit is constant
        e_dx, e_dw = R.rel_err(dx, f['ref'][0]), R.rel_err(dw, f['ref'][1])
        print('%-40s fp32 CPU dx %.2e dw %.2e | device dx %.2e (bound %.2e) dw %.2e (bound %.2e) | min top weight %.4f'
              % (label + ('[%d]' % k if len(cs['feats']) > 1 else ''), f['e32'][0], f['e32'][1], e_dx, f['bound'][0], e_dw, f['bound'][1],
                 f['top']))
        assert e_dx <= f['bound'][0] and e_dw <= f['bound'][1], (label, k, e_dx, f['bound'][0], e_dw, f['bound'][1])
        worst = max(worst, e_dx / f['bound'][0], e_dw / f['bound'][1])
    return worst


@pytest.mark.parametrize('c', CASES, ids=_case_id)
def test_backward_vs_float64(c):
    from laff_amd import ops
    cs = _case(c)
    d = cs['d']
    first = _Launch(cs).run()
    dfs, dws, dbs = first.outputs()
    _check(cs, dfs, dws, dbs, _case_id(c))
    assert first.guards_intact()                                         # nothing outside the outputs and the workspace was written
    # a second call: the same bits
    again = _Launch(cs).run()
    assert all(_same(a, b) for a, b in zip(again.outputs(), (dfs, dws, dbs))) and again.guards_intact()
    # without dw: the same dframes, dw / db / the workspace untouched
    nodw = _Launch(cs, want_dw=False).run()
    o = nodw.outputs()
    assert _same(o[0], dfs) and nodw.guards_intact()
    assert all(bool(torch.isnan(t).all()) for t in o[1] + o[2]) and bool(torch.isnan(nodw.ws).all())
    # a gradient with a wider row pitch: the same bits as its dense copy
    wide = _Launch(cs, pitch=d + 8).run()
    assert all(_same(a, b) for a, b in zip(wide.outputs(), (dfs, dws, dbs))) and wide.guards_intact()
    # one call captured in a graph and replayed: the eager bits
    cap = _Launch(cs)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode='thread_local'):
        cap.run()
    gr.replay()
    assert all(_same(a, b) for a, b in zip(cap.outputs(), (dfs, dws, dbs))) and cap.guards_intact()
    # ops.frame_fuse_backward: the same bits again, into caller-owned buffers and into its own
    outs = [torch.full((cs['B'], cs['Fmax'], d), NAN, device=DEV) for _ in cs['feats']]
    for out in (outs, None):
        r = ops.frame_fuse_backward(first.frames, first.lens, first.params, _flags(cs['kw']), [g[:, :d] for g in wide.grads], out=out)
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(r, (dfs, dws, dbs)))
        assert out is None or all(a is b for a, b in zip(r[0], out))
    r = ops.frame_fuse_backward(first.frames, first.lens, first.params, _flags(cs['kw']), first.grads, want_param_grads=False)
    assert r[1] is None and r[2] is None and _same(r[0], dfs)


def test_peaked_cases_are_peaked():
    for sc in (3.0, 12.0):
        f = _case(next(c for c in CASES if c[6] == sc))['feats'][0]
        lg = _logits(f['frames'], f['w'], True)
        assert abs(float((lg - lg.mean(1, keepdim=True)).pow(2).mean().sqrt()) - sc) < 0.05 * sc
    a = torch.softmax(lg + float(f['b']), 1)
    top = a.max(1).values
    assert float(top.median()) > 0.95 and float(top.max()) > 0.9999     # near one-hot: the typical video gives one frame all but 5 %


def test_lens_cases_hold_the_three_lengths_and_nan_padding():
    for c in CASES:
        cs = _case(c)
        if c[4] == 'full':
            assert cs['lens'] is None and all(torch.isfinite(f['frames']).all() for f in cs['feats'])
            continue
        lens, Fmax = cs['lens'], cs['Fmax']
        if cs['B'] >= 3:
            assert {0, 1, Fmax} <= set(lens.tolist())
        pad = torch.arange(Fmax)[None, :] >= lens[:, None]
        for f in cs['feats']:
            assert torch.isnan(f['frames'][pad]).all() and torch.isfinite(f['frames'][~pad]).all()


def test_empty_batch_and_no_features_touch_nothing():
    from laff_amd import ops
    lib, h = ops._context(torch.device(DEV, torch.cuda.current_device()))
    fr = TR.Frames(GUARD)
    buf = fr.floats(64)
    whole = fr.held[0][0]
    t = _table([buf])
    for count, B in ((1, 0), (0, 4)):
        assert lib.laff_frame_fuse_backward(h, count, t, None, B, 2, 8, t, t, t, 3, t, 8, t, t, t, ops._ptr(buf), 0) == 0
        assert lib.laff_frame_fuse_backward(h, count, None, None, B, 2, 8, None, None, None, 3, None, 8, None, None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all())
    w, b, gw = torch.zeros(8, device=DEV), torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    dfs, dws, dbs = ops.frame_fuse_backward([torch.empty(0, 2, 8, device=DEV)], None, [(w, b, gw)], 3, [torch.empty(0, 8, device=DEV)])
    assert tuple(dfs[0].shape) == (0, 2, 8) and not dws[0].any() and not dbs[0].any() and tuple(dws[0].shape) == (8,)
    # refused before any GPU work, with a real ctx: a misaligned base, a workspace that is too small
    x = torch.zeros(2 * 2 * 8 + 4, device=DEV)
    good, off = _table([x[:32]]), _table([x[1:33]])
    assert lib.laff_frame_fuse_backward(h, 1, off, None, 2, 2, 8, t, t, t, 3, t, 8, good, None, None, None, 0) == -3
    assert lib.laff_frame_fuse_backward(h, 1, good, None, 2, 2, 8, t, t, t, 3, t, 8, good, t, t, ops._ptr(buf), 8) == -1
    assert b'workspace' in lib.laff_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(whole).all()) and not x.any()


# ---- the modules in training mode ---------------------------------------------------------------------------------------------------
def _bound(got, r64, r32):
    e = R.rel_err(got, r64)
    return e, max(4.0 * R.rel_err(r32, r64), TOL_UNIT)


@pytest.mark.parametrize('with_ave,mul', list(itertools.product((False, True), repeat=2)))
def test_attention_1_fuse_frames_train(with_ave, mul):
    from laff_amd import ops
    from laff_amd.model.Attention import Attention_1
    torch.manual_seed(11 + 2 * with_ave + mul)
    B, Fmax, d = 6, 5, 36
    m = Attention_1(d, with_ave=with_ave, mul=mul).to(DEV).train()
    m.change_raw_global_emb_weight(0.7)
    lens = torch.tensor([0, 1, 5, 3, 2, 4], dtype=torch.int32)
    x = 0.5 * torch.randn(B, Fmax, d)
    x[torch.arange(Fmax)[None, :] >= lens[:, None]] = NAN
    dV = torch.randn(B, d)
    lin = m.embedding_common[0]
    args = (x, lin.weight.detach().cpu().reshape(-1), lin.bias.detach().cpu(), torch.tensor([0.7]), dV)
    kw = dict(with_ave=with_ave, mul=mul, lens=lens)
    assert float(R.closed_form(*args, **kw)['g_norm'][lens > 0].min()) >= 0.05
    r64, r32 = R.autograd_grads(*args, **kw), R.autograd_grads(*args, dtype=torch.float32, **kw)
    xd = x.to(DEV).requires_grad_(True)
    V = m.fuse_frames(xd, lens.to(DEV))
    assert V.shape == (B, d) and V.requires_grad
    w, b, gw = m._params()
    assert torch.equal(V.detach(), ops.frame_fuse(xd.detach(), lens.to(DEV), w.reshape(-1), b, gw, ops.attention_flags(with_ave, mul)))
    V.backward(dV.to(DEV))
    torch.cuda.synchronize()
    for name, got, k in (('frames', xd.grad, 0), ('weight', lin.weight.grad.reshape(-1), 1)):
        e, bound = _bound(got.cpu(), r64[k], r32[k])
        print('fuse_frames with_ave=%d mul=%d %-7s device %.2e (bound %.2e)' % (with_ave, mul, name, e, bound))
        assert e <= bound
    assert torch.isfinite(xd.grad).all() and not xd.grad[0].any() and not xd.grad[1, 1:].any()
    assert tuple(lin.bias.grad.shape) == (1,) and not lin.bias.grad.any() and m.global_emb_weight_net.weight.grad is None
    # frames that need no gradient: the parameters still get theirs, the same bits
    gw_bits = lin.weight.grad.clone()
    m.zero_grad()
    m.fuse_frames(x.to(DEV), lens.to(DEV)).backward(dV.to(DEV))
    assert torch.equal(lin.weight.grad, gw_bits)
    # eval mode: no graph, the bits of ops.frame_fuse
    m.eval()
    Ve = m.fuse_frames(xd, lens.to(DEV))
    assert not Ve.requires_grad and torch.equal(Ve, V.detach())


def _tower(add_fc, frame_feats, vid_dims=None, D=128, H=2, att='attention_averageMul'):
    from laff_amd.config import make_config
    from laff_amd.model.model import get_model
    cfg = make_config(vid_dims or {}, {'bow': 8}, D, H, 'FrameLAFF', frame_feats=frame_feats, batch_norm=False, dropout=0.0,
                      vis_frame_attention=att, vis_frame_addFC=add_fc, frame_feat_with_video_feat=bool(vid_dims), with_ave=True, mul=True)
    return get_model('FrameLAFF', DEV, cfg).vis_net


def _frame_vector_ref(x, mask, fc, att, dV, dtype, add_fc):
    """Linear (with add_fc) -> frame attention as a CPU torch graph in `dtype`: gradients of sum(V dV) by name, in float64."""
    leaves = {'frames': x.detach().cpu().to(dtype).requires_grad_(True),
              'att.weight': att.embedding_common[0].weight.detach().cpu().to(dtype).reshape(-1).requires_grad_(True)}
    y, lens = leaves['frames'], None
    if add_fc:
        leaves['fc.weight'] = fc.weight.detach().cpu().to(dtype).requires_grad_(True)
        leaves['fc.bias'] = fc.bias.detach().cpu().to(dtype).requires_grad_(True)
        y = y @ leaves['fc.weight'].T + leaves['fc.bias']
    else:
        lens = mask.sum(1).to(torch.int32)
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        V = fuse_ref.frame_attention(y, leaves['att.weight'], att.embedding_common[0].bias.detach().cpu().to(dtype),
                                     att.global_emb_weight_net.weight.detach().cpu().to(dtype), with_ave=att.with_ave, mul=att.mul, lens=lens)
    finally:
        fuse_ref.F64 = keep
    (V * dV.to(dtype)).sum().backward()
    return V.detach().double(), {k: v.grad.double() for k, v in leaves.items()}


@pytest.mark.parametrize('add_fc', (False, True), ids=('noFC', 'addFC'))
def test_tower_frame_vector_train(add_fc):
    from laff_amd import ops
    torch.manual_seed(31 + add_fc)
    B, Fmax, d = 6, 5, 36
    tower = _tower(add_fc, {'clip_frame': d}).train()
    seq = tower.frame_attention['clip_frame']
    att, fc = seq[-1], (seq[0] if add_fc else None)
    assert len(seq) == (2 if add_fc else 1)
    lens = torch.tensor([1, 5, 3, 2, 4, 5])
    mask = (torch.arange(Fmax)[None, :] < lens[:, None]).float()
    x = 0.5 * torch.randn(B, Fmax, d) * mask[:, :, None]                # zero padded, as the data loader leaves it
    dV = torch.randn(B, d)
    V64, r64 = _frame_vector_ref(x, mask, fc, att, dV, torch.float64, add_fc)
    assert float(V64.norm(dim=1).min()) > 0.99
    _, r32 = _frame_vector_ref(x, mask, fc, att, dV, torch.float32, add_fc)
    xd = x.to(DEV).requires_grad_(True)
    V = tower.frame_vector('clip_frame', xd, mask.to(DEV))
    assert V.requires_grad and R.rel_err(V.detach().cpu(), V64) <= TOL_UNIT
    V.backward(dV.to(DEV))
    torch.cuda.synchronize()
    got = {'frames': xd.grad, 'att.weight': att.embedding_common[0].weight.grad.reshape(-1)}
    if add_fc:
        got.update({'fc.weight': fc.weight.grad, 'fc.bias': fc.bias.grad})
    assert sorted(got) == sorted(r64)
    for n, g in got.items():
        e, bound = _bound(g.cpu(), r64[n], r32[n])
        print('frame_vector %s %-10s device %.2e (bound %.2e)' % ('addFC' if add_fc else 'noFC', n, e, bound))
        assert e <= bound, (n, e, bound)
    assert not att.embedding_common[0].bias.grad.any() and att.global_emb_weight_net.weight.grad is None
    # prepare and forward stay eval-only
    with pytest.raises(NotImplementedError, match='inference path only'):
        tower.prepare({}, {'clip_frame': x.to(DEV), 'mask_tensor': mask.to(DEV)})
    # eval mode: the launches and the bits of the path before this method was differentiable
    tower.eval()
    with torch.no_grad():
        Ve = tower.frame_vector('clip_frame', x.to(DEV), mask.to(DEV))
        w, b, gw = att._params()
        fr, ln = x.to(DEV), mask.to(DEV).sum(dim=1).to(torch.int32)
        if add_fc:
            fr, ln = ops.fc_act_bn(fr.view(B * Fmax, d), fc.weight.detach(), fc.bias.detach()).view(B, Fmax, d), None
        want = ops.frame_fuse(fr, ln, w.reshape(-1), b, gw, ops.attention_flags(att.with_ave, att.mul))
    assert not Ve.requires_grad and torch.equal(Ve, want)


# ---- end to end: frame features in front of a LAFF tower's training step ------------------------------------------------------------
def _video_side_device(tower, feats, mask):
    """frame_vector -> TransformNet.plane -> the tower's fusion block, the pieces prepare() strings together in eval mode."""
    planes = [getattr(tower, n).plane(tower.frame_vector(n, x, mask)) for n, x in feats.items()]
    return tower.vis_attention_layer.fuse_planes(planes)


def _video_side_ref(tower, feats, mask, dtype=torch.float64):
    """The same side as a CPU torch graph in `dtype`: (E (B, H, d), its leaves under the tower's parameter names)."""
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().cpu().to(dtype).requires_grad_(True)
        return leaves[name]
    lens = mask.sum(1).to(torch.int32)
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        planes = []
        for n, x in feats.items():
            att, net = tower.frame_attention[n][-1], getattr(tower, n)
            pre = 'frame_attention.%s.0.' % n
            V = fuse_ref.frame_attention(leaf('frames.' + n, x), leaf(pre + 'embedding_common.0.weight', att.embedding_common[0].weight).reshape(-1),
                                         att.embedding_common[0].bias.detach().cpu().to(dtype),
                                         att.global_emb_weight_net.weight.detach().cpu().to(dtype), with_ave=att.with_ave, mul=att.mul, lens=lens)
            planes.append(torch.tanh(V @ leaf(n + '.fc1.weight', net.fc1.weight).T + leaf(n + '.fc1.bias', net.fc1.bias)))
        heads = list(tower.vis_attention_layer.attention_layer)
        pre = 'vis_attention_layer.attention_layer.%d.embedding_common.0.'
        w = torch.stack([leaf((pre % h) + 'weight', a.embedding_common[0].weight).reshape(-1) for h, a in enumerate(heads)])
        b = torch.cat([leaf((pre % h) + 'bias', a.embedding_common[0].bias).reshape(1) for h, a in enumerate(heads)])
        gw = torch.cat([a.global_emb_weight_net.weight.detach().cpu().to(dtype).reshape(1) for a in heads])
        P = torch.stack(planes, 1)
        H = len(heads)
        E = fuse_ref.attention(FR.heads_of(P, H, P.shape[2] // H, True), w, b, gw, with_ave=True, mul=True, l2norm_each_head=False)[0]
    finally:
        fuse_ref.F64 = keep
    return E, leaves


def test_end_to_end_frame_features_margin_loss():
    """B = 16, Fmax = 5, d = 64, two frame features, H = 2 heads of 64: frame_vector (Attention_1 with_ave + mul over the frames, lens
    from the mask) -> TransformNet.train().plane (fc1 + tanh) -> Multi_head_MyApply_Attention.train().fuse_planes ->
    loss.MarginRankingLoss against text embeddings that are a leaf -> backward.  Every parameter gradient, the frames' and the text
    embeddings' gradients against the same graph in float64.

    Bound of a gradient tensor T, element by element:  max(4 e32, 1.5e-6) max |T|  +  GRAD_ABS sum_j |dT / dE_j|
    (tests/test_gpu_fuse_backward.py::test_end_to_end_two_towers_margin_loss: e32 the error of the whole graph in float32 CPU autograd,
    the second term the margin loss's own contract carried to T through the absolute values of the side's Jacobian; for the text
    embeddings, which the loss differentiates directly, that Jacobian is the identity)."""
    from laff_amd import loss as laff_loss
    B, Fmax, d, H, D, margin = 16, 5, 64, 2, 128, 0.2
    lens = torch.tensor([1, 5, 3, 2, 4, 5, 1, 2, 3, 4, 5, 5, 2, 3, 4, 1])
    mask = (torch.arange(Fmax)[None, :] < lens[:, None]).float()
    def build():
        tower = _tower(False, {'fa': d, 'fb': d}, D=D, H=H)
        with torch.no_grad():
            for n in ('fa', 'fb'):
                getattr(tower, n).fc1.bias.uniform_(-0.2, 0.2)
        z = torch.randn(B, 1, 8)
        feats = {n: (0.5 * (z @ torch.randn(8, d)) + 0.5 * torch.randn(B, Fmax, d)) * mask[:, :, None] for n in ('fa', 'fb')}
        Et = torch.randn(B, H, D // H)
        with torch.no_grad():
            return (tower, feats, Et), Et, _video_side_ref(tower, feats, mask)[0]
    tower, feats, Et = TR.hinge_clear_seed(build, margin, 300)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        Ev, lv = _video_side_ref(tower, feats, mask, dtype)
        t = Et.detach().clone().to(dtype).requires_grad_(True)
        TR.margin_loss_f64(t, Ev, margin).backward()
        grads[dtype] = dict({k: v.grad.double() for k, v in lv.items()}, text=t.grad.double())
        if dtype == torch.float64:
            l64 = float(TR.margin_loss_f64(t.detach(), Ev.detach(), margin))
    # sum_j |dT / dE_j| of the video side, from the float64 graph: one batched backward over the unit vectors of E
    absjac = TR.abs_jacobian(*_video_side_ref(tower, feats, mask))
    absjac['text'] = torch.ones(B, H, D // H, dtype=torch.float64)
    # the device
    tower = tower.train()
    dfe = {n: x.to(DEV).requires_grad_(True) for n, x in feats.items()}
    td = Et.detach().to(DEV).requires_grad_(True)
    Ev = _video_side_device(tower, dfe, mask.to(DEV))
    assert Ev.shape == (B, H, D // H)
    crit = laff_loss.MarginRankingLoss(margin=margin, max_violation=False, cost_style='sum', direction='bidir')
    loss = crit(td, Ev)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - l64) <= 2e-5 * max(1.0, abs(l64))
    got = {n: p.grad for n, p in tower.named_parameters()}
    got.update({'frames.' + n: x.grad for n, x in dfe.items()})
    got['text'] = td.grad
    for n in list(got):
        if n.endswith('global_emb_weight_net.weight') or 'layer_norm' in n:
            assert got.pop(n) is None, n                                  # gw: no gradient; layer_norm: declared and unused
        elif n.startswith('frame_attention') and n.endswith('embedding_common.0.bias'):
            assert not got.pop(n).any(), n                                # db of the frame attention: exactly zero
    ref64, ref32 = grads[torch.float64], grads[torch.float32]
    assert sorted(got) == sorted(ref64)
    worst = 0.0
    pad = (mask == 0)
    for n, g in got.items():
        r = ref64[n]
        if n.endswith('embedding_common.0.bias'):
            assert not g.any(), n                                         # db of the fusion: exactly zero
            continue
        if n.startswith('frames.'):
            assert not g.cpu()[pad].any(), n                              # padded frames: exactly zero
        bound, e32, top = TR.end_to_end_bound(r, ref32[n], absjac[n])
        err = (g.cpu().double().reshape(r.shape) - r).abs()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        print('%-62s max |g| %.3e  err %.3e  fp32 CPU %.2e  bound %.3e .. %.3e  worst err / bound %.3f'
              % (n, top, float(err.max()), e32, float(bound.min()), float(bound.max()), ratio))
        assert ratio <= 1.0, (n, ratio)
    print('end to end: worst err / bound %.3f' % worst)


# MEASURED on the MI355X by test_backward_vs_float64, per case (with several features: the worst of them): the error of float32 CPU
# autograd against float64 (i), and the device's error beside the bound it was held to, for dx and for dw.  The float32 CPU figures, and
# with them the bounds above 1.5e-6, depend a little on the CPU that runs them; these are from the GPU host.  Largest device error: dx
# 5.4e-7 in the std-12 case (bound 1.9e-6), dw 4.5e-7 at (37, 33, 36) with lens, which is also the largest used fraction of a bound
# (0.30).  Modules: fuse_frames at most 2.9e-7 (weight), frame_vector at most 2.8e-7 (the attention's weight behind the frame Linear),
# all under 1.5e-6.  End to end: the worst element used 0.40 of its bound.
#   case                                     fp32 CPU dx, dw      device dx (bound)              device dw (bound)
#   B37-F1-d36-with_ave+mul-lens             8.71e-08 0.00e+00   1.33e-07 (1.50e-06)            0.00e+00 (1.50e-06)
#   B37-F1-d36-with_ave+mul-full             8.17e-08 0.00e+00   6.72e-08 (1.50e-06)            0.00e+00 (1.50e-06)
#   B37-F3-d36-with_ave+mul-lens             1.16e-07 2.99e-07   1.15e-07 (1.50e-06)            2.06e-07 (1.50e-06)
#   B37-F3-d36-with_ave+mul-full             1.05e-07 1.49e-07   1.54e-07 (1.50e-06)            3.70e-07 (1.50e-06)
#   B37-F4-d36-with_ave+mul-lens             1.11e-07 1.66e-07   1.20e-07 (1.50e-06)            2.04e-07 (1.50e-06)
#   B37-F4-d36-with_ave+mul-full             1.16e-07 2.33e-07   1.41e-07 (1.50e-06)            2.30e-07 (1.50e-06)
#   B37-F5-d36-with_ave+mul-lens             7.64e-08 1.23e-07   1.33e-07 (1.50e-06)            2.24e-07 (1.50e-06)
#   B37-F5-d36-with_ave+mul-full             1.71e-07 1.74e-07   1.71e-07 (1.50e-06)            1.95e-07 (1.50e-06)
#   B37-F32-d36-with_ave+mul-lens            8.70e-08 3.29e-07   8.29e-08 (1.50e-06)            2.22e-07 (1.50e-06)
#   B37-F32-d36-with_ave+mul-full            1.35e-07 2.70e-07   1.35e-07 (1.50e-06)            2.42e-07 (1.50e-06)
#   B37-F33-d36-with_ave+mul-lens            9.83e-08 2.04e-07   7.85e-08 (1.50e-06)            4.50e-07 (1.50e-06)
#   B37-F33-d36-with_ave+mul-full            1.65e-07 2.14e-07   1.82e-07 (1.50e-06)            1.48e-07 (1.50e-06)
#   B37-F65-d36-with_ave+mul-lens            8.62e-08 1.55e-07   8.63e-08 (1.50e-06)            2.40e-07 (1.50e-06)
#   B37-F65-d36-with_ave+mul-full            1.38e-07 2.26e-07   1.78e-07 (1.50e-06)            2.32e-07 (1.50e-06)
#   B5-F9-d4-with_ave+mul-lens               9.13e-08 1.23e-07   7.72e-08 (1.50e-06)            1.87e-07 (1.50e-06)
#   B5-F9-d4-with_ave+mul-full               3.67e-07 1.70e-07   2.58e-07 (1.50e-06)            1.72e-07 (1.50e-06)
#   B5-F9-d252-with_ave+mul-lens             1.01e-07 9.25e-08   8.27e-08 (1.50e-06)            9.29e-08 (1.50e-06)
#   B5-F9-d252-with_ave+mul-full             1.35e-07 2.03e-07   1.18e-07 (1.50e-06)            2.03e-07 (1.50e-06)
#   B5-F9-d256-with_ave+mul-lens             1.30e-07 1.84e-07   8.27e-08 (1.50e-06)            1.83e-07 (1.50e-06)
#   B5-F9-d256-with_ave+mul-full             1.07e-07 1.45e-07   1.65e-07 (1.50e-06)            1.44e-07 (1.50e-06)
#   B5-F9-d260-with_ave+mul-lens             8.51e-08 2.14e-07   1.46e-07 (1.50e-06)            1.64e-07 (1.50e-06)
#   B5-F9-d260-with_ave+mul-full             1.58e-07 1.96e-07   1.56e-07 (1.50e-06)            1.61e-07 (1.50e-06)
#   B5-F9-d508-with_ave+mul-lens             9.86e-08 2.80e-07   7.13e-08 (1.50e-06)            1.80e-07 (1.50e-06)
#   B5-F9-d508-with_ave+mul-full             1.70e-07 2.65e-07   1.46e-07 (1.50e-06)            2.56e-07 (1.50e-06)
#   B5-F9-d512-with_ave+mul-lens             1.04e-07 3.88e-07   9.36e-08 (1.50e-06)            2.86e-07 (1.55e-06)
#   B5-F9-d512-with_ave+mul-full             1.29e-07 2.92e-07   1.44e-07 (1.50e-06)            1.63e-07 (1.50e-06)
#   B5-F9-d516-with_ave+mul-lens             1.39e-07 3.49e-07   8.91e-08 (1.50e-06)            2.03e-07 (1.50e-06)
#   B5-F9-d516-with_ave+mul-full             1.12e-07 2.52e-07   1.46e-07 (1.50e-06)            1.60e-07 (1.50e-06)
#   B5-F9-d1024-with_ave+mul-lens            1.06e-07 2.69e-07   7.77e-08 (1.50e-06)            1.50e-07 (1.50e-06)
#   B5-F9-d1024-with_ave+mul-full            1.17e-07 4.14e-07   1.13e-07 (1.50e-06)            1.75e-07 (1.66e-06)
#   B3-F200-d1024-with_ave+mul-lens          6.92e-08 2.44e-07   1.18e-07 (1.50e-06)            2.70e-07 (1.50e-06)
#   B3-F200-d1024-with_ave+mul-full          1.09e-07 2.92e-07   1.41e-07 (1.50e-06)            2.68e-07 (1.50e-06)
#   B5-F33-d260-plain-lens                   1.23e-07 2.10e-07   9.80e-08 (1.50e-06)            1.49e-07 (1.50e-06)
#   B5-F33-d260-plain-full                   1.51e-07 1.54e-07   9.98e-08 (1.50e-06)            7.94e-08 (1.50e-06)
#   B5-F33-d260-mul-lens                     1.07e-07 1.84e-07   1.26e-07 (1.50e-06)            1.57e-07 (1.50e-06)
#   B5-F33-d260-mul-full                     1.69e-07 2.78e-07   1.24e-07 (1.50e-06)            2.63e-07 (1.50e-06)
#   B5-F33-d260-with_ave-lens                1.12e-07 1.62e-07   7.93e-08 (1.50e-06)            1.68e-07 (1.50e-06)
#   B5-F33-d260-with_ave-full                1.34e-07 1.75e-07   1.05e-07 (1.50e-06)            1.58e-07 (1.50e-06)
#   B5-F33-d260-with_ave+mul-lens            1.01e-07 2.97e-07   8.55e-08 (1.50e-06)            3.29e-07 (1.50e-06)
#   B5-F33-d260-with_ave+mul-full            1.14e-07 3.57e-07   1.43e-07 (1.50e-06)            1.84e-07 (1.50e-06)
#   B1030-F2-d4-with_ave+mul-lens            1.08e-07 3.26e-07   1.36e-07 (1.50e-06)            3.50e-07 (1.50e-06)
#   B1030-F2-d4-with_ave+mul-full            2.15e-07 2.29e-07   6.88e-08 (1.50e-06)            2.92e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-lens              1.23e-07 1.77e-07   9.73e-08 (1.50e-06)            1.46e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-full              1.01e-07 2.26e-07   8.23e-08 (1.50e-06)            3.65e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-lens-x3           1.41e-07 2.84e-07   1.42e-07 (1.50e-06)            3.00e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-full-x3           1.53e-07 2.33e-07   1.51e-07 (1.50e-06)            3.65e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-lens-x9           1.41e-07 2.84e-07   1.42e-07 (1.50e-06)            3.00e-07 (1.50e-06)
#   B7-F5-d36-with_ave+mul-full-x9           1.65e-07 3.27e-07   1.77e-07 (1.50e-06)            3.65e-07 (1.50e-06)
#   B1-F9-d260-with_ave+mul-lens             9.43e-08 1.84e-07   1.06e-07 (1.50e-06)            1.56e-07 (1.50e-06)
#   B1-F9-d260-with_ave+mul-full             9.33e-08 1.62e-07   1.42e-07 (1.50e-06)            1.24e-07 (1.50e-06)
#   B9-F8-d128-with_ave+mul-full-std3        2.47e-07 1.77e-07   3.53e-07 (1.50e-06)            3.24e-07 (1.50e-06)
#   B9-F8-d128-with_ave+mul-full-std12       4.81e-07 2.34e-07   5.38e-07 (1.93e-06)            4.29e-07 (1.50e-06)
