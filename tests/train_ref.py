"""What the training-path GPU tests share (test_gpu_fc_backward, test_gpu_fc_gather_backward, test_gpu_dropout_bn, test_gpu_fuse_backward,
test_gpu_frame_fuse_backward, test_gpu_optim, test_gpu_gru_backward): the margin loss as a float64 torch graph, the pieces of the
end-to-end bound

    bound(T) = max(4 e32, TOL_UNIT) max |T|  +  GRAD_ABS sum_j |dT / dE_j|        element by element, for a gradient tensor T

the TransformNet layer and the TransformNet-projection tower as CPU torch graphs with the per-tensor rule that compares a device run
with them, and the NaN guard frames and pitched views around device buffers.  The first term is the bound of the per-kernel cases, e32 being the error of the whole
graph in float32 CPU autograd; the second is the margin loss's own contract (its d_s / d_im are within GRAD_ABS of float64, element by
element) carried to T through the absolute values of the tower's Jacobian, to first order -- T is linear in the loss's gradient.
The case lists and every assertion on device results stay in the test files."""
import numpy as np
import torch

import fc_bwd_ref
import fuse_bwd_ref
import fuse_ref
import loss_ref

TOL_UNIT = 1.5e-6             # the forward's own contract (tests/test_gpu_fuse_routes.py)
GRAD_ABS = 2e-6               # the margin loss's gradient bound (tests/test_gpu_losses.py)
HINGE_CLEAR = 1e-4            # how far every hinge decision of an end-to-end test stays from flipping, in float64


def margin_loss_f64(s, im, margin):
    """MarginRankingLoss(margin, 'cosine', max_violation=False, 'sum', 'bidir') per head, summed, in torch on (B, H, d) or (B, d)."""
    if s.dim() == 2:
        s, im = s[:, None], im[:, None]
    total = 0.0
    B = s.shape[0]
    off = ~torch.eye(B, dtype=torch.bool)
    for h in range(s.shape[1]):
        sh = s[:, h] / (s[:, h].pow(2).sum(1, keepdim=True).sqrt() + loss_ref.EPS)
        ih = im[:, h] / (im[:, h].pow(2).sum(1, keepdim=True).sqrt() + loss_ref.EPS)
        S = ih @ sh.T
        dg = torch.diag(S)
        total = total + (torch.clamp(margin + S - dg[:, None], min=0) * off).sum() + (torch.clamp(margin + S - dg[None, :], min=0) * off).sum()
    return total


def hinge_slack(Et, Ev, margin):
    """The smallest distance of any hinge decision of margin_loss_f64(Et, Ev, margin) from flipping, over the heads, in float64."""
    Et, Ev = Et.detach().double(), Ev.detach().double()
    if Et.dim() == 2:
        Et, Ev = Et[:, None], Ev[:, None]
    return min(loss_ref.margin_scores_slack(
        (Ev[:, h] / Ev[:, h].norm(dim=1, keepdim=True)).numpy() @ (Et[:, h] / Et[:, h].norm(dim=1, keepdim=True)).numpy().T,
        margin, False, 'bidir') for h in range(Et.shape[1]))


def hinge_clear_seed(build, margin, first_seed, tries=40):
    """build(seed) seeds torch itself and returns (what the test goes on with, Et, Ev in float64).  The first of `tries` seeds from
    first_seed whose pairs all stay HINGE_CLEAR off every hinge decision: the float32 and the device graph then take the decisions
    float64 takes.  No seed: the test fails."""
    for seed in range(first_seed, first_seed + tries):
        torch.manual_seed(seed)
        state, Et, Ev = build()
        slack = hinge_slack(Et, Ev, margin)
        if slack >= HINGE_CLEAR:
            break
    assert slack >= HINGE_CLEAR
    return state


def abs_jacobian(E, leaves, batched=True):
    """{name: sum_j |d leaf / d E_j|} from the float64 graph E(leaves): batched backwards over the unit vectors of E, 256 at a time,
    or (a graph that torch cannot batch, nn.GRU) one backward per element of E."""
    names = list(leaves)
    acc = {k: torch.zeros_like(leaves[k]) for k in names}
    if not batched:
        for j in range(E.numel()):
            js = torch.autograd.grad(E.reshape(-1)[j], [leaves[k] for k in names], retain_graph=True)
            for k, t in zip(names, js):
                acc[k] += t.abs()
        return acc
    eye = torch.eye(E.numel(), dtype=torch.float64).reshape(E.numel(), *E.shape)
    for lo in range(0, E.numel(), 256):
        js = torch.autograd.grad(E, [leaves[k] for k in names], eye[lo:lo + 256], retain_graph=True, is_grads_batched=True)
        for k, j in zip(names, js):
            acc[k] += j.abs().sum(0)
    return acc


def end_to_end_bound(r64, r32, absjac):
    """(bound of the docstring above for the tensor whose float64 / float32 CPU gradients are r64 / r32, e32, max |r64|)."""
    top = float(r64.abs().max())
    e32 = fuse_bwd_ref.rel_err(r32, r64)
    return max(4.0 * e32, TOL_UNIT) * top + GRAD_ABS * absjac, e32, top


def untouched_around(buf, view):
    """Whether every float of the NaN-filled buffer outside `view` (a view into it, strided or not) is NaN still."""
    chk = buf.clone()
    torch.as_strided(chk, view.shape, view.stride(), view.storage_offset()).fill_(float('nan'))
    return bool(chk.isnan().all())


class Frames:
    """Device buffers inside NaN frames of `guard` floats on either side: every float outside what was handed out has to be NaN still
    after the launches.  `held` lists (the whole buffer, the 16-byte aligned view in its middle)."""

    def __init__(self, guard, device='cuda'):
        assert guard % 4 == 0
        self.guard, self.device, self.held = guard, device, []

    def floats(self, *shape):
        n = int(np.prod(shape))
        whole = torch.full((n + 2 * self.guard,), float('nan'), dtype=torch.float32, device=self.device)
        self.held.append((whole, whole[self.guard:self.guard + n]))
        return self.held[-1][1].view(*shape)

    def bytes(self, nbytes):
        n = (nbytes + 3) // 4
        return self.floats(max(n, 4)).view(torch.uint8)[:max(nbytes, 16)]

    def intact(self):
        return all(untouched_around(whole, view) for whole, view in self.held)


# ---- pitched and offset row views (test_gpu_fc_backward, test_gpu_fc_gather_backward) -----------------------------------------------
def pitch(cols, layout):
    """(row pitch, floats between a 16-byte boundary and the base) of a (rows, cols) view.  'dense': rows on a 16-byte aligned base;
    'pitch4': a wider pitch that keeps the rows 16-byte aligned; 'pitch3': a wider pitch that does not; 'offset': the pitch of
    'pitch4', the base 4 bytes past a 16-byte boundary; 'window': a column window at an odd offset of a wider buffer."""
    up = (cols + 3) // 4 * 4
    return {'dense': (cols, 0), 'pitch4': (up + 4, 0), 'pitch3': (cols + 3, 0), 'offset': (up + 4, 1), 'window': (cols + 9, 3)}[layout]


def pitched(rows, cols, layout, device='cuda'):
    """A NaN-filled device buffer and the (rows, cols) view of `layout` inside it, one row of canary in front and one behind:
    (buffer, view), as untouched_around takes them."""
    ld, off = pitch(cols, layout)
    base = (ld + 3) // 4 * 4 + off
    buf = torch.full((base + (rows + 1) * ld + 4,), float('nan'), device=device)
    view = torch.as_strided(buf, (rows, cols), (ld, 1), base)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    return buf, view


def place(t, layout, device='cuda'):
    """A device copy of the 2-D CPU tensor t in `layout`, NaN all around it: (buffer, view)."""
    buf, view = pitched(t.shape[0], t.shape[1], layout, device)
    view.copy_(t)
    return buf, view


def out_vec(n, aligned=False, device='cuda'):
    """A NaN-filled buffer and a [n] view inside it, 4 bytes past a 16-byte boundary or (aligned) on one: (buffer, view)."""
    buf = torch.full((n + 8,), float('nan'), device=device)
    lo = 4 if aligned else 1
    return buf, buf[lo:lo + n]


# ---- the TransformNet layer and the per-tensor rule of the module-level tests --------------------------------------------------------
def layer_graph(dtype, W, b, x, dE, activation, bn, mask=None, p=0.0, eps=1e-5, momentum=0.1):
    """The reference's layer restated from torch modules on the CPU in `dtype`: Linear -> activation -> dropout by a given keep mask (a
    bool array or tensor; None: no dropout) at rate p -> BatchNorm1d(eps, momentum) in training mode where bn, driven backwards by dE.
    Returns every compared tensor by name, x.grad and the activation output a among them, in float64."""
    lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(b)
    xs = x.to(dtype).requires_grad_(True)
    y = a = fc_bwd_ref.forward_torch(xs, lin.weight, lin.bias, activation)
    if mask is not None:
        y = y * torch.as_tensor(mask).to(dtype) / (1.0 - p)
    if bn:
        norm = torch.nn.BatchNorm1d(W.shape[0], eps=eps, momentum=momentum).to(dtype).train()
        y = norm(y)
    y.backward(dE.to(dtype))
    out = {'y': y, 'a': a, 'x.grad': xs.grad, 'fc1.weight.grad': lin.weight.grad, 'fc1.bias.grad': lin.bias.grad}
    if bn:
        out.update({'bn1.weight.grad': norm.weight.grad, 'bn1.bias.grad': norm.bias.grad, 'running_mean': norm.running_mean,
                    'running_var': norm.running_var})
    return {k: v.detach().double() for k, v in out.items()}


def compare(got, ref, f32, label=''):
    """Per tensor of `got`: max |device - float64| / max |float64| <= max(4 e32, TOL_UNIT), e32 the same error of the float32 CPU graph
    f32 against the float64 one ref.  Returns the largest err / bound."""
    worst = 0.0
    for k, g in got.items():
        e32 = fc_bwd_ref.rel_err(f32[k], ref[k])
        bound = max(4.0 * e32, TOL_UNIT)
        err = fc_bwd_ref.rel_err(g.detach().cpu(), ref[k])
        worst = max(worst, err / bound)
        print('%s%-16s device %.3e  fp32 CPU %.3e  bound %.3e' % (label and label + ' ', k, err, e32, bound))
        assert err <= bound, (k, err, bound)
    return worst


# ---- the TransformNet-projection tower of the end-to-end tests -------------------------------------------------------------------------
class Side(torch.nn.Module):
    """One tower: L TransformNet projections (fc1 + tanh) whose plane() outputs go to the fusion block's fuse_planes."""

    def __init__(self, dims, D, H):
        super().__init__()
        from laff_amd.model.Attention import Multi_head_MyApply_Attention
        from laff_amd.model.model import TransformNet
        self.proj = torch.nn.ModuleList([TransformNet((k, D), batch_norm=False, activation='tanh', dropout=0.0) for k in dims])
        self.att = Multi_head_MyApply_Attention(D, H, D // H, with_ave=True, mul=True)

    def forward(self, feats):
        return self.att.fuse_planes([p.plane(f) for p, f in zip(self.proj, feats)])


def side_f64(side, feats, dtype=torch.float64, clone=False):
    """The same tower as a CPU torch graph in `dtype` with fuse_ref.attention: (E, its leaves by name).  clone: the leaves are copies,
    for a caller that steps them."""
    leaves = {}

    def leaf(name, t):
        t = t.detach().cpu().to(dtype)
        leaves[name] = (t.clone() if clone else t).requires_grad_(True)
        return leaves[name]
    fs = [leaf('feat%d' % i, f) for i, f in enumerate(feats)]
    planes = torch.stack([torch.tanh(f @ leaf('proj.%d.fc1.weight' % i, p.fc1.weight).T + leaf('proj.%d.fc1.bias' % i, p.fc1.bias))
                          for i, (p, f) in enumerate(zip(side.proj, fs))], 1)
    heads = [(leaf('att.attention_layer.%d.embedding_common.0.weight' % h, a.embedding_common[0].weight),
              leaf('att.attention_layer.%d.embedding_common.0.bias' % h, a.embedding_common[0].bias),
              a.global_emb_weight_net.weight.detach().cpu().to(dtype).reshape(1)) for h, a in enumerate(side.att.attention_layer)]
    w = torch.stack([h[0].reshape(-1) for h in heads])
    b = torch.cat([h[1].reshape(1) for h in heads])
    gw = torch.cat([h[2].reshape(1) for h in heads])
    H = len(heads)
    keep = fuse_ref.F64
    fuse_ref.F64 = dtype
    try:
        E = fuse_ref.attention(fuse_bwd_ref.heads_of(planes, H, planes.shape[2] // H, True), w, b, gw, with_ave=True, mul=True,
                               l2norm_each_head=False)[0]
    finally:
        fuse_ref.F64 = keep
    return E, leaves
