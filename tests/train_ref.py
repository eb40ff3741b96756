"""What the training-path GPU tests share (test_gpu_fc_backward, test_gpu_fuse_backward, test_gpu_frame_fuse_backward, test_gpu_optim,
test_gpu_gru_backward): the margin loss as a float64 torch graph, the pieces of the end-to-end bound

    bound(T) = max(4 e32, TOL_UNIT) max |T|  +  GRAD_ABS sum_j |dT / dE_j|        element by element, for a gradient tensor T

and the NaN guard frames around device buffers.  The first term is the bound of the per-kernel cases, e32 being the error of the whole
graph in float32 CPU autograd; the second is the margin loss's own contract (its d_s / d_im are within GRAD_ABS of float64, element by
element) carried to T through the absolute values of the tower's Jacobian, to first order -- T is linear in the loss's gradient.
The towers, the case lists and every assertion stay in the test files."""
import numpy as np
import torch

import fuse_bwd_ref
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
