"""A plain torch restatement of the multi-head self-attention fusion block (laff_amd.model.Attention.Multi_head_MyApply_selfAttention,
laff_amd/csrc/selfattn_fuse.hip), every operation on the CPU in float64 or float32.  Gradients come from
torch.autograd through it.  It is the checker of the kernels (tests/test_gpu_selfattn_fuse.py) and is itself held to the reference's
own class through tests/golden/selfattn.*.npz (tests/test_selfattn_ref.py).

Per group (row n, head h) of planes (N, L, H * d), plane l holding x_l[n, h * d + c]:
    tokens: the L head slices; 'max_embedding' / 'mean_embedding' put the elementwise max / the mean over l in front (T = L + 1)
    l2norm_each_head: t_i <- t_i / (|t_i| + 1e-13 + 1e-14)
    A = softmax_j(s t_i . t_j),  s = (d // H) ** -0.5;   r_i = sum_j A_ij t_j + t_i
    o_i = gamma * (r_i - mean r_i) / sqrt(var r_i + 1e-5) + beta   (biased variance)
    pooled by the output type; under 'Attention_1' head h of the o_i goes through an Attention_1 block of its own.
Maxima take the LOWEST index on a tie, in the forward and in the routing of the gradient.
"""
import numpy as np
import torch

F64 = torch.float64
NORM_EPS = 1e-13 + 1e-14
LN_EPS = 1e-5
OUTPUT_TYPES = ('mean', 'max', 'first', 'last', 'second', 'third', 'max_embedding', 'mean_embedding', 'random', 'Attention_1')


def _t(a, dtype=F64):
    return a.detach().to('cpu', dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype)


def first_max(x, dim):
    """max over `dim`; on a tie the value (and so the gradient) is the first index's"""
    is_max = x == x.max(dim, keepdim=True).values
    first = is_max & (is_max.cumsum(dim) == 1)
    return torch.where(first, x, torch.zeros_like(x)).sum(dim)


def tokens_out(planes, H, d, gamma, beta, output_type, l2norm_each_head, scale=None):
    """(o (N, H, T, d), A (N, H, T, T)) in the dtype of `planes`.  scale: s, where `planes` hold some of the block's heads only."""
    N, L = planes.shape[:2]
    x = planes.reshape(N, L, H, d).permute(0, 2, 1, 3)                 # (N, H, L, d)
    if output_type == 'max_embedding':
        x = torch.cat([first_max(x, 2).unsqueeze(2), x], 2)
    elif output_type == 'mean_embedding':
        x = torch.cat([x.mean(2, keepdim=True), x], 2)
    if l2norm_each_head:
        x = x / (x.pow(2).sum(3, keepdim=True).sqrt() + NORM_EPS)
    s = (d // H) ** -0.5 if scale is None else scale
    A = torch.softmax(s * torch.einsum('nhid,nhjd->nhij', x, x), dim=3)
    r = torch.einsum('nhij,nhjd->nhid', A, x) + x
    mu = r.mean(3, keepdim=True)
    var = (r - mu).pow(2).mean(3, keepdim=True)
    return gamma * (r - mu) / (var + LN_EPS).sqrt() + beta, A


def attention_1(x, w, b, gw, with_ave, mul):
    """The Attention_1 block on x (N, L, d): (E (N, d), the weights it records (N, L))"""
    mean = x.mean(1)
    common = x * mean[:, None] if mul else x
    a = torch.softmax(common @ w + b, dim=1)
    g = (a[:, :, None] * x).sum(1)
    rec = a
    if with_ave:
        g = g + gw * x.sum(1)                                          # gw times the SUM over l: the mean is added to every l
        rec = a + gw / a.shape[1]
    return g / g.pow(2).sum(1, keepdim=True).sqrt(), rec


def forward(planes, H, d, gamma, beta, output_type, l2norm_each_head=False, att1=None, training=False, scale=None):
    """E (N, H, d).  att1 (for 'Attention_1'): {'w': (H, d), 'b': (H,), 'gw': (H,), 'with_ave': bool, 'mul': bool}.
    Returns (E, weights): weights is what get_attention_weight answers under 'Attention_1' (N, L), else None."""
    if output_type not in OUTPUT_TYPES or (training and output_type == 'random'):
        raise ValueError(output_type)
    L = planes.shape[1]
    o, _ = tokens_out(planes, H, d, gamma, beta, output_type, l2norm_each_head, scale)
    if output_type in ('mean', 'random'):
        return o.mean(2), None
    if output_type == 'max':
        return first_max(o, 2), None
    if output_type in ('first', 'max_embedding', 'mean_embedding'):
        return o[:, :, 0], None
    if output_type == 'last':
        return o[:, :, -1], None
    if output_type == 'second':
        return o[:, :, 1 if L >= 2 else 0], None
    if output_type == 'third':
        return o[:, :, 2 if L >= 3 else 0], None
    E, W = [], None
    for h in range(H):
        e, rec = attention_1(o[:, h], att1['w'][h], att1['b'][h], att1['gw'][h], att1['with_ave'], att1['mul'])
        E.append(e)
        W = rec if W is None else W + rec
    return torch.stack(E, 1), W / H


def run(planes, H, d, gamma, beta, output_type, l2norm_each_head=False, att1=None, dE=None, dtype=F64):
    """{'E', 'weights', and with dE: 'dx' (N, L, H d), 'dgamma', 'dbeta', 'dw', 'db'} -- computed in `dtype`, returned in float64."""
    P = _t(planes, dtype).requires_grad_(dE is not None)
    g, b = _t(gamma, dtype).requires_grad_(dE is not None), _t(beta, dtype).requires_grad_(dE is not None)
    a1 = None
    if att1 is not None:
        a1 = dict(att1, w=_t(att1['w'], dtype).requires_grad_(dE is not None), b=_t(att1['b'], dtype).requires_grad_(dE is not None),
                  gw=_t(att1['gw'], dtype))
    with torch.enable_grad():
        E, W = forward(P, H, d, g, b, output_type, l2norm_each_head, a1)
        assert E.dtype == dtype
        out = {'E': E.detach().to(F64), 'weights': None if W is None else W.detach().to(F64)}
        if dE is not None:
            (E * _t(dE, dtype).reshape(E.shape)).sum().backward()
            out.update(dx=P.grad.to(F64), dgamma=g.grad.to(F64), dbeta=b.grad.to(F64))
            if a1 is not None:
                out.update(dw=a1['w'].grad.to(F64), db=a1['b'].grad.to(F64))
    return out


def max_gap_groups(planes, H, d, gamma, beta, output_type, l2norm_each_head, rel=1e-5):
    """(N, H) bool: the groups that hold an element whose two largest candidates of a maximum ('max': over the o_i; 'max_embedding':
    over the planes) lie within rel * max |o| (resp. max |x|) of each other in float64 -- there a float32 run may route the gradient
    elsewhere.  All False for the other output types."""
    P = _t(planes)
    N, L = P.shape[:2]
    none = torch.zeros(N, H, dtype=torch.bool)
    if output_type == 'max':
        cand, _ = tokens_out(P, H, d, _t(gamma), _t(beta), output_type, l2norm_each_head)
    elif output_type == 'max_embedding':
        cand = P.reshape(N, L, H, d).permute(0, 2, 1, 3)
    else:
        return none
    if cand.shape[2] < 2:
        return none
    top = cand.topk(2, dim=2).values
    return ((top[:, :, 0] - top[:, :, 1]) < rel * float(cand.abs().max())).any(2)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (tests/fuse_bwd_ref.rel_err): a reference of zeros admits nothing but zeros."""
    got, ref = _t(got).reshape(-1), _t(ref).reshape(-1)
    if ref.numel() == 0:
        return 0.0
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if not bool(got.any()) else float('inf')
    return float((got - ref).abs().max()) / top


def fixture_cases():
    """Every case of tests/golden/selfattn.*.npz (tools/gen_golden_selfattn.py) as (id, dict): the reference's own class on the CPU --
    'shape' (N, L, H, d), 'type', 'l2n', the float32 inputs, the float64 results, 'e32' per result, 'att1' (or None), 'state_dict'."""
    import glob
    import json
    import os
    out = []
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'selfattn.*.npz'))):
        z = np.load(path)
        meta = json.loads(str(z['meta']))
        for name in meta['cases']:
            t, l2n = name.rsplit('.', 1)
            c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '/')}
            case = {'shape': tuple(meta['shape']), 'type': t, 'l2n': bool(int(l2n)), 'state_dict': meta['state_dict'][name],
                    'e32': {k[4:]: float(v) for k, v in c.items() if k.startswith('e32/')}, 'att1': None}
            case.update({k: v for k, v in c.items() if not k.startswith('e32/')})
            if t == 'Attention_1':
                case['att1'] = {'w': c['w'], 'b': c['b'], 'gw': c['gw'], 'with_ave': bool(c['with_ave']), 'mul': bool(c['mul'])}
            out.append(('%s-L%dH%dd%d' % ((name,) + tuple(meta['shape'][1:])), case))
    return out
