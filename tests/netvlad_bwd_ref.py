"""A float64 numpy restatement of the backward of the reference's NetVLAD (model/Attention.py:862-913) for its two parameters,
fc1.weight and centeroids, beside tests/netvlad_ref.py's forward: the checker of tests/test_netvlad_bwd_ref.py and
tests/test_gpu_netvlad_backward.py.  And the module itself restated in torch, operation for operation, whose
CPU autograd in float32 is the yardstick of the GPU tests' error rule and in float64 their second opinion.

A caption is its rows X (M, D); a caption of Z all-zero rows is np.zeros((Z, D)); an empty caption is np.zeros((0, D)) (the
reference never sees one: the encoder here returns a zero row for it, and it adds nothing to either gradient)."""
import numpy as np

EPS = 1e-12                   # F.normalize's


def netvlad_backward(captions, fc1, cent, d_out):
    """captions: list of (M_i, D) arrays; fc1, cent (K, D); d_out (N, K * D).  Returns (out (N, K * D), d_fc1, d_cent) in float64.
    The clamped branches follow torch: clamp_min passes no gradient to a norm that is not above eps, the derivative is d / eps."""
    fc1, cent, d_out = (np.asarray(a, np.float64) for a in (fc1, cent, d_out))
    K, D = cent.shape
    out = np.zeros((len(captions), K * D))
    d_fc1, d_cent = np.zeros((K, D)), np.zeros((K, D))
    for i, X in enumerate(captions):
        X = np.asarray(X, np.float64).reshape(-1, D)
        xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), EPS)
        z = xh @ fc1.T
        a = np.exp(z - z.max(1, keepdims=True)) if len(X) else z
        a = a / a.sum(1, keepdims=True) if len(X) else a
        s = a.sum(0)
        u = a.T @ xh - s[:, None] * cent
        nu = np.linalg.norm(u, axis=1, keepdims=True)
        w = u / np.maximum(nu, EPS)
        v = w.reshape(-1)
        nv = np.linalg.norm(v)
        o = v / max(nv, EPS)
        out[i] = o
        g = d_out[i]
        dv = ((g - o * (o @ g)) / nv if nv > EPS else g / EPS).reshape(K, D)
        du = np.where(nu > EPS, (dv - w * (w * dv).sum(1, keepdims=True)) / np.maximum(nu, EPS), dv / EPS)
        d_cent -= s[:, None] * du
        da = xh @ du.T - (du * cent).sum(1)[None, :]
        dz = a * (da - (a * da).sum(1, keepdims=True))
        d_fc1 += dz.T @ xh
    return out, d_fc1, d_cent


def torch_encoder(captions, fc1, cent, dtype):
    """NetVLAD.forward restated in torch with the reference's own operations (normalize, Linear, softmax, the expanded residual, the
    two normalisations) on the CPU in `dtype`: (out (N, K * D) with its graph, the leaves {'fc1.weight', 'centeroids'}).  Empty
    captions are left out of the module's input; their rows of out are zeros."""
    import torch
    F = torch.nn.functional
    W = torch.tensor(np.asarray(fc1), dtype=dtype, requires_grad=True)
    C = torch.tensor(np.asarray(cent), dtype=dtype, requires_grad=True)
    K, D = C.shape
    keep = [i for i, X in enumerate(captions) if len(X)]
    out = torch.zeros(len(captions), K * D, dtype=dtype)
    if keep:
        vlad = []
        for i in keep:
            x = F.normalize(torch.tensor(np.asarray(captions[i]), dtype=dtype).reshape(-1, D), p=2, dim=-1)
            M = x.shape[0]
            a = F.softmax(F.linear(x, W), dim=-1)
            residual = x.expand(K, -1, -1).permute(1, 0, 2) - C.expand(M, -1, -1)
            residual = residual * a.unsqueeze(-1)
            vlad.append(residual.sum(dim=0))
        vlad = F.normalize(torch.stack(vlad, 0), p=2, dim=2)
        vlad = F.normalize(vlad.view(vlad.size(0), -1), p=2, dim=1)
        out = out.index_copy(0, torch.tensor(keep), vlad)
    return out, {'fc1.weight': W, 'centeroids': C}


def torch_module_grads(captions, fc1, cent, d_out, dtype):
    """torch_encoder driven backwards by d_out: {'out', 'fc1.weight', 'centeroids'} as float64 numpy."""
    import torch
    out, leaves = torch_encoder(captions, fc1, cent, dtype)
    if out.requires_grad:
        out.backward(torch.tensor(np.asarray(d_out), dtype=dtype))
    res = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in leaves.items()}
    return dict(res, out=out.detach().double().numpy())


def rel_err(got, want):
    """max |got - want| / max |want| (the absolute error where want is all zeros)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    return err / top if top > 0 else err
