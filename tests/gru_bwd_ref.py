"""References of the differentiable GRU caption encoder, on the CPU:

  torch_encoder / autograd_grads
                  torch.nn.GRU (CPU: no MIOpen) loaded from the encoder's own state dict, nn.Embedding, pack_padded_sequence and the
                  reference's pooling (model/model.py:340-387) under autograd, in float64 (the reference) or float32 (the yardstick of
                  the error rule);
  bptt            the hand-written float64 backpropagation through time, formula for formula what gru_bwd.hip computes, over the same
                  packed layout; tests/test_gru_bwd_ref.py holds it against autograd_grads.

Both take the captions as token-id arrays in input order and a gradient dout of the output, and return (out, {state-dict key: grad})."""
import numpy as np
import torch


def rel_err(got, want):
    """max |got - want| / max |want|; a reference that is zero throughout admits only zeros."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = float(np.abs(want).max()) if want.size else 0.0
    diff = float(np.abs(got - want).max()) if want.size else 0.0
    if top == 0.0:
        return 0.0 if diff == 0.0 else float('inf')
    return diff / top


def torch_encoder(ids_list, sd, pooling, bidirectional, dtype=torch.float64):
    """The encoder as a CPU torch graph in `dtype`: (out (N, width), its leaves under the encoder's state-dict names)."""
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}
    V, we_dim = sd['we.weight'].shape
    H = sd['rnn.weight_hh_l0'].shape[1]
    we = torch.nn.Embedding(V, we_dim).to(dtype)
    rnn = torch.nn.GRU(we_dim, H, 1, batch_first=True, bidirectional=bidirectional).to(dtype)
    we.load_state_dict({'weight': sd['we.weight']})
    rnn.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith('rnn.')})
    lens = [len(v) for v in ids_list]
    N, T = len(ids_list), max(lens)
    tok = torch.zeros(N, T, dtype=torch.long)
    for i, v in enumerate(ids_list):
        tok[i, :lens[i]] = torch.as_tensor(np.asarray(v), dtype=torch.long)
    packed = torch.nn.utils.rnn.pack_padded_sequence(we(tok), torch.tensor(lens), batch_first=True, enforce_sorted=False)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(rnn(packed)[0], batch_first=True)            # zeros past a row's end
    ln = torch.tensor(lens, dtype=dtype)[:, None]
    mean = y.sum(1) / ln
    last = y[torch.arange(N), torch.tensor(lens) - 1, :H]                                       # bigru: the forward half only
    out = last if pooling == 'last' else torch.cat([mean, last], 1) if pooling == 'mean_last' else mean
    leaves = {'we.weight': we.weight}
    leaves.update({'rnn.' + k: p for k, p in rnn.named_parameters()})
    return out, leaves


def autograd_grads(ids_list, sd, pooling, bidirectional, dout, dtype=torch.float64):
    out, leaves = torch_encoder(ids_list, sd, pooling, bidirectional, dtype)
    out.backward(torch.as_tensor(np.asarray(dout)).to(dtype))
    return out.detach().numpy(), {k: (None if p.grad is None else p.grad.numpy()) for k, p in leaves.items()}


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def bptt(ids_list, sd, pooling, bidirectional, dout):
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    dout = np.asarray(dout, np.float64)
    we = sd['we.weight']
    H = sd['rnn.weight_hh_l0'].shape[1]
    lens_in = np.array([len(v) for v in ids_list])
    perm = np.argsort(-lens_in, kind='stable')
    lens = lens_in[perm]
    N, T = len(ids_list), int(lens.max())
    bs = [int((lens > t).sum()) for t in range(T)]
    off = np.concatenate([[0], np.cumsum(bs)])
    M = int(off[-1])
    tokens = np.concatenate([[ids_list[perm[r]][t] for r in range(bs[t])] for t in range(T)]).astype(np.int64)      # packed order
    X = we[tokens]
    ndirs = 2 if bidirectional and pooling == 'mean' else 1
    width = H if pooling == 'last' else 2 * H if (pooling == 'mean_last' or ndirs == 2) else H
    out = np.zeros((N, width))
    grads = {k: None for k in sd}
    d_x = np.zeros_like(X)
    for d in range(ndirs):
        sfx = '_l0_reverse' if d else '_l0'
        w_ih, w_hh, b_ih, b_hh = (sd['rnn.%s%s' % (n, sfx)] for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
        GI = X @ w_ih.T + b_ih
        R, Z, Nn, Q, HP = (np.zeros((M, H)) for _ in range(5))
        h = np.zeros((N, H))
        total = np.zeros((N, H))
        for i in range(T):                                          # the saving forward
            t = T - 1 - i if d else i
            B, p = bs[t], slice(off[t], off[t] + bs[t])
            hp = h[:B].copy()
            gh = hp @ w_hh.T + b_hh
            r = _sigmoid(GI[p, :H] + gh[:, :H])
            z = _sigmoid(GI[p, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(GI[p, 2 * H:] + r * gh[:, 2 * H:])
            R[p], Z[p], Nn[p], Q[p], HP[p] = r, z, n, gh[:, 2 * H:], hp
            h[:B] = n + z * (hp - n)
            total[:B] += h[:B]
            if not d:
                at_last = np.nonzero(lens[:B] - 1 == t)[0]
                if pooling == 'last':
                    out[perm[at_last], :H] = h[at_last]
                elif pooling == 'mean_last':
                    out[perm[at_last], H:] = h[at_last]
        if pooling != 'last':
            out[perm, d * H:(d + 1) * H] = total / lens[:, None]
        dGI, dGH = np.zeros((M, 3 * H)), np.zeros((M, 3 * H))
        carry = np.zeros((N, H))
        for i in range(T):                                          # the backward recurrence
            t = i if d else T - 1 - i
            nb = t - 1 if d else t + 1
            B, p = bs[t], slice(off[t], off[t] + bs[t])
            dh = np.zeros((B, H))
            if 0 <= nb < T:
                Bnb = min(bs[nb], B)
                dh[:Bnb] = dGH[off[nb]:off[nb] + Bnb] @ w_hh
            dh += carry[:B]
            g = dout[perm[:B]]
            if pooling == 'mean':
                dh += g[:, d * H:(d + 1) * H] / lens[:B, None]
            else:
                at_last = (lens[:B] - 1 == t)[:, None]
                if pooling == 'last':
                    dh += np.where(at_last, g[:, :H], 0.0)
                else:
                    dh += g[:, :H] / lens[:B, None] + np.where(at_last, g[:, H:], 0.0)
            r, z, n, q, hp = R[p], Z[p], Nn[p], Q[p], HP[p]
            da_n = dh * (1 - z) * (1 - n * n)
            da_z = dh * (hp - n) * z * (1 - z)
            da_r = da_n * q * r * (1 - r)
            dGI[p] = np.concatenate([da_r, da_z, da_n], 1)
            dGH[p] = np.concatenate([da_r, da_z, da_n * r], 1)
            carry[:B] = dh * z
        grads['rnn.weight_hh' + sfx] = dGH.T @ HP
        grads['rnn.bias_hh' + sfx] = dGH.sum(0)
        grads['rnn.weight_ih' + sfx] = dGI.T @ X
        grads['rnn.bias_ih' + sfx] = dGI.sum(0)
        d_x += dGI @ w_ih
    d_we = np.zeros_like(we)
    np.add.at(d_we, tokens, d_x)
    grads['we.weight'] = d_we
    return out, grads
