"""A float64 numpy restatement of the reference's GRU caption encoder (torch.nn.GRU arithmetic, gate order r, z, n; h0 = 0;
model/model.py:340-387 pooling): the checker of tests/test_gru_host.py and tests/test_gpu_gru.py."""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_run(ids_list, we, w_ih, w_hh, b_ih, b_hh, reverse=False):
    """Per caption (list of token-id arrays): the (len, H) float64 hidden states of one direction, in time order."""
    we, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in (we, w_ih, w_hh, b_ih, b_hh))
    H = w_hh.shape[1]
    P = we @ w_ih.T + b_ih                                         # the input half of every token, [V, 3H]
    lens = np.array([len(v) for v in ids_list])
    T, N = int(lens.max()), len(ids_list)
    out = np.zeros((N, T, H))
    h = np.zeros((N, H))
    for s in range(T):
        t = T - 1 - s if reverse else s
        act = np.nonzero(lens > t)[0]
        if reverse:
            h[lens == t + 1] = 0.0                                 # a row starts its reverse pass at its last token
        x = P[np.array([ids_list[i][t] for i in act])]
        gh = h[act] @ w_hh.T + b_hh
        r = _sigmoid(x[:, :H] + gh[:, :H])
        z = _sigmoid(x[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(x[:, 2 * H:] + r * gh[:, 2 * H:])
        h[act] = (1 - z) * n + z * h[act]
        out[act, t] = h[act]
    return [out[i, :lens[i]] for i in range(N)]


def gru_features(ids_list, sd, pooling='mean', bidirectional=False):
    """sd: the reference's state-dict names (we.weight, rnn.weight_ih_l0, ... [_reverse]) -> (N, width) float64."""
    def run(sfx, rev):
        return gru_run(ids_list, sd['we.weight'], sd['rnn.weight_ih_l0' + sfx], sd['rnn.weight_hh_l0' + sfx],
                       sd['rnn.bias_ih_l0' + sfx], sd['rnn.bias_hh_l0' + sfx], rev)
    fwd = run('', False)
    mean = np.stack([f.mean(axis=0) for f in fwd])
    last = np.stack([f[-1] for f in fwd])
    if pooling == 'last':
        return last                                                # bigru: the forward half only, as the reference gathers it
    if pooling == 'mean_last':
        if bidirectional:
            raise ValueError('bigru_mean_last')
        return np.concatenate([mean, last], axis=1)
    if bidirectional:
        return np.concatenate([mean, np.stack([r.mean(axis=0) for r in run('_reverse', True)])], axis=1)
    return mean
