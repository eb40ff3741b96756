"""A float64 torch restatement of clip.model.CLIP.encode_text (model/clip/model.py:153-206, 245-358): all context_length positions
with the dense causal mask, so it checks the ragged cut of laff_clip_encode as well.  The checker of tests/test_clip_host.py and
tests/test_gpu_clip.py; runs on the CPU for small configs and on the device (float64) at full size."""
import numpy as np
import torch


def full_text_sd(z):
    """The fixture's text state dict (stored as int8 q * 2**e, the exact values the reference ran on) with the whole token-embedding
    table (rows the captions do not use are zero)."""
    e = z.sub('e/')
    sd = {k: (q.astype(np.float32) * np.float32(2.0 ** int(e[k]))) for k, q in z.sub('q/').items()}
    cfg = z.json('cfg')
    te = np.zeros((cfg['vocab_size'], cfg['width']), np.float32)
    te[z['tok_rows']] = sd['token_embedding.weight']
    sd['token_embedding.weight'] = te
    return sd


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def encode_text64(ids, sd, device='cpu', chunk=256):
    """ids [N, context] (clip.tokenize), sd: the bare text state dict (arrays or tensors) -> (N, embed_dim) float64 numpy."""
    t = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=torch.float64).to(device)
         for k, v in sd.items()}
    W = t['ln_final.weight'].shape[0]
    H = W // 64
    layers = len(set(k.split('.')[2] for k in t if k.startswith('transformer.resblocks')))
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long, device=device)
    N, L = ids.shape
    mask = torch.full((L, L), float('-inf'), dtype=torch.float64, device=device).triu_(1)
    outs = []
    for s in range(0, N, chunk):
        tok = ids[s:s + chunk]
        n = tok.shape[0]
        x = t['token_embedding.weight'][tok] + t['positional_embedding'][:L]
        for i in range(layers):
            p = 'transformer.resblocks.%d.' % i
            h = _ln(x, t[p + 'ln_1.weight'], t[p + 'ln_1.bias'])
            qkv = h @ t[p + 'attn.in_proj_weight'].T + t[p + 'attn.in_proj_bias']
            q, k, v = (a.reshape(n, L, H, 64).transpose(1, 2) for a in qkv.split(W, dim=-1))
            att = torch.softmax(q @ k.transpose(-1, -2) / 8.0 + mask, dim=-1)
            a = (att @ v).transpose(1, 2).reshape(n, L, W)
            x = x + a @ t[p + 'attn.out_proj.weight'].T + t[p + 'attn.out_proj.bias']
            h = _ln(x, t[p + 'ln_2.weight'], t[p + 'ln_2.bias'])
            m = h @ t[p + 'mlp.c_fc.weight'].T + t[p + 'mlp.c_fc.bias']
            m = m * torch.sigmoid(1.702 * m)
            x = x + m @ t[p + 'mlp.c_proj.weight'].T + t[p + 'mlp.c_proj.bias']
        x = _ln(x, t['ln_final.weight'], t['ln_final.bias'])
        outs.append((x[torch.arange(n, device=device), tok.argmax(dim=-1)] @ t['text_projection']).cpu().numpy())
    return np.concatenate(outs) if outs else np.zeros((0, t['text_projection'].shape[1]))


class _QuickGELU(torch.nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _RefBlock(torch.nn.Module):
    def __init__(self, width, heads):
        import collections
        super().__init__()
        self.attn = torch.nn.MultiheadAttention(width, heads)
        self.ln_1 = torch.nn.LayerNorm(width)
        self.mlp = torch.nn.Sequential(collections.OrderedDict([('c_fc', torch.nn.Linear(width, 4 * width)), ('gelu', _QuickGELU()),
                                                                ('c_proj', torch.nn.Linear(4 * width, width))]))
        self.ln_2 = torch.nn.LayerNorm(width)


def _ln_cast(m, x):
    return m(x.float()).to(x.dtype)                       # clip.model.LayerNorm: fp32 inside, the stream's dtype outside


class RefTextFp16(torch.nn.Module):
    """The shape of the reference's encode_text as clip.load leaves it on a GPU (convert_weights: Linear / MultiheadAttention
    weights and text_projection in fp16, LayerNorm and the embeddings in fp32 cast at use), built from torch modules: fp16 stream,
    all context_length positions, nn.MultiheadAttention with the additive causal mask.  The yardstick of the fp16 encoder."""

    def __init__(self, sd, device='cuda'):
        super().__init__()
        sd = {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=torch.float32)
              for k, v in sd.items()}
        W = sd['ln_final.weight'].shape[0]
        layers = len(set(k.split('.')[2] for k in sd if k.startswith('transformer.resblocks')))
        V, E = sd['token_embedding.weight'].shape[0], sd['text_projection'].shape[1]
        L = sd['positional_embedding'].shape[0]
        self.token_embedding = torch.nn.Embedding(V, W)
        self.positional_embedding = torch.nn.Parameter(torch.empty(L, W))
        self.transformer = torch.nn.Module()
        self.transformer.resblocks = torch.nn.Sequential(*[_RefBlock(W, W // 64) for _ in range(layers)])
        self.ln_final = torch.nn.LayerNorm(W)
        self.text_projection = torch.nn.Parameter(torch.empty(W, E))
        self.load_state_dict(sd, strict=True)
        self.to(device)
        for m in self.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.MultiheadAttention)):
                m.half()
        self.text_projection.data = self.text_projection.data.half()
        self.register_buffer('mask', torch.full((L, L), float('-inf'), device=device).triu_(1).half())

    @torch.no_grad()
    def forward(self, ids):
        x = self.token_embedding(ids).half() + self.positional_embedding.half()
        x = x.permute(1, 0, 2)
        for b in self.transformer.resblocks:
            h = _ln_cast(b.ln_1, x)
            x = x + b.attn(h, h, h, need_weights=False, attn_mask=self.mask)[0]
            x = x + b.mlp(_ln_cast(b.ln_2, x))
        x = _ln_cast(self.ln_final, x.permute(1, 0, 2))
        return x[torch.arange(x.shape[0], device=x.device), ids.argmax(dim=-1)] @ self.text_projection
