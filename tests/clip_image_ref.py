"""A float64 torch restatement of clip.model.VisualTransformer.forward (model/clip/model.py:153-243): conv1 as a dense patch matmul,
dense attention over every row of every block, ln_post of the class row, proj.  The checker of tests/test_clip_image_host.py and
tests/test_gpu_clip_image.py; runs on the CPU for small configs and on the device (float64) at full size.  Also the reference-shaped
torch fp16 path (RefImageFp16), the yardstick of the fp16 encoder."""
import collections

import numpy as np
import torch
import torch.nn.functional as Fn


def fixture_config(z, name):
    """(cfg, visual state dict of fp32 arrays under `visual.*`, frames [F, 3, R, R] fp32) of fixture config `name`; every value is
    the stored int8 q * 2**e, the exact values the reference ran on."""
    e = z.sub(name + '/e/')
    sd = {k: q.astype(np.float32) * np.float32(2.0 ** int(e[k])) for k, q in z.sub(name + '/q/').items()}
    pix = z[name + '/pix_q'].astype(np.float32) * np.float32(2.0 ** int(z[name + '/pix_e']))
    return z.json(name + '/cfg'), sd, pix


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def _t64(sd, device):
    return {k: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=torch.float64).to(device)
            for k, v in sd.items()}


def encode_image64(pixels, sd, device='cpu', chunk=64):
    """pixels [F, 3, R, R], sd: the visual state dict (`visual.*` names; arrays or tensors) -> (F, embed_dim) float64 numpy."""
    t = _t64({k[len('visual.'):]: v for k, v in sd.items()}, device)
    conv = t['conv1.weight']
    W, P = conv.shape[0], conv.shape[-1]
    H = W // 64
    layers = len([k for k in t if k.endswith('.attn.in_proj_weight')])
    wc = conv.reshape(W, -1)
    pix = torch.as_tensor(np.asarray(pixels.detach().cpu() if isinstance(pixels, torch.Tensor) else pixels), dtype=torch.float64)
    outs = []
    for s in range(0, pix.shape[0], chunk):
        x = pix[s:s + chunk].to(device)
        n, R = x.shape[0], x.shape[-1]
        g = R // P
        # [n, 3, g, P, g, P] -> [n, g, g, 3, P, P]: patch (py, px) in row-major order, (c, ky, kx) in conv1.weight's order
        p = x.reshape(n, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * P * P)
        x = torch.cat([t['class_embedding'].expand(n, 1, W), p @ wc.T], dim=1) + t['positional_embedding']
        x = _ln(x, t['ln_pre.weight'], t['ln_pre.bias'])
        L = x.shape[1]
        for i in range(layers):
            pre = 'transformer.resblocks.%d.' % i
            h = _ln(x, t[pre + 'ln_1.weight'], t[pre + 'ln_1.bias'])
            qkv = h @ t[pre + 'attn.in_proj_weight'].T + t[pre + 'attn.in_proj_bias']
            q, k, v = (a.reshape(n, L, H, 64).transpose(1, 2) for a in qkv.split(W, dim=-1))
            att = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)
            a = (att @ v).transpose(1, 2).reshape(n, L, W)
            x = x + a @ t[pre + 'attn.out_proj.weight'].T + t[pre + 'attn.out_proj.bias']
            h = _ln(x, t[pre + 'ln_2.weight'], t[pre + 'ln_2.bias'])
            m = h @ t[pre + 'mlp.c_fc.weight'].T + t[pre + 'mlp.c_fc.bias']
            m = m * torch.sigmoid(1.702 * m)
            x = x + m @ t[pre + 'mlp.c_proj.weight'].T + t[pre + 'mlp.c_proj.bias']
        outs.append((_ln(x[:, 0], t['ln_post.weight'], t['ln_post.bias']) @ t['proj']).cpu().numpy())
    return np.concatenate(outs) if outs else np.zeros((0, t['proj'].shape[1]))


class _QuickGELU(torch.nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _RefBlock(torch.nn.Module):
    def __init__(self, width, heads):
        super().__init__()
        self.attn = torch.nn.MultiheadAttention(width, heads)
        self.ln_1 = torch.nn.LayerNorm(width)
        self.mlp = torch.nn.Sequential(collections.OrderedDict([('c_fc', torch.nn.Linear(width, 4 * width)), ('gelu', _QuickGELU()),
                                                                ('c_proj', torch.nn.Linear(4 * width, width))]))
        self.ln_2 = torch.nn.LayerNorm(width)


def _ln_cast(m, x):
    return m(x.float()).to(x.dtype)                       # clip.model.LayerNorm: fp32 inside, the stream's dtype outside


class RefImageFp16(torch.nn.Module):
    """The shape of the reference's encode_image as clip.load leaves it on a GPU (convert_weights: conv1, Linear / MultiheadAttention
    weights and proj in fp16; LayerNorm fp32 cast at use; class / positional embeddings cast to the stream's fp16), built from torch
    modules: F.conv2d, nn.MultiheadAttention over all rows.  Takes the `visual.*` state dict."""

    def __init__(self, sd, device='cuda'):
        super().__init__()
        sd = {k[len('visual.'):]: torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v),
                                                  dtype=torch.float32) for k, v in sd.items()}
        W, P = sd['conv1.weight'].shape[0], sd['conv1.weight'].shape[-1]
        layers = len([k for k in sd if k.endswith('.attn.in_proj_weight')])
        self.patch = P
        self.conv1 = torch.nn.Conv2d(3, W, kernel_size=P, stride=P, bias=False)
        self.class_embedding = torch.nn.Parameter(torch.empty(W))
        self.positional_embedding = torch.nn.Parameter(torch.empty(sd['positional_embedding'].shape))
        self.ln_pre = torch.nn.LayerNorm(W)
        self.transformer = torch.nn.Module()
        self.transformer.resblocks = torch.nn.Sequential(*[_RefBlock(W, W // 64) for _ in range(layers)])
        self.ln_post = torch.nn.LayerNorm(W)
        self.proj = torch.nn.Parameter(torch.empty(sd['proj'].shape))
        self.load_state_dict(sd, strict=True)
        self.to(device)
        for m in self.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear, torch.nn.MultiheadAttention)):
                m.half()
        self.proj.data = self.proj.data.half()

    @torch.no_grad()
    def forward(self, pixels):
        x = Fn.conv2d(pixels.half(), self.conv1.weight, stride=self.patch)
        x = x.reshape(x.shape[0], x.shape[1], -1).permute(0, 2, 1)
        cls = self.class_embedding.half() + torch.zeros(x.shape[0], 1, x.shape[-1], dtype=x.dtype, device=x.device)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.half()
        x = _ln_cast(self.ln_pre, x).permute(1, 0, 2)
        for b in self.transformer.resblocks:
            h = _ln_cast(b.ln_1, x)
            x = x + b.attn(h, h, h, need_weights=False)[0]
            x = x + b.mlp(_ln_cast(b.ln_2, x))
        x = _ln_cast(self.ln_post, x.permute(1, 0, 2)[:, 0, :])
        return x @ self.proj
