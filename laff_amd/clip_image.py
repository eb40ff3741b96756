"""The CLIP image encoder on the device: preprocessed frames -> per-frame and per-video CLIP features, a drop-in for the visual half of
the reference's `CLIPEncoder` (model/model.py:485-525) over `clip.model.CLIP.encode_image` (VisualTransformer, model/clip/model.py:
153-243, 342-343).  The ViT towers only (ViT-B/32, ViT-B/16, ViT-L/14); the transformer runs on the GPU (`laff_clip_image_encode`,
laff_amd/csrc/clip_image.hip).

Frames come either as the reference's data provider leaves them -- `vis_origin_frame_tuple`, one [F_v, 3, R, R] fp32 tensor per video,
already resized and normalised -- or as decoded RGB uint8 frames of any size (`encode_raw_frames`, `video_features_raw`): those are
resized, cropped and normalised on the device too, bit for bit as the reference's torchvision-on-Pillow transform does it
(laff_amd/frame_prep.py, `laff_frame_preprocess`).  Only decoding stays with the caller.  `ClipFrameLoader` wraps a loader of
`collate_vision` batches and fills the per-video mean and the zero-padded per-frame features, so a LAFF / FrameLAFF model's predict()
runs from frames of either form.
"""
import numpy as np
import torch
import torch.nn as nn

from .clip_text import _Block, _check_dims, _init_blocks
from .ragged import _Weights, _chunks

_PREFIXES = ('clip_model.ClipModel.', 'ClipModel.')


class _ClipVisual(nn.Module):
    """The parameters of clip.model.VisualTransformer under their names there (conv1 has no bias)."""

    def __init__(self, width, layers, patch_size, input_resolution, embed_dim):
        super().__init__()
        g = input_resolution // patch_size
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn(g * g + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.Sequential(*[_Block(width) for _ in range(layers)])
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, embed_dim))
        _init_blocks(self.transformer.resblocks, width, layers)    # (the visual tower's own scales are the ones above)


class _ClipModel(nn.Module):
    def __init__(self, *dims):
        super().__init__()
        self.visual = _ClipVisual(*dims)


class ClipImageEncoder(nn.Module):
    """Drop-in for the visual half of model.model.CLIPEncoder (frozen, inference).  Parameters keep the reference's names under
    `ClipModel.visual.` (ClipModel.visual.conv1.weight, ClipModel.visual.transformer.resblocks.0.attn.in_proj_weight, ...).
    precision: 'fp16' (fp16 matrix operands, MFMA attention; fp32 accumulation, softmax, LayerNorm and residual stream) or 'fp32'.
    A frame's feature is bitwise the same in any batch and any chunking.  The packed weights are cached and rebuilt whenever a
    parameter changes.  max_frames bounds the frames per device call (and so the workspace); it does not change any result."""

    def __init__(self, width, layers, heads, patch_size, input_resolution, embed_dim, precision='fp16', device='cuda', max_frames=1024):
        super().__init__()
        width, layers, heads = int(width), int(layers), int(heads)
        patch_size, input_resolution = int(patch_size), int(input_resolution)
        _check_dims('ClipImageEncoder', precision, width, heads, layers)
        if patch_size < 1 or input_resolution % patch_size:
            raise NotImplementedError('ClipImageEncoder: input_resolution=%d is not a multiple of patch_size=%d'
                                      % (input_resolution, patch_size))
        L = (input_resolution // patch_size) ** 2 + 1
        if not 2 <= L <= 257:
            raise NotImplementedError('ClipImageEncoder: %d tokens per frame; the attention kernels take 2 .. 257 (ViT-L/14@336 and its '
                                      '577 tokens are not supported)' % L)
        self.device, self.precision = device, precision
        self.width, self.layers, self.heads, self.embed_dim = width, layers, heads, int(embed_dim)
        self.patch_size, self.input_resolution, self.tokens = patch_size, input_resolution, L
        self.max_frames = int(max_frames)
        self.ClipModel = _ClipModel(width, layers, patch_size, input_resolution, self.embed_dim)
        self.to(device)
        self._weights = _Weights(self.ClipModel, precision)

    @staticmethod
    def visual_state_dict(sd):
        """The visual entries of a CLIP state dict (bare, `ClipModel.`- or `clip_model.ClipModel.`-prefixed), as `visual.*` names.
        A ModifiedResNet tower (visual.layer1.*) is refused."""
        for pre in _PREFIXES:
            if any(k.startswith(pre) for k in sd):
                sd = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
                break
        vis = {k: v for k, v in sd.items() if k.startswith('visual.')}
        if 'visual.proj' not in vis:
            if any(k.startswith('visual.layer1.') for k in vis):
                raise NotImplementedError('ClipImageEncoder: a ModifiedResNet visual tower (RN50 / RN101 / RN50x4 ...); only the ViT '
                                          'towers are supported')
            raise ValueError('ClipImageEncoder: no visual.proj in the state dict: not a CLIP ViT checkpoint')
        return vis

    @staticmethod
    def dims(sd):
        """(width, layers, heads, patch_size, input_resolution, embed_dim) the way clip.model.build_model infers them."""
        sd = ClipImageEncoder.visual_state_dict(sd)
        conv = sd['visual.conv1.weight']
        width, patch = int(conv.shape[0]), int(conv.shape[-1])
        layers = len([k for k in sd if k.endswith('.attn.in_proj_weight')])
        grid = round((int(sd['visual.positional_embedding'].shape[0]) - 1) ** 0.5)
        return width, layers, width // 64, patch, patch * grid, int(sd['visual.proj'].shape[1])

    @classmethod
    def from_state_dict(cls, sd, precision='fp16', device='cuda', **kw):
        width, layers, heads, patch, res, embed = cls.dims(sd)
        if width % 64:
            raise NotImplementedError('ClipImageEncoder: width=%d; only a head dim of 64 is supported' % width)
        enc = cls(width, layers, heads, patch, res, embed, precision=precision, device=device, **kw)
        vis = cls.visual_state_dict(sd)
        enc.ClipModel.load_state_dict({k: torch.as_tensor(np.asarray(v.detach().cpu()) if isinstance(v, torch.Tensor) else np.asarray(v),
                                                          dtype=torch.float32) for k, v in vis.items()}, strict=True)
        return enc

    def _model(self):
        """The packed weights and the laff_clip_visual struct, rebuilt when any parameter has changed since the last build."""
        from . import _lib, ops
        m = self.ClipModel.visual
        return self._weights.get(lambda w: _lib.ClipVisual(
            self.width, self.layers, self.heads, self.embed_dim, self.input_resolution, self.patch_size,
            w.packed(m.conv1.weight.reshape(self.width, -1), padded_cols=ops.clip_image_kpad(self.patch_size, self.precision)),
            w.f32(m.class_embedding), w.f32(m.positional_embedding), w.f32(m.ln_pre.weight), w.f32(m.ln_pre.bias),
            w.blocks(m.transformer.resblocks), w.f32(m.ln_post.weight), w.f32(m.ln_post.bias), w.packed(m.proj, transpose=True)))

    def _pixels(self, frames):
        dev = self.ClipModel.visual.proj.device
        x = torch.as_tensor(frames).to(device=dev, dtype=torch.float32).contiguous()
        R = self.input_resolution
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, R, R):
            raise ValueError('frames must be [F, 3, %d, %d], got %s' % (R, R, tuple(x.shape)))
        return x

    def workspace_bytes(self, F):
        from . import ops
        return ops.clip_image_workspace_bytes(F, self.width, self.input_resolution, self.patch_size, self.precision)

    def encode_batch(self, pixels, frame_off=None, frame_off_host=None, out=None, out_mean=None, workspace=None):
        """The device call: pixels [F, 3, R, R] fp32 on the device, optionally frame_off [V+1] int32 (device) + frame_off_host (host)
        for the per-video means; returns (out [F, E], out_mean [V, E] or None).  Allocates nothing when out, out_mean and workspace
        are given."""
        from . import ops
        return ops.clip_image_encode(pixels, frame_off, frame_off_host, self._model(), self.precision, out=out, out_mean=out_mean,
                                     workspace=workspace)

    def _run(self, pixels, counts, max_frames):
        """Frame features [F, E] and the per-video means [V, E] of videos with `counts` frames each, in calls of whole videos of at
        most max_frames frames (a longer video gets a call of its own)."""
        dev = pixels.device
        F, V = pixels.shape[0], len(counts)
        out = torch.empty((F, self.embed_dim), device=dev, dtype=torch.float32)
        mean = torch.empty((V, self.embed_dim), device=dev, dtype=torch.float32)
        off = np.zeros(V + 1, np.int64)
        off[1:] = np.cumsum(counts)
        budget = max(int(max_frames or self.max_frames), 1)
        for v0, v1, ws in _chunks(off, budget, lambda v0, v1: self.workspace_bytes(int(off[v1] - off[v0])), dev):
            f0, f1 = int(off[v0]), int(off[v1])
            roh = (off[v0:v1 + 1] - f0).astype(np.int32)
            self.encode_batch(pixels[f0:f1], torch.from_numpy(roh).to(dev), roh, out=out[f0:f1], out_mean=mean[v0:v1], workspace=ws)
        return out, mean

    def encode_frames(self, frames, max_frames=None):
        """Frames [F, 3, R, R] -> (F, embed_dim) fp32, in calls of at most max_frames frames."""
        x = self._pixels(frames)
        return self._run(x, [1] * x.shape[0], max_frames)[0]

    def _frames(self, vis_origin_frame_tuple):
        counts = [int(t.shape[0]) for t in vis_origin_frame_tuple]
        if any(c < 1 for c in counts):
            raise ValueError('every video needs at least one frame')
        return self._pixels(torch.cat([torch.as_tensor(t) for t in vis_origin_frame_tuple], dim=0)), counts

    def video_features(self, vis_origin_frame_tuple, max_frames=None):
        """(mean [V, E], frames [V, Fmax, E] zero-padded, mask_tensor [V, Fmax] fp32): the layout collate_vision gives a FrameLAFF
        model's vis_feat_dict / vis_frame_feat_dict, on the device."""
        x, counts = self._frames(vis_origin_frame_tuple)
        feats, mean = self._run(x, counts, max_frames)
        V, Fmax = len(counts), max(counts)
        cnt = torch.as_tensor(counts, device=x.device)
        mask = (torch.arange(Fmax, device=x.device)[None, :] < cnt[:, None]).float()
        frames = torch.zeros((V, Fmax, self.embed_dim), device=x.device, dtype=torch.float32)
        frames[mask.bool()] = feats
        return mean, frames, mask

    def preprocessor(self, kind='clip'):
        """The FramePreprocessor of this encoder's input_resolution and device (one per kind, kept: its tap tables are cached)."""
        from .frame_prep import FramePreprocessor
        pre = self.__dict__.setdefault('_preprocessors', {})
        if kind not in pre:
            pre[kind] = FramePreprocessor(self.input_resolution, kind=kind, device=self.ClipModel.visual.proj.device)
        return pre[kind]

    def encode_raw_frames(self, frames, kind='clip', max_frames=None):
        """Decoded RGB uint8 frames of any size (a list of [H, W, 3] arrays / tensors or one [F, H, W, 3] tensor) -> (F, embed_dim) fp32:
        the preprocessing of `kind` ('clip' / 'slip', laff_amd/frame_prep.py) on the device, then encode_frames."""
        return self.encode_frames(self.preprocessor(kind)(frames), max_frames)

    def video_features_raw(self, list_of_videos, kind='clip', max_frames=None):
        """video_features of videos given as decoded uint8 frames: one list of [H, W, 3] frames (or one [F_v, H, W, 3] tensor) per
        video."""
        pre = self.preprocessor(kind)
        vids = [pre._frame_list(v) for v in list_of_videos]
        if any(len(v) < 1 for v in vids):
            raise ValueError('every video needs at least one frame')
        pix = pre([f for v in vids for f in v])
        off = np.concatenate([[0], np.cumsum([len(v) for v in vids])])
        return self.video_features(tuple(pix[off[i]:off[i + 1]] for i in range(len(vids))), max_frames)

    def forward(self, caption_feat_dict=None, vis_origin_frame_tuple=None, frame_agg_method='mean'):
        """The visual half of CLIPEncoder.forward: {'visual_features': [V, E]}, the mean of each video's frame features (the text
        half is clip_text.ClipTxtEncoder; caption_feat_dict is not read here)."""
        output = {}
        if vis_origin_frame_tuple is not None:
            if frame_agg_method != 'mean':
                raise Exception("frame_agg_method is not applied.")
            x, counts = self._frames(vis_origin_frame_tuple)
            output['visual_features'] = self._run(x, counts, None)[1]
        return output


def _is_raw(vis_origin_frame_tuple):
    """True when the tuple holds decoded uint8 frames (every video: a uint8 array / tensor or a list of them)."""
    def raw(v):
        if isinstance(v, (list, tuple)):
            return len(v) > 0 and all(raw(f) for f in v)
        return isinstance(v, (np.ndarray, torch.Tensor)) and v.dtype in (np.uint8, torch.uint8)
    return len(vis_origin_frame_tuple) > 0 and all(raw(v) for v in vis_origin_frame_tuple)


class ClipFrameLoader(object):
    """Wraps a loader of collate_vision batches (dicts with 'vis_feat_dict', 'vis_frame_feat_dict', 'vis_origin_frame_tuple', ...):
    encodes each batch's frames and puts the per-video mean into vis_feat_dict[mean_name] and the zero-padded per-frame features into
    vis_frame_feat_dict[frame_name] (+ 'mask_tensor'), all on the device.  mean_name / frame_name None: that entry is not filled.
    A batch whose vis_origin_frame_tuple holds decoded uint8 frames (per video a [F_v, H, W, 3] tensor / array or a list of [H, W, 3]
    frames) goes through `preprocessor` first (None: the encoder's own 'clip' one); fp32 tuples are encoded as they are."""

    def __init__(self, vis_loader, encoder, mean_name='mean_clip_frame_feat_ViT-B_32,os', frame_name='clip_frame_feat_ViT-B_32,os',
                 max_frames=None, preprocessor=None):
        self.vis_loader, self.encoder, self.preprocessor = vis_loader, encoder, preprocessor
        self.mean_name, self.frame_name, self.max_frames = mean_name, frame_name, max_frames
        for a in ('batch_size', 'dataset'):
            if hasattr(vis_loader, a):
                setattr(self, a, getattr(vis_loader, a))

    def __len__(self):
        return len(self.vis_loader)

    def __iter__(self):
        for batch in self.vis_loader:
            batch = dict(batch)
            frames = batch.get('vis_origin_frame_tuple')
            if frames is None or any(f is None for f in frames):
                raise ValueError('ClipFrameLoader: the batch carries no vis_origin_frame_tuple')
            if _is_raw(frames):
                pre = self.preprocessor if self.preprocessor is not None else self.encoder.preprocessor()
                vids = [pre._frame_list(v) for v in frames]
                off = np.concatenate([[0], np.cumsum([len(v) for v in vids])])
                pix = pre([f for v in vids for f in v])
                frames = tuple(pix[off[i]:off[i + 1]] for i in range(len(vids)))
            mean, feats, mask = self.encoder.video_features(frames, self.max_frames)
            if self.mean_name is not None:
                batch['vis_feat_dict'] = dict(batch.get('vis_feat_dict') or {}, **{self.mean_name: mean})
            if self.frame_name is not None:
                batch['vis_frame_feat_dict'] = dict(batch.get('vis_frame_feat_dict') or {}, **{self.frame_name: feats, 'mask_tensor': mask})
            yield batch
