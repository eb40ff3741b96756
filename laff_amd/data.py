"""Bulk feature loading for the retrieval path.

The reference's VisionDataset / TextDataset (/root/reference/data_provider.py:380-618) do one open/seek/fromfile and a
Python-list round trip PER ITEM PER FEATURE through BigFile.read_one, then collate 64 items at a time.  Once the GPU pass
takes ~1 ms that dominates wall time.  These loaders keep the batch-dict layout `predict()` consumes
(`collate_vision` :38-73, `collate_text` :76-89) and the loader surface it touches (`.dataset.length`, `len(.dataset)`,
`.batch_size`, `len(loader)`), but gather whole batches of rows with one mmap take into pinned host memory followed by
an asynchronous H2D copy.  On-disk format unchanged (txt2bin.py:64-74: float32 rows, id.txt, shape.txt).

Training has a loader of its own further down: `pair_provider(params)` / `PairProvider` keep the whole training set on the device and
gather each batch with one launch.
"""
import os

import numpy as np
import torch

from .bigfile import BigFile


def write_bigfile(datadir, ids, matrix):
    """feature.bin / id.txt / shape.txt as txt2bin.py writes them (newline separated ids)."""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    assert matrix.ndim == 2 and matrix.shape[0] == len(ids)
    os.makedirs(datadir, exist_ok=True)
    matrix.tofile(os.path.join(datadir, 'feature.bin'))
    with open(os.path.join(datadir, 'id.txt'), 'w') as f:
        f.write('\n'.join(ids) + '\n')
    with open(os.path.join(datadir, 'shape.txt'), 'w') as f:
        f.write('%d %d' % matrix.shape)


class NpyFeatures:
    """Features kept as a numpy file instead of a BigFile directory -- the two forms the reference reads: a pickled
    `{id: vector}` dict (`np.load(path, allow_pickle=True).item()`, trainer.py:144-148) or a plain (N, D) array next to an id list.
    Exposes the part of the BigFile surface the bulk loaders use (`names`, `ndims`, `nr_of_images`, `shape()`, `read_matrix`,
    `read`, `read_one`), so it can stand wherever a BigFile is expected in BulkVisLoader / BulkTxtLoader."""

    def __init__(self, path_or_array, ids=None):
        obj = np.load(path_or_array, allow_pickle=True) if isinstance(path_or_array, str) else path_or_array
        if isinstance(obj, np.ndarray) and obj.dtype == object and obj.shape == ():
            obj = obj.item()
        if isinstance(obj, dict):
            self.names = list(obj.keys())
            self._m = np.ascontiguousarray(np.stack([np.asarray(obj[k], dtype=np.float32).reshape(-1) for k in self.names]))
        else:
            if ids is None:
                raise ValueError('a plain (N, D) array needs the list of ids of its rows')
            self.names = list(ids)
            self._m = np.ascontiguousarray(np.asarray(obj, dtype=np.float32))
            if self._m.ndim != 2 or self._m.shape[0] != len(self.names):
                raise ValueError('array of shape %s does not match %d ids' % (self._m.shape, len(self.names)))
        self.name2index = dict(zip(self.names, range(len(self.names))))
        self.nr_of_images, self.ndims = self._m.shape

    def _matrix(self):
        return self._m

    def shape(self):
        return [self.nr_of_images, self.ndims]

    def read_matrix(self, names, out=None):
        idx = np.fromiter((self.name2index[n] for n in names), dtype=np.int64, count=len(names))
        if out is None:
            out = np.empty((len(idx), self.ndims), dtype=np.float32)
        np.take(self._m, idx, axis=0, out=out)
        return out

    def read(self, requested, isname=True):
        """BigFile.read semantics (bigfile.py:187-213): duplicates removed, unknown ids dropped, rows in storage order."""
        idx = sorted({self.name2index[r] for r in requested if r in self.name2index} if isname else set(requested))
        return [self.names[i] for i in idx], [self._m[i].tolist() for i in idx]

    def read_one(self, name):
        renamed, vectors = self.read([name])
        return vectors[0]


class _Dataset:
    def __init__(self, n, captions=None):
        self.length = n
        self.captions = captions or {}

    def __len__(self):
        return self.length


def _to_device(arr, device, pin):
    t = torch.from_numpy(arr)
    if device is None or torch.device(device).type == 'cpu':
        return t
    if pin:
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


class BulkVisLoader:
    """Video side: yields `collate_vision`-shaped dicts for `batch_size` videos at a time, tensors already on `device`."""

    def __init__(self, vis_feat_files, vis_ids, batch_size=8192, device='cuda', vis_frame_feat_dicts=None, max_frame=200,
                 pin_memory=True):
        self.files = dict(vis_feat_files or {})
        self.vis_ids = list(vis_ids)
        self.batch_size = int(batch_size)
        self.device, self.pin = device, pin_memory
        self.dataset = _Dataset(len(self.vis_ids))
        self.frame_files = dict(vis_frame_feat_dicts or {})
        self.max_frame = max_frame
        self._frames = {}
        for name, bf in self.frame_files.items():      # video id -> frame row indices in frame order (data_provider.py:432-449)
            groups = {}
            for row, fid in enumerate(bf.names):
                vid, num = fid.rsplit('_', 1)
                groups.setdefault(vid, []).append((int(num), row))
            self._frames[name] = {v: [r for _, r in sorted(lst)][:max_frame] for v, lst in groups.items()}

    def __len__(self):
        return (len(self.vis_ids) + self.batch_size - 1) // self.batch_size

    def whole(self):
        """The whole collection as ONE batch dict: model.retrieve() / predict() then run each tower once over the full matrices (one
        grouped FC launch, one fuse launch per side) instead of once per batch."""
        return next(self._batches(max(1, len(self.vis_ids))), None)

    def __iter__(self):
        return self._batches(self.batch_size)

    def _batches(self, batch_size):
        n = len(self.vis_ids)
        for s in range(0, n, batch_size):
            ids = self.vis_ids[s:s + batch_size]
            feats = {name: _to_device(bf.read_matrix(ids), self.device, self.pin) for name, bf in self.files.items()}
            frame_dict = {}
            if self.frame_files:
                first = next(iter(self._frames))
                lens = np.array([len(self._frames[first][v]) for v in ids], dtype=np.int64)
                fmax = int(lens.max())
                mask = (np.arange(fmax)[None, :] < lens[:, None]).astype(np.float32)
                frame_dict['mask_tensor'] = _to_device(mask, self.device, self.pin)
                for name, bf in self.frame_files.items():
                    out = np.zeros((len(ids), fmax, bf.ndims), dtype=np.float32)
                    mm = bf._matrix()
                    for i, v in enumerate(ids):
                        rows = self._frames[name][v]
                        out[i, :len(rows)] = mm[rows]
                    frame_dict[name] = _to_device(out, self.device, self.pin)
            yield {'vis_feat_dict': feats, 'idxs': list(range(s, s + len(ids))), 'vis_ids': tuple(ids),
                   'vis_frame_feat_dict': frame_dict, 'vis_origin_frame_tuple': (None,) * len(ids)}


class BulkTxtLoader:
    """Text side: yields (caption_feat_dict, idxs, cap_ids) like `collate_text`, in caption-file order.

    `text_feat_files`: {caption_feat_dict key (e.g. 'CLIP_encoding', 'bow_encoding'): BigFile keyed by caption id}.
    (The reference sorts each batch by token count for its GRU's packed sequences; with pre-extracted features the
    order is irrelevant and rows stay in file order -- `txt_ids` returned by predict() reflects that.)"""

    def __init__(self, capfile_or_pairs, text_feat_files, batch_size=16384, device='cuda', pin_memory=True):
        if isinstance(capfile_or_pairs, str):
            pairs = []
            with open(capfile_or_pairs) as reader:                 # data_provider.py:548-559
                for line in reader:
                    if line.strip() == '':
                        continue
                    parts = line.strip().split(None, 1)
                    pairs.append((parts[0], parts[1] if len(parts) > 1 else ''))
        else:
            pairs = list(capfile_or_pairs)
        self.cap_ids = [p[0] for p in pairs]
        self.files = dict(text_feat_files)
        self.batch_size = int(batch_size)
        self.device, self.pin = device, pin_memory
        self.dataset = _Dataset(len(pairs), dict(pairs))

    def __len__(self):
        return (len(self.cap_ids) + self.batch_size - 1) // self.batch_size

    def whole(self):
        """All captions as ONE (caption_feat_dict, idxs, cap_ids) batch (see BulkVisLoader.whole)."""
        return next(self._batches(max(1, len(self.cap_ids))), None)

    def __iter__(self):
        return self._batches(self.batch_size)

    def _batches(self, batch_size):
        n = len(self.cap_ids)
        for s in range(0, n, batch_size):
            ids = self.cap_ids[s:s + batch_size]
            cap = {'caption': [self.dataset.captions[i] for i in ids]}
            for key, bf in self.files.items():
                cap[key] = _to_device(bf.read_matrix(ids), self.device, self.pin)
            yield cap, list(range(s, s + len(ids))), tuple(ids)


# ---- the training pair provider -----------------------------------------------------------------------------
# The reference's pair_provider (data_provider.py:621-698, :834-843) reads every item of every batch from the feature files, stacks
# and pads on the host, and the text encoders tokenise the batch's strings again at every step.  Nothing of a training set changes
# between steps: here features, token ids and the caption-to-video map are read, tokenised and uploaded ONCE (PairPlan on the host,
# PairProvider on the device); a batch is then an index list, one pinned int32 control block, one H2D copy and one launch
# (ops.batch_assemble).

def read_capfile(capfile):
    """(cap_ids, texts) of a caption file as TextDataset reads it (data_provider.py:551-561): blank lines skipped, a line without a
    text is an empty caption, a repeated id stays in the list and every occurrence carries the LAST text."""
    cap_ids, captions = [], {}
    with open(capfile) as reader:
        for line in reader.readlines():
            if line.strip() == '':
                continue
            parts = line.strip().split(None, 1)
            captions[parts[0]] = parts[1] if len(parts) > 1 else ''
            cap_ids.append(parts[0])
    return cap_ids, [captions[c] for c in cap_ids]


def frame_rows_of(bf, max_frame):
    """{video id: file rows of its frames} of a frame feature file as the reference's PairDataset reads them: the frame set is the
    first `max_frame` frame ids by trailing number (data_provider.py:430-446, :475-477), their ORDER is BigFile.read's -- ascending
    file row, duplicates dropped (bigfile.py:194-204) -- not the frame number's."""
    groups = {}
    for fid in bf.names:
        groups.setdefault('_'.join(fid.split('_')[0:-1]), []).append(fid)
    out = {}
    for vid, lst in groups.items():
        lst.sort(key=lambda x: int(x.split('_')[-1]))
        out[vid] = np.array(sorted({bf.name2index[f] for f in lst[:max_frame]}), dtype=np.int64)
    return out


def _align4(n):
    return (n + 3) // 4 * 4


class BatchLayout:
    """Where a batch's integers sit in its control block (int32 indices), and what the host kept of them."""
    __slots__ = ('B', 'rows', 'cap_at', 'vid_at', 'crow_at', 'fmax_at', 'fmax', 'nnz', 'colptr_at', 'csc_rows_at', 'csc_vals_at', 'total')


class PairPlan:
    """The host half of PairProvider: everything that can be decided without a GPU.  Reads the caption file, maps captions to
    videos, lays the frame sets out video-major, tokenises every caption once through the encoders' vectorisers, draws the batches
    and fills their control blocks.  `params` is the reference's dict (see pair_provider)."""

    def __init__(self, params):
        from . import txt2vec as T
        config = params.get('config')
        if config is not None and getattr(config, 'frame_loader', False):
            raise NotImplementedError('pair_provider: config.frame_loader (raw-frame loading) is not supported')
        for key in ('capfile_task2', 'capfile_task3', 'vis_muti_feat_dicts'):
            if params.get(key) is not None:
                raise NotImplementedError('pair_provider: %s is not supported%s' % (
                    key, ' (the task-3 negation captions and their captions_task3 / captions_task3_mask fields)'
                    if key == 'capfile_task3' else ''))
        self.batch_size = int(params.get('batch_size', 1))
        if not 1 <= self.batch_size <= 4096:
            raise ValueError('pair_provider: batch_size=%d; a batch has 1 to 4096 rows' % self.batch_size)
        self.shuffle, self.sampler = bool(params.get('shuffle', False)), params.get('sampler')
        if self.shuffle and self.sampler is not None:
            raise ValueError('pair_provider: sampler option is mutually exclusive with shuffle')          # torch's DataLoader rule
        self.cap_ids, self.texts = read_capfile(params['capfile'])
        n = len(self.cap_ids)
        #: tokens per caption under the reference's tokeniser rules (collate_pair sorts a batch by them, data_provider.py:93)
        self.ntok = np.array([len(T.tokenize(t)) for t in self.texts], dtype=np.int64)
        # ---- captions -> videos
        self.vis_ids, index = [], {}
        self.cap_vid = np.empty(n, dtype=np.int32)
        for i, cap_id in enumerate(self.cap_ids):
            vid = cap_id.split('#', 1)[0]
            if vid not in index:
                index[vid] = len(self.vis_ids)
                self.vis_ids.append(vid)
            self.cap_vid[i] = index[vid]
        first_cap = {}
        for i, v in enumerate(self.cap_vid):
            first_cap.setdefault(int(v), self.cap_ids[i])
        self.vis_files = dict(params.get('vis_feat_files') or {})
        for name, bf in self.vis_files.items():
            for v, vid in enumerate(self.vis_ids):
                if vid not in bf.name2index:
                    raise KeyError("video '%s' of caption '%s' is missing from the feature file '%s'" % (vid, first_cap[v], name))
        # ---- frames, video-major in BigFile.read's order
        self.frame_files = dict(params.get('vis_frame_feat_dicts') or {})
        self.frame_rows, self.seg_off = {}, None
        if self.frame_files:
            max_frame = int(params['max_frame'])
            lens0 = name0 = None
            for name, bf in self.frame_files.items():
                groups = frame_rows_of(bf, max_frame)
                for v, vid in enumerate(self.vis_ids):
                    if vid not in groups:
                        raise KeyError("video '%s' of caption '%s' has no frame in the frame feature file '%s'" % (vid, first_cap[v], name))
                lens = np.array([len(groups[vid]) for vid in self.vis_ids], dtype=np.int64)
                if lens0 is None:
                    lens0, name0 = lens, name
                elif not np.array_equal(lens, lens0):
                    bad = int(np.nonzero(lens != lens0)[0][0])
                    raise ValueError("frame feature '%s' has %d frames for video '%s', '%s' has %d: the mask comes from the first frame "
                                     "feature, so the per-video counts must agree" % (name, lens[bad], self.vis_ids[bad], name0, lens0[bad]))
                self.frame_rows[name] = np.concatenate([groups[vid] for vid in self.vis_ids]) if self.vis_ids else np.zeros(0, np.int64)
            self.frame_len = lens0
            self.seg_off = np.concatenate([[0], np.cumsum(lens0)]).astype(np.int32)
        # ---- pre-calculated caption features (data_provider.py:565-574)
        self.cap_files = {}
        enc_cfg = getattr(config, 'text_encoding', None) or {}
        for name, each in enc_cfg.items():
            if 'no' in each['name'] or 'dir_name' not in each:
                continue
            self.cap_files[name] = BigFile(os.path.join(os.path.dirname(params['capfile']), each['dir_name']))
        for name, bf in self.cap_files.items():
            for cap_id in self.cap_ids:
                if cap_id not in bf.name2index:
                    raise KeyError("caption '%s' is missing from the pre-calculated feature '%s'" % (cap_id, name))
        # ---- the encoders' vectorisers, once per caption
        self.encoders = dict(params.get('encoders') or {})
        self.bow = None                         # (encoder, crow, col, val): the host CSR of all captions
        self.gru_ids, self.w2v_rows, self.w2v_enc, self.netvlad_enc = {}, {}, [], []    # {encoder: [ids]}, {W2Vec: [raw_ids]}
        for name, enc in self.encoders.items():
            if isinstance(enc, T.BoWTxtEncoder):
                if self.bow is not None:
                    raise ValueError("pair_provider: encoders holds two bag-of-words encoders ('%s'); one is supported" % name)
                rows = [enc.t2v_bow._ids(t) for t in self.texts]
                crow = np.zeros(n + 1, np.int64)
                crow[1:] = np.cumsum([len(c) for c, _ in rows])
                if crow[-1] >= 2 ** 31:
                    raise ValueError('pair_provider: the bag-of-words matrix has %d entries, 32-bit indexing holds 2^31 - 1' % crow[-1])
                col = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]) if n else np.zeros(0, np.int32)
                val = np.concatenate([np.asarray(v, np.float32) for _, v in rows]) if n else np.zeros(0, np.float32)
                self.bow = (enc, crow.astype(np.int32), col.astype(np.int32), val.astype(np.float32))
            elif isinstance(enc, T.GruTxtEncoder):
                self.gru_ids[enc] = [enc.t2v_idx.encoding(t) for t in self.texts]
            elif isinstance(enc, (T.W2VTxtEncoder, T.NetVLADTxtEncoder)):
                (self.w2v_enc if isinstance(enc, T.W2VTxtEncoder) else self.netvlad_enc).append(enc)
                if isinstance(enc, T.NetVLADTxtEncoder) and enc.t2v_w2v not in self.w2v_rows:
                    self.w2v_rows[enc.t2v_w2v] = [(np.asarray(r, np.int32), k) for r, k in map(enc.t2v_w2v.raw_ids, self.texts)]
            else:
                raise TypeError("pair_provider: encoders['%s'] is a %s; BoWTxtEncoder, W2VTxtEncoder, GruTxtEncoder and "
                                "NetVLADTxtEncoder of laff_amd.txt2vec are supported" % (name, type(enc).__name__))
        # ---- the control block: the most integers a batch can need
        bs = min(self.batch_size, max(n, 1))
        need = 3 * bs + 2
        if self.bow is not None:
            row_len = np.sort(np.diff(self.bow[1].astype(np.int64)))[::-1]
            self.max_batch_nnz = int(row_len[:bs].sum())
            need = _align4(need) + _align4(self.bow[0].t2v_bow.ndims + 1) + 2 * _align4(self.max_batch_nnz)
        self.control_ints = _align4(need)

    def __len__(self):
        return len(self.cap_ids)

    def feature_bytes(self):
        """{what: bytes} of every array the provider keeps on the device."""
        n, out = len(self.cap_ids), {}
        for name, bf in self.vis_files.items():
            out['vis_feat_files[%s]' % name] = 4 * len(self.vis_ids) * bf.ndims
        for name, bf in self.frame_files.items():
            out['vis_frame_feat_dicts[%s]' % name] = 4 * len(self.frame_rows[name]) * bf.ndims
        if self.frame_files:
            out['frame offsets'] = 4 * len(self.seg_off)
        for name, bf in self.cap_files.items():
            out['captions[%s]' % name] = 4 * n * bf.ndims
        if self.bow is not None:
            out['bag of words (CSR)'] = 4 * (n + 1) + 8 * len(self.bow[2])
        for enc in self.w2v_enc:
            out['word2vec means [%d]' % enc.t2v_w2v.ndims] = 4 * n * enc.t2v_w2v.ndims
        return out

    def batches(self):
        """The index lists of one epoch, as torch's DataLoader draws them for the reference: a RandomSampler over the captions with
        shuffle=True (a new permutation from torch's global generator at every call), the given sampler otherwise, in file order
        without either; BatchSampler with drop_last=False.  A DataLoader draws one number (its workers' base seed) from the global
        generator when an iterator is made, before the sampler draws its own: so does this, and under torch.manual_seed the epoch
        orders are the DataLoader's."""
        from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
        sampler = self.sampler
        if sampler is None:
            sampler = RandomSampler(range(len(self))) if self.shuffle else SequentialSampler(range(len(self)))
        torch.empty((), dtype=torch.int64).random_()
        return iter(BatchSampler(sampler, self.batch_size, False))

    def order(self, indices):
        """The batch's caption indices in collate_pair's row order: by token count, longest first, stable."""
        idx = np.asarray(list(indices), dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError('pair_provider: the sampler gave an index outside [0, %d)' % len(self))
        return idx[np.argsort(-self.ntok[idx], kind='stable')]

    def fill(self, indices, control):
        """Writes the control block of the batch `indices` into `control` (a numpy int32 array of at least control_ints) and returns
        its BatchLayout."""
        rows = self.order(indices)
        B = len(rows)
        lay = BatchLayout()
        lay.B, lay.rows = B, rows
        lay.cap_at, lay.vid_at, lay.crow_at, lay.fmax_at = 0, B, 2 * B, 3 * B + 1
        control[0:B] = rows
        control[B:2 * B] = self.cap_vid[rows]
        lay.fmax = int(self.frame_len[self.cap_vid[rows]].max()) if self.frame_files else 0
        lay.nnz, lay.total = 0, 3 * B + 2
        control[lay.crow_at:lay.crow_at + B + 1] = 0
        control[lay.fmax_at] = lay.fmax
        lay.colptr_at = lay.csc_rows_at = lay.csc_vals_at = -1
        if self.bow is not None:
            enc, crow, col, val = self.bow
            start, length = crow[rows].astype(np.int64), (crow[rows + 1] - crow[rows]).astype(np.int64)
            crow_dst = np.concatenate([[0], np.cumsum(length)])
            control[lay.crow_at:lay.crow_at + B + 1] = crow_dst
            nnz = lay.nnz = int(crow_dst[-1])
            # the batch's entries in CSR order, from the host copy: what the transposed pattern is formed from (ops.csr_transpose)
            src = np.repeat(start - crow_dst[:-1], length) + np.arange(nnz)
            bcol, brow = col[src], np.repeat(np.arange(B, dtype=np.int32), length)
            order = np.argsort(bcol.astype(np.int64), kind='stable')
            Dk = enc.t2v_bow.ndims
            lay.colptr_at = _align4(lay.total)
            lay.csc_rows_at = lay.colptr_at + _align4(Dk + 1)
            lay.csc_vals_at = lay.csc_rows_at + _align4(nnz)
            lay.total = lay.csc_vals_at + _align4(nnz)
            control[lay.colptr_at:lay.colptr_at + Dk + 1] = np.searchsorted(bcol[order], np.arange(Dk + 1), side='left')
            control[lay.csc_rows_at:lay.csc_rows_at + nnz] = brow[order]
            control[lay.csc_vals_at:lay.csc_vals_at + nnz] = val[src][order].view(np.int32)
        return lay


class _ControlSlot:
    def __init__(self, ints):
        self.tensor = torch.empty(ints, dtype=torch.int32).pin_memory()
        self.array = self.tensor.numpy()
        self.event = None


class PairProvider:
    """The reference's pair_provider over a device-resident training set: iterating it yields `collate_pair`-shaped dicts
    (data_provider.py:92-152) whose tensors are fresh device tensors, gathered by one ops.batch_assemble launch per batch.

    params: the reference's dict -- vis_feat_files {name: BigFile}, vis_frame_feat_dicts {name: BigFile} with max_frame, capfile,
    config (its text_encoding entries with a dir_name are read as pre-calculated caption features, data_provider.py:565-574),
    batch_size, shuffle, sampler; pin_memory and num_workers are accepted and ignored.  Added here: device (default 'cuda'), encoders
    {name: the model's txt2vec encoder object} and max_resident_bytes (None: no limit).

    With `encoders` every caption is tokenised once at build and each batch carries the encoders' prepared inputs under
    captions[txt2vec.PREPARED_KEY] (see there); the strings stay in captions['caption'].
    A set that does not fit max_resident_bytes is refused with MemoryError before anything is allocated: there is no host fallback."""

    def __init__(self, params):
        device = torch.device(params.get('device', 'cuda'))
        if device.type != 'cuda':
            raise RuntimeError("pair_provider: device must be a CUDA (ROCm) device, got '%s': laff_amd has no CPU path" % device)
        self.plan = PairPlan(params)
        p = self.plan
        self.device, self.batch_size = device, p.batch_size
        self.dataset = _Dataset(len(p), dict(zip(p.cap_ids, p.texts)))
        sizes = p.feature_bytes()
        limit = params.get('max_resident_bytes')
        if limit is not None and sum(sizes.values()) > int(limit):
            raise MemoryError('pair_provider: the training set needs %d bytes on the device, max_resident_bytes is %d: %s' % (
                sum(sizes.values()), int(limit), ', '.join('%s %d' % kv for kv in sizes.items())))

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self._vis = {name: up(bf.read_matrix(p.vis_ids)) for name, bf in p.vis_files.items()}
        self._frames = {name: up(bf.read_matrix([bf.names[r] for r in p.frame_rows[name]])) for name, bf in p.frame_files.items()}
        self._seg_off = up(p.seg_off) if p.frame_files else None
        self._cap = {name: up(bf.read_matrix(p.cap_ids)) for name, bf in p.cap_files.items()}
        self._bow = tuple(up(a) for a in p.bow[1:]) if p.bow is not None else None
        self._w2v = {}
        for enc in p.w2v_enc:                     # the existing encode, in chunks: a caption's row does not depend on its batch
            if enc.t2v_w2v not in self._w2v:
                parts = [enc.t2v_w2v.encode(p.texts[s:s + 4096], device) for s in range(0, len(p), 4096)]
                self._w2v[enc.t2v_w2v] = torch.cat(parts, 0) if parts else torch.zeros((0, enc.t2v_w2v.ndims), device=device)
        self._slots, self._next = [_ControlSlot(p.control_ints) for _ in range(4)], 0

    @property
    def resident_bytes(self):
        """Bytes of the device arrays the provider holds."""
        ts = list(self._vis.values()) + list(self._frames.values()) + list(self._cap.values()) + list(self._w2v.values())
        ts += list(self._bow or ()) + ([self._seg_off] if self._seg_off is not None else [])
        return sum(t.numel() * t.element_size() for t in ts)

    def __len__(self):
        return (len(self.plan) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for indices in self.plan.batches():
            yield self.batch(indices)

    def batch(self, indices):
        """The batch of the given caption indices (rows in collate_pair's order): fresh tensors, one H2D copy, one launch per 16 jobs."""
        from . import ops
        from .txt2vec import PREPARED_KEY, IdxVec, W2Vec
        p, dev = self.plan, self.device
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        if slot.event is not None:
            slot.event.synchronize()              # the copy that last read this pinned block has long finished; wait if it has not
        lay = p.fill(indices, slot.array)
        B = lay.B
        control = slot.tensor[:lay.total].to(dev, non_blocking=True)
        slot.event = torch.cuda.Event()
        slot.event.record()

        def new(*shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev)
        jobs, vis_feats, frame_dict, prepared = [], {}, {}, {}
        rows = lay.rows
        captions = {'caption': [p.texts[i] for i in rows]}
        for name, src in self._vis.items():
            vis_feats[name] = new(B, src.shape[1])
            jobs.append(('rows', src, lay.vid_at, vis_feats[name]))
        if self._frames:
            mask = frame_dict['mask_tensor'] = new(B, lay.fmax)
            for name, src in self._frames.items():
                frame_dict[name] = new(B, lay.fmax, src.shape[1])
                jobs.append(('ragged', src, self._seg_off, lay.vid_at, frame_dict[name], mask))
                mask = None                        # the first frame job writes it
        for name, src in self._cap.items():
            captions[name] = new(B, src.shape[1])
            jobs.append(('rows', src, lay.cap_at, captions[name]))
        for enc in p.w2v_enc:
            src = self._w2v[enc.t2v_w2v]
            prepared[enc] = new(B, src.shape[1])
            jobs.append(('rows', src, lay.cap_at, prepared[enc]))
        if self._bow is not None:
            enc = p.bow[0]
            col, val = new(lay.nnz, dtype=torch.int32), new(lay.nnz)
            jobs.append(('csr', self._bow, lay.cap_at, lay.crow_at, (col, val)))
            x = torch.sparse_csr_tensor(control[lay.crow_at:lay.crow_at + B + 1], col, val, size=(B, enc.t2v_bow.ndims))
            if enc.with_csc:
                x.laff_csc = (control[lay.colptr_at:lay.colptr_at + enc.t2v_bow.ndims + 1],
                              control[lay.csc_rows_at:lay.csc_rows_at + lay.nnz],
                              control[lay.csc_vals_at:lay.csc_vals_at + lay.nnz].view(torch.float32))
            prepared[enc] = x
        host = slot.array[:lay.total]
        for s in range(0, len(jobs), 16):
            ops.batch_assemble(jobs[s:s + 16], control, host, B)
        for enc, ids in p.gru_ids.items():
            prepared[enc] = enc.to_device(IdxVec.batch_ids([ids[i] for i in rows]))
        for enc in p.netvlad_enc:
            stored = p.w2v_rows[enc.t2v_w2v]
            prepared[enc] = enc.to_device(*W2Vec.ragged_rows([stored[i] for i in rows]))
        if prepared:
            captions[PREPARED_KEY] = prepared
        vids = p.cap_vid[rows]
        return {'vis_feats': vis_feats, 'vis_muti_feat': None, 'vis_frame_feat_dict': frame_dict,
                'vis_origin_frame_tuple': (None,) * B, 'captions': captions, 'captions_task2': None, 'idxs': [int(i) for i in rows],
                'vis_ids': tuple(p.vis_ids[v] for v in vids), 'cap_ids': tuple(p.cap_ids[i] for i in rows)}


def pair_provider(params):
    """Drop-in for the reference's data_provider.pair_provider(params): see PairProvider."""
    return PairProvider(params)
