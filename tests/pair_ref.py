"""Plain numpy restatements for the training pair provider, independent of laff_amd.data's own planning:

    collate(ds, indices)   the reference's PairDataset.__getitem__ + collate_pair (data_provider.py:92-152, :621-698) on a dataset
                           held as arrays (the fixture's layout: tests/golden/pair_batches.npz, tools/gen_golden_pairs.py)
    rows_ref / ragged_ref / csr_ref   what the three job kinds of laff_batch_assemble write

and the helpers the host and GPU tests share: the fixture as a dataset, the dataset written to disk as the provider reads it.
"""
import functools
import os
import re
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CAP_DIRS = {'CLIP_encoding': 'clip_text'}


def n_tokens(text):
    """len(TextTool.tokenize(text)) (textlib.py:27-45: clean, English, stop words kept)."""
    return len(re.sub(r'[^A-Za-z0-9]', ' ', text.replace('\r', ' ')).strip().lower().split())


def parse_capfile(text):
    ids, cap = [], {}
    for line in text.split('\n'):
        if line.strip() == '':
            continue
        parts = line.strip().split(None, 1)
        cap[parts[0]] = parts[1] if len(parts) > 1 else ''
        ids.append(parts[0])
    return ids, [cap[i] for i in ids]


class Dataset:
    """capfile text, {name: (ids, matrix)} for video, frame and caption features, max_frame."""

    def __init__(self, capfile, vis, frame, cap, max_frame):
        self.capfile, self.vis, self.frame, self.cap, self.max_frame = capfile, vis, frame, cap, int(max_frame)
        self.cap_ids, self.texts = parse_capfile(capfile)


@functools.lru_cache(maxsize=None)
def fixture():
    """(arrays, Dataset) of tests/golden/pair_batches.npz."""
    z = np.load(os.path.join(GOLDEN, 'pair_batches.npz'))
    arrays = {k: z[k] for k in z.files}

    def feats(kind):
        names = sorted({k.split('/')[1] for k in arrays if k.startswith(kind + '/')})
        return {n: ([str(s) for s in arrays['%s/%s/ids' % (kind, n)]], arrays['%s/%s/matrix' % (kind, n)]) for n in names}
    return arrays, Dataset(str(arrays['capfile']), feats('vis'), feats('frame'), feats('cap'), arrays['meta'][2])


def frame_rows(ids, vid, max_frame):
    """File rows of a video's frames as VisionDataset.get_feat_by_id reads them: the first max_frame ids by trailing number, then
    BigFile.read's order (ascending file row, a set)."""
    mine = [f for f in ids if '_'.join(f.split('_')[0:-1]) == vid]
    mine.sort(key=lambda x: int(x.split('_')[-1]))
    index = dict(zip(ids, range(len(ids))))
    return sorted({index[f] for f in mine[:max_frame]})


def collate(ds, indices):
    """The batch dict of collate_pair over the items `indices`, numpy arrays in place of tensors."""
    items = []
    for i in indices:
        cap_id = ds.cap_ids[i]
        vid = cap_id.split('#', 1)[0]
        vis = {n: m[ids.index(vid)] for n, (ids, m) in ds.vis.items()}
        frames = {n: m[frame_rows(ids, vid, ds.max_frame)] for n, (ids, m) in ds.frame.items()}
        cap = {n: m[ids.index(cap_id)] for n, (ids, m) in ds.cap.items()}
        items.append((vis, cap, ds.texts[i], int(i), vid, cap_id, frames))
    items.sort(key=lambda x: n_tokens(x[2]), reverse=True)
    out = {'vis_feats': {n: np.stack([it[0][n] for it in items]) for n in ds.vis}, 'vis_frame_feat_dict': {},
           'captions': {'caption': [it[2] for it in items]}, 'idxs': [it[3] for it in items], 'vis_ids': tuple(it[4] for it in items),
           'cap_ids': tuple(it[5] for it in items), 'vis_muti_feat': None, 'captions_task2': None,
           'vis_origin_frame_tuple': (None,) * len(items)}
    for n in ds.cap:
        out['captions'][n] = np.stack([it[1][n] for it in items])
    if ds.frame:
        first = next(iter(ds.frame))
        lens = [len(it[6][first]) for it in items]
        mask = np.zeros((len(items), max(lens)), np.float32)
        for b, k in enumerate(lens):
            mask[b, :k] = 1
        out['vis_frame_feat_dict']['mask_tensor'] = mask
        for n, (_, m) in ds.frame.items():
            t = np.zeros((len(items), max(lens), m.shape[1]), np.float32)
            for b, it in enumerate(items):
                t[b, :lens[b]] = it[6][n]
            out['vis_frame_feat_dict'][n] = t
    return out


def write_dataset(ds, root, **extra):
    """The dataset on disk and the params dict of laff_amd.data.pair_provider for it (BigFile directories under `root`, the caption
    features next to the caption file under CAP_DIRS' or the feature's own name)."""
    from laff_amd.bigfile import BigFile
    from laff_amd.data import write_bigfile
    root = str(root)
    capfile = os.path.join(root, 'TextData', 'train.caption.txt')
    os.makedirs(os.path.dirname(capfile), exist_ok=True)
    with open(capfile, 'w') as f:
        f.write(ds.capfile)
    files = {}
    for kind, feats in (('vis', ds.vis), ('frame', ds.frame)):
        files[kind] = {}
        for n, (ids, m) in feats.items():
            write_bigfile(os.path.join(root, kind, n), ids, m)
            files[kind][n] = BigFile(os.path.join(root, kind, n))
    enc = {'bow_encoding': {'name': 'bow_nsw'}, 'w2v_encoding': {'name': 'no'}}
    for n, (ids, m) in ds.cap.items():
        write_bigfile(os.path.join(root, 'TextData', CAP_DIRS.get(n, n)), ids, m)
        enc[n] = {'name': n, 'dir_name': CAP_DIRS.get(n, n)}
    params = dict(vis_feat_files=files['vis'], vis_frame_feat_dicts=files['frame'] or None, max_frame=ds.max_frame, capfile=capfile,
                  capfile_task2=None, capfile_task3=None, config=types.SimpleNamespace(frame_loader=False, text_encoding=enc),
                  pin_memory=False, num_workers=0)
    params.update(extra)
    return params


# ---- the three job kinds of laff_batch_assemble
def rows_ref(src, rows):
    return src[np.asarray(rows)]


def ragged_ref(src, seg_off, segs, fmax):
    """(dst [B, fmax, w], mask [B, fmax])."""
    dst = np.zeros((len(segs), fmax, src.shape[1]), src.dtype)
    mask = np.zeros((len(segs), fmax), np.float32)
    for b, g in enumerate(segs):
        k = min(int(seg_off[g + 1] - seg_off[g]), fmax)
        dst[b, :k] = src[seg_off[g]:seg_off[g] + k]
        mask[b, :k] = 1
    return dst, mask


def csr_ref(crow, col, val, rows):
    """(crow_dst [B + 1], col_dst, val_dst)."""
    lens = [int(crow[r + 1] - crow[r]) for r in rows]
    crow_dst = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    pick = np.concatenate([np.arange(crow[r], crow[r + 1]) for r in rows]).astype(np.int64) if rows else np.zeros(0, np.int64)
    return crow_dst, col[pick], val[pick]
