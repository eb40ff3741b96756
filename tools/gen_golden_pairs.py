#!/usr/bin/env python3
"""tests/golden/pair_batches.npz: a tiny training set and the batches the REAL reference's pair_provider makes of it
(tools/gen_golden.py's stub recipe covers data_provider's imports).

    python tools/gen_golden_pairs.py

Reference symbols exercised (file:line relative to the reference tree): data_provider.py:834-843 pair_provider, :621-698
PairDataset, :380-498 VisionDataset (frame sets :430-446, :475-479), :501-596 TextDataset (pre-calculated features :565-574),
:92-152 collate_pair, bigfile.py:187-240 BigFile.read / read_one, textlib.py:27-45 TextTool.tokenize.

The set: 9 videos (ids with an underscore of their own) and one video no caption names, 23 captions with 1 to 5 per video, one of
them without a text; video features of width 5 / 12 / 130, each file in an order of its own; one frame feature of width 8 with 1
to 7 frames per video, written in a shuffled file order, read with max_frame = 5; one pre-calculated caption feature of width 6.
Two runs at batch size 10: one under a fixed `sampler` (three batches, the last of 3 rows, recorded whole) and one with shuffle=True
under torch.manual_seed(SEED) over two epochs (the caption order of every batch).
Arrays, ids and strings only; the files the reference reads are written to a temporary directory by laff_amd.data.write_bigfile.
"""
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (imports the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import data_provider as ref_dp  # noqa: E402
import bigfile as ref_bigfile  # noqa: E402
from laff_amd.data import write_bigfile  # noqa: E402

SEED, BATCH, MAX_FRAME = 1234, 10, 5
VIS = {'X3D_L': 5, 'mean_irCSN': 12, 'clip_ft': 130}
FRAME, FRAME_W, CAP_FEAT, CAP_W = 'Frame_clip_ft', 8, 'CLIP_encoding', 6
FRAMES_PER_VIDEO = [3, 1, 7, 5, 2, 6, 4, 1, 5]
CAPS_PER_VIDEO = [3, 1, 5, 2, 4, 2, 3, 1, 2]
TEXTS = ['a man is playing a guitar on stage', 'Two dogs run, fast!', 'someone cooks', 'A woman talks to the camera about cars',
         'kids', 'the cat sits on the mat and looks at a bird outside', 'people are dancing in a room', 'a car drives',
         'water flows down the river bank', 'He said: "no" -- twice', 'a b c d e f g h i j k l', 'one two', 'three four',
         'a person folds paper', 'rain', 'the band plays its last song tonight', 'a dog', 'birds fly over the sea at dusk',
         'it is what it is', 'x', 'two men shake hands', 'a girl sings a song', 'snow falls on the quiet town']


def main():
    g = np.random.default_rng(7)
    vids = ['vid_%s%d' % ('ab'[i % 2], i) for i in range(9)]
    cap_ids, texts = [], []
    for v, k in zip(vids, CAPS_PER_VIDEO):
        for c in range(k):
            cap_ids.append('%s#%d' % (v, c))
    assert len(cap_ids) == len(TEXTS) == 23
    texts = list(TEXTS)
    texts[13] = ''                                           # one caption without a text
    order = g.permutation(len(cap_ids))                      # captions of a video are not neighbours in the file
    cap_ids, texts = [cap_ids[i] for i in order], [texts[i] for i in order]
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        capfile = os.path.join(tmp, 'TextData', 'train.caption.txt')
        os.makedirs(os.path.dirname(capfile))
        with open(capfile, 'w') as f:
            f.write('\n'.join(('%s %s' % (c, t)).rstrip() for c, t in zip(cap_ids, texts)) + '\n')
        arrays['capfile'] = np.array(open(capfile).read())
        vis_files = {}
        for name, w in VIS.items():
            ids = [vids[i] for i in g.permutation(len(vids))] + ['vid_z99']
            ids = [ids[i] for i in g.permutation(len(ids))]
            m = g.standard_normal((len(ids), w)).astype(np.float32)
            write_bigfile(os.path.join(tmp, name), ids, m)
            vis_files[name] = ref_bigfile.BigFile(os.path.join(tmp, name))
            arrays['vis/%s/ids' % name], arrays['vis/%s/matrix' % name] = np.array(ids), m
        fids = ['%s_%d' % (v, k) for v, n in zip(vids, FRAMES_PER_VIDEO) for k in range(n)]
        fids = [fids[i] for i in g.permutation(len(fids))]
        fm = g.standard_normal((len(fids), FRAME_W)).astype(np.float32)
        write_bigfile(os.path.join(tmp, FRAME), fids, fm)
        arrays['frame/%s/ids' % FRAME], arrays['frame/%s/matrix' % FRAME] = np.array(fids), fm
        cids = [cap_ids[i] for i in g.permutation(len(cap_ids))]
        cm = g.standard_normal((len(cids), CAP_W)).astype(np.float32)
        write_bigfile(os.path.join(tmp, 'TextData', 'clip_text'), cids, cm)
        arrays['cap/%s/ids' % CAP_FEAT], arrays['cap/%s/matrix' % CAP_FEAT] = np.array(cids), cm
        config = types.SimpleNamespace(frame_loader=False, text_encoding={
            'bow_encoding': {'name': 'bow_nsw'}, 'w2v_encoding': {'name': 'no'},
            CAP_FEAT: {'name': 'CLIP_encoding', 'dir_name': 'clip_text'}})

        def params(**kw):
            return dict(vis_feat_files=vis_files, vis_frame_feat_dicts={FRAME: ref_bigfile.BigFile(os.path.join(tmp, FRAME))},
                        max_frame=MAX_FRAME, capfile=capfile, capfile_task2=None, capfile_task3=None, config=config, vis_ids=vids,
                        batch_size=BATCH, pin_memory=False, num_workers=0, **kw)
        sampler = [int(i) for i in g.permutation(len(cap_ids))]
        batches = list(ref_dp.pair_provider(params(sampler=sampler)))
        assert [len(b['idxs']) for b in batches] == [10, 10, 3]
        for k, b in enumerate(batches):
            pre = 'batch%d/' % k
            assert b['vis_muti_feat'][0] is None and b['captions_task2'][0] is None and b['vis_origin_frame_tuple'][0] is None
            for name in VIS:
                arrays[pre + 'vis_feats/' + name] = b['vis_feats'][name].numpy()
            arrays[pre + 'frames/' + FRAME] = b['vis_frame_feat_dict'][FRAME].numpy()
            arrays[pre + 'mask_tensor'] = b['vis_frame_feat_dict']['mask_tensor'].numpy()
            arrays[pre + 'caption'] = np.array(b['captions']['caption'])
            arrays[pre + CAP_FEAT] = b['captions'][CAP_FEAT].numpy()
            arrays[pre + 'idxs'] = np.array(b['idxs'], dtype=np.int64)
            arrays[pre + 'vis_ids'], arrays[pre + 'cap_ids'] = np.array(b['vis_ids']), np.array(b['cap_ids'])
        torch.manual_seed(SEED)
        loader = ref_dp.pair_provider(params(shuffle=True))
        for epoch in range(2):
            for k, b in enumerate(loader):
                arrays['shuffle/epoch%d/batch%d/idxs' % (epoch, k)] = np.array(b['idxs'], dtype=np.int64)
    arrays['sampler'], arrays['vids'] = np.array(sampler, dtype=np.int64), np.array(vids)
    arrays['meta'] = np.array([SEED, BATCH, MAX_FRAME], dtype=np.int64)
    G.save('pair_batches', **arrays)


if __name__ == '__main__':
    main()
