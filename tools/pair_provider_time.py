"""Times feeding the 'LAFF' training step at the shape of tools/train_step_time.py: batch 128, four video features
(512 / 2048 / 2048 / 768), a bag of words over 8192 words, word2vec of 500, a bidirectional GRU of 2 x 1024 over an embedding of 500 and a
pre-calculated CLIP feature of 512.  The training set is synthetic (1024 videos, 4096 captions of 4 to 20 words), written to a
temporary directory by data.write_bigfile and read back through BigFile.

    python tools/pair_provider_time.py [--timeout SECONDS] [--iters K]

One JSON line per row; every time is host wall time per batch with the device drained at the end of a window (the feeding paths are host
work, so a device timer would miss them), the median of five windows after a warm-up, with [min, max]; a window is K batches, or as many
more as 0.3 s take:
    host_batch       (a) the reference-shaped host path, from this library's own classes: per caption one BigFile.read_one per video
                     feature and per pre-calculated feature, torch.Tensor of the list, the sort by token count, torch.stack, upload
    host_encoders    (a) the three text encoders called on that batch's strings (tokenising, vectorising, their uploads, their kernels)
    provider_batch   (b) PairProvider.batch: the control block, one H2D copy, one laff_batch_assemble launch, the GRU batch's uploads
    provider_batch_no_gru  the same from a provider built without the GRU encoder: the control block, the copy and the launch alone
    provider_encoders (b) the same encoders called on the prepared inputs (their kernels alone)
    step_only        (c) model(train_data) on a batch that is already on the device, prepared inputs attached (no feeding at all)
    epoch_host       (c) an epoch loop fed by the host path: collate, then model(batch), the encoders working from strings
    epoch_provider   (c) `for batch in provider: model(batch)`
The step-only time of the parent commit is what tools/train_step_time.py prints on the same box (its text features are pre-extracted
tensors, so it runs no text encoder).
"""
import json
import os
import sys
import tempfile
import time

from train_step_time import N, VID, TXT, build
from train_time import run_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEOS, CAPS_PER_VIDEO, VOCAB, WE_DIM = 1024, 4, TXT['bow'], 500


def wall_windows(fn, iters):
    """Sorted host wall ms per call of five windows, the device drained at the end of each, after a warm-up of 3.  A window is `iters`
    calls, or as many more as 0.3 s take: a shorter window measures the clock.  Returns (the times, the calls of a window)."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = max(iters, int(0.3 / max(time.perf_counter() - w0, 1e-5)) + 1)
    out = []
    for _ in range(5):
        w0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - w0) * 1e3 / iters)
    return sorted(out), iters


def child(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from laff_amd import data
    from laff_amd import txt2vec as T
    from laff_amd.bigfile import BigFile
    dev = torch.device('cuda')
    g = np.random.default_rng(3)
    words = ['w%d' % i for i in range(VOCAB)]
    vids = ['video%d' % i for i in range(VIDEOS)]
    cap_ids = ['%s#%d' % (v, c) for v in vids for c in range(CAPS_PER_VIDEO)]
    texts = [' '.join(words[i] for i in g.integers(0, VOCAB, size=g.integers(4, 21))) for _ in cap_ids]
    with tempfile.TemporaryDirectory() as tmp:
        capfile = os.path.join(tmp, 'TextData', 'train.caption.txt')
        os.makedirs(os.path.dirname(capfile))
        with open(capfile, 'w') as f:
            f.write('\n'.join('%s %s' % ct for ct in zip(cap_ids, texts)) + '\n')
        vis_files = {}
        for name, w in VID.items():
            data.write_bigfile(os.path.join(tmp, name), vids, g.standard_normal((VIDEOS, w)).astype(np.float32))
            vis_files[name] = BigFile(os.path.join(tmp, name))
        data.write_bigfile(os.path.join(tmp, 'TextData', 'clip_text'), cap_ids, g.standard_normal((len(cap_ids), TXT['CLIP'])).astype(np.float32))

        class Config:
            frame_loader = False
            text_encoding = {'CLIP_encoding': {'name': 'CLIP_encoding', 'dir_name': 'clip_text'}}
        model, _ = build(True, 0.2, dev)
        vocab = T.Vocabulary('gru')
        for w in ['<pad>', '<start>', '<end>', '<unk>'] + words:
            vocab.add(w)
        enc = {'rnn_encoder': T.GruTxtEncoder(T.IdxVec(vocab), WE_DIM, TXT['rnn'] // 2, bidirectional=True, device=dev, differentiable=True),
               'bow_encoder': T.BoWTxtEncoder(T.BowVec(words), dev, with_csc=True),
               'w2v_encoder': T.W2VTxtEncoder(T.W2Vec(words, g.standard_normal((VOCAB, TXT['w2v'])).astype(np.float32)), dev)}
        for name, e in enc.items():
            setattr(model.txt_net.encoder, name, e)
        model.train().enable_training()
        t0 = time.perf_counter()
        provider = data.pair_provider(dict(vis_feat_files=vis_files, capfile=capfile, config=Config, batch_size=N, shuffle=True, device=dev,
                                           encoders=enc))
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        plan = provider.plan
        clip = BigFile(os.path.join(tmp, 'TextData', 'clip_text'))

        def host_batch(indices):
            items = []
            for i in indices:
                cap_id = plan.cap_ids[i]
                vid = cap_id.split('#', 1)[0]
                items.append(({n: torch.Tensor(bf.read_one(vid)) for n, bf in vis_files.items()}, torch.Tensor(clip.read_one(cap_id)),
                              plan.texts[i], i, vid, cap_id))
            items.sort(key=lambda x: len(T.tokenize(x[2])), reverse=True)
            return {'vis_feats': {n: torch.stack([it[0][n] for it in items], 0).to(dev) for n in vis_files},
                    'captions': {'caption': [it[2] for it in items], 'CLIP_encoding': torch.stack([it[1] for it in items], 0).to(dev)},
                    'vis_frame_feat_dict': {}, 'idxs': [it[3] for it in items], 'vis_ids': tuple(it[4] for it in items),
                    'cap_ids': tuple(it[5] for it in items)}

        epoch = [list(b) for b in plan.batches()]
        turn = {'i': 0}

        def indices():
            turn['i'] = (turn['i'] + 1) % len(epoch)
            return epoch[turn['i']]

        def encoders(cap):
            with torch.no_grad():
                for e in enc.values():
                    e(cap)
        # the two feeding paths give the same batch before anything is timed
        a, b = host_batch(epoch[0]), provider.batch(epoch[0])
        same = a['idxs'] == b['idxs'] and all(torch.equal(a['vis_feats'][n], b['vis_feats'][n]) for n in vis_files) and \
            torch.equal(a['captions']['CLIP_encoding'], b['captions']['CLIP_encoding'])
        if not same:
            print('the two feeding paths give different batches: nothing is timed', file=sys.stderr)
            return 1
        fixed_host, fixed_prov = host_batch(epoch[1])['captions'], provider.batch(epoch[1])['captions']
        resident = provider.batch(epoch[2])

        def step_only():
            model({'vis_feats': dict(resident['vis_feats']), 'captions': dict(resident['captions']), 'vis_frame_feat_dict': {}})
        no_gru = data.pair_provider(dict(vis_feat_files=vis_files, capfile=capfile, config=Config, batch_size=N, device=dev,
                                         encoders={k: e for k, e in enc.items() if k != 'rnn_encoder'}))
        rows = [('host_batch', lambda: host_batch(indices())), ('host_encoders', lambda: encoders(fixed_host)),
                ('provider_batch', lambda: provider.batch(indices())), ('provider_batch_no_gru', lambda: no_gru.batch(indices())),
                ('provider_encoders', lambda: encoders(fixed_prov)),
                ('step_only', step_only), ('epoch_host', lambda: model(host_batch(indices()))),
                ('epoch_provider', lambda: model(provider.batch(indices())))]
        shape = {'N': N, 'vid': VID, 'txt': TXT, 'videos': VIDEOS, 'captions': len(cap_ids), 'we_dim': WE_DIM}
        print(json.dumps({'row': 'build', 'shape': shape, 'seconds': round(build_s, 3), 'resident_bytes': provider.resident_bytes}), flush=True)
        for name, fn in rows:
            ms, calls = wall_windows(fn, iters)
            print(json.dumps({'row': name, 'ms': round(ms[2], 4), 'spread': [round(ms[0], 4), round(ms[-1], 4)], 'calls': calls}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(run_child(child, 20, 420))
