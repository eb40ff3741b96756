"""laff_batch_assemble and the training pair provider on the MI355X.  Everything here is a copy, so every
comparison is torch.equal / array_equal: the kernel against tests/pair_ref.py, the provider against the fixture of the reference's
pair_provider (tests/golden/pair_batches.npz), the encoders' prepared inputs against their own from-strings path, and training steps
fed by the provider against the same steps fed by host-collated dicts."""
import numpy as np
import pytest
import torch

import pair_ref
import tower_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
WIDTHS = (1, 3, 5, 130, 512)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _control(*parts):
    """(device control, host control, offsets of the parts)."""
    at, off = [], 0
    for p in parts:
        at.append(off)
        off += len(p)
    host = np.concatenate([np.asarray(p, np.int32) for p in parts]).astype(np.int32)
    return _dev(host), host, at


def _rows_for(B, n, g):
    rows = g.integers(0, n, size=B)
    rows[0] = n - 1                                             # the last source row
    if B > 1:
        rows[-1] = rows[0]                                      # a source row twice in the batch
    return rows


@pytest.mark.parametrize('B', [1, 3, 65])
def test_rows_jobs_against_the_restatement(B):
    """Every width as a dense matrix (16-byte accesses where the width allows them, with the scalar tail), as a window of a wider
    matrix that starts one element in (4-byte but not 16-byte aligned: the scalar path), as a 16-byte aligned window of a wider matrix
    (pitch > width) and as int32; destinations dense and as windows.  All in one launch: 4 x 5 jobs take two calls of at most 16."""
    from laff_amd import ops
    g = np.random.default_rng(B)
    n = 37
    rows = _rows_for(B, n, g)
    control, host, (at,) = _control(rows)
    jobs, checks = [], []
    for w in WIDTHS:
        pitch = (w + 12 + 3) // 4 * 4                            # a multiple of 4: the aligned window keeps 16-byte rows
        wide = g.standard_normal((n, pitch)).astype(np.float32)
        wide_d = _dev(wide)
        for c0, d0 in ((None, None), (1, 2), (4, 8)):
            if c0 is None:
                src, src_np, frame, dst = _dev(wide[:, :w]), wide[:, :w], None, torch.empty(B, w, device=DEV)
            else:
                src, src_np, frame = wide_d[:, c0:c0 + w], wide[:, c0:c0 + w], torch.full((B, pitch), -3.0, device=DEV)
                dst = frame[:, d0:d0 + w]
            jobs.append(('rows', src, at, dst))
            checks.append((dst, pair_ref.rows_ref(src_np, rows), frame))
        ints = g.integers(-2 ** 31, 2 ** 31 - 1, size=(n, w)).astype(np.int32)
        dst = torch.empty(B, w, dtype=torch.int32, device=DEV)
        jobs.append(('rows', _dev(ints), at, dst))
        checks.append((dst, pair_ref.rows_ref(ints, rows), None))
    for s in range(0, len(jobs), 16):
        ops.batch_assemble(jobs[s:s + 16], control, host, B)
    torch.cuda.synchronize()
    for dst, want, frame in checks:
        assert torch.equal(dst.cpu(), torch.from_numpy(want)), (B, tuple(dst.shape))
        if frame is not None:                                   # nothing outside the window was written
            outside = torch.ones_like(frame, dtype=torch.bool)
            c0 = (dst.data_ptr() - frame.data_ptr()) // 4
            outside[:, c0:c0 + dst.shape[1]] = False
            assert bool((frame[outside] == -3.0).all())


@pytest.mark.parametrize('B', [1, 3, 65])
def test_ragged_jobs_against_the_restatement(B):
    """Segments of 1, exactly Fmax and more than Fmax rows (cut, as the provider's max_frame cut leaves none); widths that take the
    16-byte path (8, 512), the scalar path (5, and 8 read out of a window one element in) and a pitch above the width; the mask from the
    first job only."""
    from laff_amd import ops
    g = np.random.default_rng(10 + B)
    lens = np.array([1, 7, 9, 3, 7, 12, 2], np.int64)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    segs = g.integers(0, len(lens), size=B)
    segs[0] = 1
    if B > 1:
        segs[1], segs[-1] = 0, 5
    fmax = 7
    control, host, (at,) = _control(segs)
    jobs, checks = [], []
    mask = torch.full((B, fmax), -1.0, device=DEV)
    for k, w in enumerate((8, 5, 512, 8)):
        wide = g.standard_normal((int(seg_off[-1]), w + 8)).astype(np.float32)
        c0 = (0, 0, 4, 1)[k]
        src = _dev(wide)[:, c0:c0 + w] if k >= 2 else _dev(wide[:, :w])
        dst = torch.full((B, fmax, w), 9.0, device=DEV)
        jobs.append(('ragged', src, _dev(seg_off), at, dst, mask if k == 0 else None))
        checks.append((dst, pair_ref.ragged_ref(wide[:, c0:c0 + w], seg_off, segs, fmax)))
    ops.batch_assemble(jobs, control, host, B)
    torch.cuda.synchronize()
    for dst, (want, want_mask) in checks:
        assert torch.equal(dst.cpu(), torch.from_numpy(want))
        assert torch.equal(mask.cpu(), torch.from_numpy(want_mask))
    assert set(mask.sum(1).cpu().tolist()) <= {1.0, 3.0, 7.0, 2.0}
    # a padded row is never read from the source: the last segment's padding would lie behind the matrix
    last = np.array([len(lens) - 1] * B)
    control, host, (at,) = _control(last)
    src = g.standard_normal((int(seg_off[-1]), 8)).astype(np.float32)
    dst = torch.empty(B, 4, 8, device=DEV)
    ops.batch_assemble([('ragged', _dev(src), _dev(seg_off), at, dst, None)], control, host, B)
    assert torch.equal(dst.cpu(), torch.from_numpy(pair_ref.ragged_ref(src, seg_off, last, 4)[0]))


@pytest.mark.parametrize('B', [1, 3, 65])
def test_csr_jobs_against_the_restatement(B):
    from laff_amd import ops
    g = np.random.default_rng(20 + B)
    lens = np.array([3, 0, 70, 1, 0, 5], np.int64)              # empty rows, and one longer than a wave
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = g.integers(0, 1000, size=int(crow[-1])).astype(np.int32)
    val = g.standard_normal(int(crow[-1])).astype(np.float32)
    rows = _rows_for(B, len(lens), g).tolist()
    if B > 1:
        rows[1] = 1
    rows[-1] = 2 if B > 1 else 5
    empty = [1] * B                                             # and a batch without a single entry: nnz == 0
    crow_dst, want_col, want_val = pair_ref.csr_ref(crow, col, val, rows)
    crow_e, _, _ = pair_ref.csr_ref(crow, col, val, empty)
    control, host, (at, cat, eat, ecat) = _control(rows, crow_dst, empty, crow_e)
    src = (_dev(crow), _dev(col), _dev(val))
    col_d, val_d = torch.full((len(want_col),), -1, dtype=torch.int32, device=DEV), torch.full((len(want_val),), -1.0, device=DEV)
    col_e, val_e = torch.empty(0, dtype=torch.int32, device=DEV), torch.empty(0, device=DEV)
    ops.batch_assemble([('csr', src, at, cat, (col_d, val_d)), ('csr', src, eat, ecat, (col_e, val_e))], control, host, B)
    torch.cuda.synchronize()
    assert int(crow_e[-1]) == 0 and torch.equal(col_d.cpu(), torch.from_numpy(want_col)) and torch.equal(val_d.cpu(), torch.from_numpy(want_val))
    x = torch.sparse_csr_tensor(control[cat:cat + B + 1], col_d, val_d, size=(B, 1000))
    assert x.shape == (B, 1000) and int(x.crow_indices()[-1]) == len(want_col)


def test_sixteen_jobs_in_one_call_and_the_same_bits_twice():
    from laff_amd import ops
    g = np.random.default_rng(3)
    B, n = 65, 50
    rows = _rows_for(B, n, g)
    lens = g.integers(1, 9, size=n)
    seg_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    crow = np.concatenate([[0], np.cumsum(g.integers(0, 6, size=n))]).astype(np.int32)
    col, val = g.integers(0, 99, size=int(crow[-1])).astype(np.int32), g.standard_normal(int(crow[-1])).astype(np.float32)
    crow_dst, want_col, want_val = pair_ref.csr_ref(crow, col, val, rows.tolist())
    control, host, (at, cat) = _control(rows, crow_dst)
    fmax = int(lens[rows].max())
    srcs = [g.standard_normal((n, w)).astype(np.float32) for w in (1, 3, 5, 130, 512, 4, 8, 12, 16, 20, 24, 28, 6)]
    fsrcs = [g.standard_normal((int(seg_off[-1]), w)).astype(np.float32) for w in (8, 5)]

    def run():
        outs = [torch.empty(B, s.shape[1], device=DEV) for s in srcs]
        fouts = [torch.empty(B, fmax, s.shape[1], device=DEV) for s in fsrcs]
        mask, c, v = torch.empty(B, fmax, device=DEV), torch.empty(len(want_col), dtype=torch.int32, device=DEV), torch.empty(len(want_val), device=DEV)
        jobs = [('rows', _dev(s), at, o) for s, o in zip(srcs, outs)]
        jobs += [('ragged', _dev(s), _dev(seg_off), at, o, mask if i == 0 else None) for i, (s, o) in enumerate(zip(fsrcs, fouts))]
        jobs.append(('csr', (_dev(crow), _dev(col), _dev(val)), at, cat, (c, v)))
        assert len(jobs) == 16
        ops.batch_assemble(jobs, control, host, B)
        with pytest.raises(ValueError, match='1 to 16 jobs'):
            ops.batch_assemble(jobs + jobs[:1], control, host, B)
        return outs + fouts + [mask, c, v]
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for s, o in zip(srcs, a):
        assert torch.equal(o.cpu(), torch.from_numpy(s[rows]))
    for s, o in zip(fsrcs, a[len(srcs):]):
        want, want_mask = pair_ref.ragged_ref(s, seg_off, rows, fmax)
        assert torch.equal(o.cpu(), torch.from_numpy(want)) and torch.equal(a[-3].cpu(), torch.from_numpy(want_mask))
    assert torch.equal(a[-2].cpu(), torch.from_numpy(want_col)) and torch.equal(a[-1].cpu(), torch.from_numpy(want_val))
    with pytest.raises(RuntimeError, match=r'row\[0\] = 49 is outside \[0, 4\)'):          # the host copy of the control block is checked
        ops.batch_assemble([('rows', _dev(srcs[0][:4]), at, a[0])], control, host, B)


def _same_batch(got, want):
    """A provider batch (device tensors) against a collate_pair-shaped dict of numpy arrays."""
    assert set(got) == {'vis_feats', 'vis_muti_feat', 'vis_frame_feat_dict', 'vis_origin_frame_tuple', 'captions', 'captions_task2', 'idxs',
                        'vis_ids', 'cap_ids'}
    assert got['idxs'] == want['idxs'] and got['vis_ids'] == tuple(want['vis_ids']) and got['cap_ids'] == tuple(want['cap_ids'])
    assert got['vis_muti_feat'] is None and got['captions_task2'] is None and got['vis_origin_frame_tuple'] == (None,) * len(got['idxs'])
    assert got['captions']['caption'] == want['captions']['caption']
    for side in ('vis_feats', 'vis_frame_feat_dict'):
        assert set(got[side]) == set(want[side])
        for k, v in want[side].items():
            assert got[side][k].is_cuda and torch.equal(got[side][k].cpu(), torch.from_numpy(v)), (side, k)
    for k, v in want['captions'].items():
        if k != 'caption':
            assert torch.equal(got['captions'][k].cpu(), torch.from_numpy(v)), k


def test_provider_reproduces_the_reference_batches(tmp_path):
    from laff_amd import data
    arrays, ds = pair_ref.fixture()
    sampler = [int(i) for i in arrays['sampler']]
    provider = data.pair_provider(pair_ref.write_dataset(ds, tmp_path, batch_size=10, sampler=sampler, device=DEV))
    assert len(provider) == 3 and provider.batch_size == 10 and len(provider.dataset) == 23
    assert provider.resident_bytes == sum(provider.plan.feature_bytes().values())
    first = list(provider)
    torch.cuda.synchronize()
    for k, got in enumerate(first):
        pre = 'batch%d/' % k
        want = {'idxs': arrays[pre + 'idxs'].tolist(), 'vis_ids': arrays[pre + 'vis_ids'].tolist(), 'cap_ids': arrays[pre + 'cap_ids'].tolist(),
                'captions': {'caption': [str(s) for s in arrays[pre + 'caption']], 'CLIP_encoding': arrays[pre + 'CLIP_encoding']},
                'vis_feats': {n: arrays[pre + 'vis_feats/' + n] for n in ds.vis},
                'vis_frame_feat_dict': {'mask_tensor': arrays[pre + 'mask_tensor'], 'Frame_clip_ft': arrays[pre + 'frames/Frame_clip_ft']}}
        _same_batch(got, want)
        assert torch.equal(got['vis_frame_feat_dict']['mask_tensor'].sum(1).cpu(), torch.from_numpy((arrays[pre + 'mask_tensor'] > 0).sum(1)).float())
    # every step gets fresh dicts and tensors: writing into one epoch's batches leaves the next epoch's alone
    for b in first:
        for t in list(b['vis_feats'].values()) + [b['vis_frame_feat_dict']['Frame_clip_ft'], b['captions']['CLIP_encoding']]:
            t.fill_(float('nan'))
    again = list(provider)
    assert all(g['vis_feats']['X3D_L'].data_ptr() != f['vis_feats']['X3D_L'].data_ptr() for g, f in zip(again, first))
    _same_batch(again[2], pair_ref.collate(ds, sampler[20:]))
    # without frame features the frame dict is empty; shuffle draws a new permutation at every iter()
    params = pair_ref.write_dataset(pair_ref.Dataset(ds.capfile, ds.vis, {}, ds.cap, ds.max_frame), tmp_path / 'noframes', batch_size=7,
                                    shuffle=True, device=DEV)
    provider = data.pair_provider(params)
    torch.manual_seed(5)
    e1, e2 = [b['idxs'] for b in provider], [b['idxs'] for b in provider]
    assert e1 != e2 and sorted(i for b in e1 for i in b) == list(range(23)) and [len(b) for b in e1] == [7, 7, 7, 2]
    assert next(iter(provider))['vis_frame_feat_dict'] == {}


WORDS = ['man', 'guitar', 'dogs', 'run', 'fast', 'woman', 'camera', 'cars', 'cat', 'mat', 'bird', 'people', 'room', 'car', 'water', 'river',
         'a', 'the', 'is', 'on', 'song', 'sings', 'snow', 'town', 'two', 'it', 'what', 'x', 'rain', 'dog']


def _encoders(differentiable):
    from laff_amd import txt2vec as T
    vocab = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + WORDS:
        vocab.add(w)
    g = np.random.default_rng(2)
    w2v = T.W2Vec(WORDS[:24], g.standard_normal((24, 20)).astype(np.float32), stopwords={'a', 'the'})
    torch.manual_seed(4)
    return {'bow_encoder': T.BoWTxtEncoder(T.BowVec(WORDS, stopwords={'is', 'on'}), DEV, with_csc=differentiable),
            'w2v_encoder': T.W2VTxtEncoder(w2v, DEV),
            'rnn_encoder': T.GruTxtEncoder(T.IdxVec(vocab), 12, 32, bidirectional=True, device=DEV, differentiable=differentiable),
            'NetVLAD_encoder': T.NetVLADTxtEncoder(w2v, num_clusters=4, device=DEV, differentiable=differentiable)}


@pytest.mark.parametrize('differentiable', [False, True])
def test_prepared_inputs_give_the_bits_of_the_strings(tmp_path, differentiable):
    """Each of the four encoders on every batch of the fixture set (an empty caption and captions without a known word among them):
    the prepared input and the strings give the same output bits; in differentiable training mode the same parameter gradients too."""
    from laff_amd import data
    from laff_amd import txt2vec as T
    arrays, ds = pair_ref.fixture()
    enc = _encoders(differentiable)
    for e in enc.values():
        e.train(differentiable)
    provider = data.pair_provider(pair_ref.write_dataset(ds, tmp_path, batch_size=10, sampler=[int(i) for i in arrays['sampler']],
                                                         device=DEV, encoders=enc))
    for batch in provider:
        cap = batch['captions']
        assert set(cap[T.PREPARED_KEY]) == set(enc.values())
        strings = {'caption': cap['caption']}
        for name, e in enc.items():
            outs, grads = [], []
            for d in (cap, strings):
                e.zero_grad(set_to_none=True)
                y = e(d)['text_features']
                if y.layout == torch.sparse_csr:
                    outs.append((y.crow_indices(), y.col_indices(), y.values()) + tuple(getattr(y, 'laff_csc', ())))
                    assert y.crow_indices().dtype == y.col_indices().dtype == torch.int32 and (hasattr(y, 'laff_csc') == differentiable)
                    continue
                outs.append((y.detach(),))
                if differentiable and y.requires_grad:
                    y.backward(torch.linspace(-1, 1, y.numel(), device=DEV).reshape(y.shape))
                    grads.append([p.grad.clone() for p in e.parameters()])
            assert len(outs[0]) == len(outs[1]) and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(*outs)), name
            if differentiable and name in ('rnn_encoder', 'NetVLAD_encoder'):
                assert len(grads) == 2 and grads[0] and all(torch.equal(a, b) for a, b in zip(*grads)), name
    torch.cuda.synchronize()


def _training_set(meta, n_caps, g, frame_lens=None, real_text=False):
    """A synthetic pair_ref.Dataset with the shapes of a training-step fixture case: its video (and frame) features, and its text
    features as pre-calculated caption features -- the bag of words and word2vec left to real encoders with real_text."""
    B = meta['N']
    vids = ['v%d' % i for i in range(B)]
    cap_ids = ['%s#%d' % (vids[i % B], i // B) for i in range(n_caps)]
    texts = [' '.join(g.choice(WORDS, size=g.integers(1, 9)).tolist()) for _ in range(n_caps)]
    order = g.permutation(B)
    vis = {n: ([vids[i] for i in order], g.standard_normal((B, w)).astype(np.float32)) for n, w in meta['vid_dims'].items()}
    frame = {}
    if frame_lens is not None:
        fids = [('%s_%d' % (v, k)) for v, n in zip(vids, frame_lens) for k in range(n)]
        fids = [fids[i] for i in g.permutation(len(fids))]
        frame = {n: (fids, g.standard_normal((len(fids), d)).astype(np.float32)) for n, d in meta['frame_feats'].items()}
    keys = {'bow': 'bow_encoding', 'w2v': 'w2v_encoding', 'CLIP': 'CLIP_encoding'}
    cap = {keys[k]: (cap_ids, g.standard_normal((n_caps, w)).astype(np.float32)) for k, w in meta['txt_dims'].items()
           if not (real_text and k in ('bow', 'w2v'))}
    capfile = '\n'.join('%s %s' % (c, t) for c, t in zip(cap_ids, texts)) + '\n'
    return pair_ref.Dataset(capfile, vis, frame, cap, meta.get('max_frame', 200))


def _to_device(batch):
    out = dict(batch)
    for side in ('vis_feats', 'vis_frame_feat_dict'):
        out[side] = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in batch[side].items()}
    out['captions'] = {k: v if k == 'caption' else torch.from_numpy(v.copy()).to(DEV) for k, v in batch['captions'].items()}
    return out


def _two_steps_fed_both_ways(key, tmp_path, real_text, frame_lens=None):
    from laff_amd import data
    from laff_amd import txt2vec as T
    _, meta = tower_ref.load_case(key)
    assert meta['dropout'] == 0
    B = meta['N']
    ds = _training_set(meta, 2 * B, np.random.default_rng(31), frame_lens, real_text)
    sampler = [int(i) for i in np.random.default_rng(8).permutation(2 * B)]

    def model():
        m = tower_ref.device_model(key, DEV)
        enc = {}
        if real_text:
            w2v = T.W2Vec(WORDS[:25], np.random.default_rng(6).standard_normal((25, meta['txt_dims']['w2v'])).astype(np.float32))
            enc = {'bow_encoder': T.BoWTxtEncoder(T.BowVec(WORDS), DEV, with_csc=True), 'w2v_encoder': T.W2VTxtEncoder(w2v, DEV)}
            assert len(WORDS) == meta['txt_dims']['bow']
            for name, e in enc.items():
                setattr(m.txt_net.encoder, name, e)
        return m.train().enable_training(), enc
    fed, enc = model()
    provider = data.pair_provider(pair_ref.write_dataset(ds, tmp_path, batch_size=B, sampler=sampler, device=DEV, encoders=enc))
    host, _ = model()
    losses = []
    for step, batch in enumerate(provider):
        assert (T.PREPARED_KEY in batch['captions']) == real_text
        a = fed(batch)
        b = host(_to_device(pair_ref.collate(ds, sampler[step * B:(step + 1) * B])))
        torch.cuda.synchronize()
        la, lb = a['triplet_loss'].detach(), b['triplet_loss'].detach()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
        losses.append(float(la))
        for (k, p), q in zip(fed.named_parameters(), host.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), (step, k)
            assert torch.equal(p.detach(), q.detach()), (step, k)
    assert step == 1 and fed.iters == host.iters == 2 and losses[0] != losses[1]
    for (k, p), q in zip(fed.state_dict().items(), host.state_dict().values()):
        assert torch.equal(p, q), k
    if real_text:
        assert fed.txt_net.transform_layer.bow_encoder_transform.fc1.weight.grad.abs().max() > 0


def test_two_laff_steps_fed_by_the_provider_and_by_host_collated_dicts(tmp_path):
    """Case 'a' of the training-step fixture ('LAFF'; video 128 + 40, bag of words 30, word2vec 20, CLIP 128; D 512, H 4, N 12, dropout 0),
    the bag of words and word2vec through the real encoders: prepared inputs on the provider's side, strings on the other."""
    _two_steps_fed_both_ways('a', tmp_path, real_text=True)


def test_two_framelaff_steps_fed_by_the_provider_and_by_host_collated_dicts(tmp_path):
    """Case 'e' ('FrameLAFF': video 40 + 24, the frame feature of 512 with 1 to 13 frames, N 10)."""
    _two_steps_fed_both_ways('e', tmp_path, real_text=False, frame_lens=[13, 1, 7, 4, 13, 2, 9, 5, 1, 11])
