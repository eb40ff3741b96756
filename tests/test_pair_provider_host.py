"""The training pair provider without a GPU: the numpy restatement of the reference's collate_pair against the
fixture of its real pair_provider (tests/golden/pair_batches.npz), the provider's host planning against the same fixture, the epoch
order against torch's DataLoader, and every refusal of data.PairPlan / PairProvider, ops.batch_assemble and laff_batch_assemble."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import pair_ref
from conftest import ROOT


def _fixture_batches():
    arrays, ds = pair_ref.fixture()
    sampler, bs = [int(i) for i in arrays['sampler']], int(arrays['meta'][1])
    return arrays, ds, [sampler[s:s + bs] for s in range(0, len(sampler), bs)]


def test_fixture_is_what_the_issue_asks_for():
    arrays, ds, batches = _fixture_batches()
    assert len(ds.cap_ids) == 23 and len(arrays['vids']) == 9 and [len(b) for b in batches] == [10, 10, 3]
    assert sorted(m.shape[1] for _, m in ds.vis.values()) == [5, 12, 130] and '' in ds.texts
    ids, m = ds.frame['Frame_clip_ft']
    per_video = [sum(f.rsplit('_', 1)[0] == v for f in ids) for v in arrays['vids']]
    assert m.shape[1] == 8 and min(per_video) == 1 and max(per_video) == 7 and ds.max_frame == 5
    v = str(arrays['vids'][2])                                  # the file order is not the frame-number order
    nums = [int(f.rsplit('_', 1)[1]) for f in ids if f.rsplit('_', 1)[0] == v]
    assert nums != sorted(nums)


def test_collate_restatement_reproduces_the_reference_batches():
    arrays, ds, batches = _fixture_batches()
    for k, indices in enumerate(batches):
        got, pre = pair_ref.collate(ds, indices), 'batch%d/' % k
        assert got['idxs'] == arrays[pre + 'idxs'].tolist()
        assert list(got['vis_ids']) == arrays[pre + 'vis_ids'].tolist() and list(got['cap_ids']) == arrays[pre + 'cap_ids'].tolist()
        assert got['captions']['caption'] == [str(s) for s in arrays[pre + 'caption']]
        assert np.array_equal(got['captions']['CLIP_encoding'], arrays[pre + 'CLIP_encoding'])
        for name in ds.vis:
            assert np.array_equal(got['vis_feats'][name], arrays[pre + 'vis_feats/' + name])
        assert np.array_equal(got['vis_frame_feat_dict']['mask_tensor'], arrays[pre + 'mask_tensor'])
        assert np.array_equal(got['vis_frame_feat_dict']['Frame_clip_ft'], arrays[pre + 'frames/Frame_clip_ft'])
        assert arrays[pre + 'mask_tensor'].shape[1] <= ds.max_frame


def test_plan_gives_the_fixture_rows(tmp_path):
    from laff_amd import data
    arrays, ds, batches = _fixture_batches()
    plan = data.PairPlan(pair_ref.write_dataset(ds, tmp_path, batch_size=10, sampler=[i for b in batches for i in b]))
    assert plan.cap_ids == ds.cap_ids and plan.texts == ds.texts and len(plan) == 23
    assert plan.ntok.tolist() == [pair_ref.n_tokens(t) for t in ds.texts]
    assert [list(b) for b in plan.batches()] == batches
    # frames: video-major, each video's rows in file order, cut to max_frame by frame number
    ids, _ = ds.frame['Frame_clip_ft']
    want = [pair_ref.frame_rows(ids, v, ds.max_frame) for v in plan.vis_ids]
    assert plan.frame_rows['Frame_clip_ft'].tolist() == [r for rows in want for r in rows]
    assert plan.seg_off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want])]).tolist()
    control = np.full(plan.control_ints, -7, np.int32)
    for k, indices in enumerate(batches):
        lay, pre = plan.fill(indices, control), 'batch%d/' % k
        B = len(indices)
        assert lay.B == B and lay.rows.tolist() == arrays[pre + 'idxs'].tolist() == control[lay.cap_at:lay.cap_at + B].tolist()
        vid_rows = control[lay.vid_at:lay.vid_at + B]
        assert [plan.vis_ids[v] for v in vid_rows] == arrays[pre + 'vis_ids'].tolist()
        assert lay.fmax == control[lay.fmax_at] == arrays[pre + 'mask_tensor'].shape[1]
        assert lay.total == 3 * B + 2 <= plan.control_ints and not control[lay.crow_at:lay.crow_at + B + 1].any()


def test_shuffle_order_is_the_dataloaders(tmp_path):
    from torch.utils.data import DataLoader
    from laff_amd import data
    arrays, ds, _ = _fixture_batches()
    plan = data.PairPlan(pair_ref.write_dataset(ds, tmp_path, batch_size=10, shuffle=True))
    torch.manual_seed(int(arrays['meta'][0]))
    own = [[list(b) for b in plan.batches()] for _ in range(2)]
    torch.manual_seed(int(arrays['meta'][0]))
    loader = DataLoader(range(len(plan)), batch_size=10, shuffle=True, collate_fn=list)
    theirs = [[b for b in loader] for _ in range(2)]
    assert own == theirs and own[0] != own[1] and sorted(i for b in own[0] for i in b) == list(range(23))
    for e in range(2):                                       # and the reference's own run under that seed
        for k, b in enumerate(own[e]):
            assert plan.order(b).tolist() == arrays['shuffle/epoch%d/batch%d/idxs' % (e, k)].tolist()


def test_batch_row_order_is_stable_longest_first(tmp_path):
    from laff_amd import data
    _, ds, _ = _fixture_batches()
    plan = data.PairPlan(pair_ref.write_dataset(ds, tmp_path))
    idx = list(range(23))[::-1]
    want = sorted(idx, key=lambda i: pair_ref.n_tokens(ds.texts[i]), reverse=True)
    assert plan.order(idx).tolist() == want and len(set(plan.ntok.tolist())) < 23          # ties are there to be kept in order
    with pytest.raises(IndexError, match='outside'):
        plan.order([0, 23])


def test_build_refusals(tmp_path):
    from laff_amd import data
    _, ds, _ = _fixture_batches()
    params = pair_ref.write_dataset(ds, tmp_path)
    with pytest.raises(RuntimeError, match='no CPU path'):
        data.pair_provider(dict(params, device='cpu'))
    with pytest.raises(NotImplementedError, match='frame_loader'):
        data.PairPlan(dict(params, config=types.SimpleNamespace(frame_loader=True, text_encoding={})))
    for key, word in (('capfile_task3', 'task-3 negation'), ('capfile_task2', 'capfile_task2'), ('vis_muti_feat_dicts', 'vis_muti_feat_dicts')):
        with pytest.raises(NotImplementedError, match=word):
            data.PairPlan(dict(params, **{key: 'x'}))
    with pytest.raises(ValueError, match='batch_size=5000'):
        data.PairPlan(dict(params, batch_size=5000))
    with pytest.raises(ValueError, match='mutually exclusive'):
        data.PairPlan(dict(params, shuffle=True, sampler=[0]))
    with pytest.raises(TypeError, match="encoders\\['x'\\] is a Linear"):
        data.PairPlan(dict(params, encoders={'x': torch.nn.Linear(1, 1)}))
    # a caption whose video a feature file lacks: KeyError at build, naming the id
    ids, m = ds.vis['X3D_L']
    gone = ds.cap_ids[4].split('#', 1)[0]
    keep = [i for i, v in enumerate(ids) if v != gone]
    short = pair_ref.Dataset(ds.capfile, dict(ds.vis, X3D_L=([ids[i] for i in keep], m[keep])), ds.frame, ds.cap, ds.max_frame)
    with pytest.raises(KeyError, match=gone):
        data.PairPlan(pair_ref.write_dataset(short, tmp_path / 'short'))
    cids, cm = ds.cap['CLIP_encoding']
    short = pair_ref.Dataset(ds.capfile, ds.vis, ds.frame, {'CLIP_encoding': (cids[1:], cm[1:])}, ds.max_frame)
    with pytest.raises(KeyError, match=re.escape(cids[0])):
        data.PairPlan(pair_ref.write_dataset(short, tmp_path / 'nocap'))
    # a second frame feature with other per-video counts
    fids, fm = ds.frame['Frame_clip_ft']
    drop = next(i for i, f in enumerate(fids) if 2 <= sum(g.rsplit('_', 1)[0] == f.rsplit('_', 1)[0] for g in fids) <= ds.max_frame)
    keep = [i for i in range(len(fids)) if i != drop]
    two = pair_ref.Dataset(ds.capfile, ds.vis, dict(ds.frame, other=([fids[i] for i in keep], fm[keep])), ds.cap, ds.max_frame)
    with pytest.raises(ValueError, match="frame feature 'other' has . frames for video"):
        data.PairPlan(pair_ref.write_dataset(two, tmp_path / 'two'))


def test_resident_limit_is_checked_before_anything_is_allocated(tmp_path):
    from laff_amd import data
    _, ds, _ = _fixture_batches()
    params = pair_ref.write_dataset(ds, tmp_path)
    plan = data.PairPlan(params)
    sizes = plan.feature_bytes()
    assert sizes['vis_feat_files[clip_ft]'] == 4 * 9 * 130 and sizes['captions[CLIP_encoding]'] == 4 * 23 * 6
    assert sizes['vis_frame_feat_dicts[Frame_clip_ft]'] == 4 * 8 * int(plan.seg_off[-1])
    with pytest.raises(MemoryError, match=r'vis_feat_files\[clip_ft\] 4680'):          # (raised without a GPU: nothing was allocated)
        data.pair_provider(dict(params, max_resident_bytes=sum(sizes.values()) - 1))


def test_stored_ids_give_the_batches_of_the_strings():
    from laff_amd import txt2vec as T
    words = ['w%d' % i for i in range(12)]
    vocab = T.Vocabulary('gru')
    for w in ['<pad>', '<start>', '<end>', '<unk>'] + words:
        vocab.add(w)
    caps = ['w1 w2 w3', '', 'w4 nope w4', 'w5', 'w1 w9 w2 w7']
    idx = T.IdxVec(vocab)
    a, b = idx.batch(caps), T.IdxVec.batch_ids([idx.encoding(c) for c in caps])
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a.batch_sizes == b.batch_sizes
    w2v = T.W2Vec(words, np.zeros((12, 4), np.float32))
    stored = [(np.asarray(r, np.int32), n) for r, n in map(w2v.raw_ids, caps + ['nope nope'])]
    for x, y in zip(w2v.ragged(caps + ['nope nope']), T.W2Vec.ragged_rows(stored)):
        assert np.array_equal(x, y) and x.dtype == y.dtype
    assert T.prepared_input({'caption': caps}, idx) is None and T.prepared_input({T.PREPARED_KEY: {idx: 5}}, idx) == 5


def test_wrapper_refusals():
    from laff_amd import ops
    z = torch.zeros(4, 8)
    with pytest.raises(ValueError, match='1 to 16 jobs'):
        ops.batch_assemble([], z, None, 4)
    with pytest.raises(ValueError, match='1 to 4096 batch rows'):
        ops.batch_assemble([('rows', z, 0, z)], z, None, 4097)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.batch_assemble([('rows', z, 0, z)], torch.zeros(4, dtype=torch.int32), np.zeros(4, np.int32), 4)


def _job(lib_mod, **kw):
    q = lib_mod.AssembleJob()
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_abi_refusals_come_before_the_ctx():
    """Every refusal of laff_batch_assemble with a NULL ctx: the shapes and the control block are judged first, the ctx last (no
    pointer is followed on the way: the device pointers here are host addresses that are never read)."""
    from laff_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'laff_hip.h')).read()
    assert 'LAFF_ASSEMBLE_MAX_JOBS %d' % _lib.ASSEMBLE_MAX_JOBS in header and 'LAFF_ASSEMBLE_MAX_BATCH %d' % _lib.ASSEMBLE_MAX_BATCH in header
    buf = np.zeros(64, np.float32)
    ctl = np.array([0, 1, 2, 0, 0, 2, 2, 5], np.int32)         # rows 0 1 2 | - | crow_dst 0 2 2 5
    p, cp = buf.ctypes.data, ctl.ctypes.data_as(C.c_void_p)
    rows = dict(kind=0, rows_at=0, w=5, ld_src=8, ld_dst=5, n_src=3, src=p, dst=p)

    def call(jobs, B=3, count=None, control=cp, host=cp, n=8):
        arr = (_lib.AssembleJob * max(1, len(jobs)))(*jobs)
        rc = lib.laff_batch_assemble(None, arr, len(jobs) if count is None else count, B, control, host, n)
        return rc, lib.laff_last_error().decode()

    assert call([_job(_lib, **rows)]) == (-1, 'laff_batch_assemble: null ctx')                 # nothing else to object to
    for count in (0, 17):
        rc, msg = call([_job(_lib, **rows)], count=count)
        assert rc == -2 and '%d jobs' % count in msg
    for B in (0, 4097):
        rc, msg = call([_job(_lib, **rows)], B=B)
        assert rc == -2 and 'B=%d' % B in msg
    assert call([_job(_lib, **rows)], host=None)[0] == -1
    for bad, word in ((dict(kind=3), 'bad kind 3'), (dict(w=0), 'bad shape w=0'), (dict(ld_src=4), 'ld_src=4'), (dict(ld_dst=4), 'ld_dst=4'),
                      (dict(src=None), 'null src'), (dict(src=p + 2), '4-byte aligned'), (dict(n_src=2), 'row[2] = 2 is outside [0, 2)'),
                      (dict(rows_at=6), 'lie outside the control block'), (dict(rows_at=-1), 'lie outside the control block'),
                      (dict(ld_dst=1 << 20), 'overflows 32-bit indexing (B * ld_dst)')):
        B = 4096 if 'ld_dst' in bad and bad['ld_dst'] > 4 else 3
        host = np.zeros(4096, np.int32) if B == 4096 else ctl
        rc, msg = call([_job(_lib, **dict(rows, **bad))], B=B, host=host.ctypes.data_as(C.c_void_p), n=host.size)
        assert rc < 0 and word in msg, (bad, msg)
    ragged = dict(kind=1, rows_at=0, w=4, ld_src=4, n_src=3, n_items=9, fmax=3, src=p, dst=p, off_src=p)
    assert call([_job(_lib, **ragged)])[1].endswith('null ctx')
    for bad, word in ((dict(fmax=0), 'fmax=0'), (dict(off_src=None), 'null seg_off'), (dict(n_src=1), 'seg[1] = 1 is outside [0, 1)')):
        rc, msg = call([_job(_lib, **dict(ragged, **bad))])
        assert rc < 0 and word in msg, (bad, msg)
    host = np.zeros(4096, np.int32)
    rc, msg = call([_job(_lib, **dict(ragged, fmax=1024, w=512, ld_src=512))], B=4096, host=host.ctypes.data_as(C.c_void_p), n=4096)
    assert rc == -2 and 'overflows 32-bit indexing (B * fmax * w)' in msg
    csr = dict(kind=2, rows_at=0, crow_at=4, n_src=3, n_items=9, cap_dst=5, src=p, dst=p, off_src=p, col_src=p, col_dst=p)
    assert call([_job(_lib, **csr)])[1].endswith('null ctx')
    for bad, word in ((dict(cap_dst=4), 'crow_dst[B] = 5 entries, col_dst / val_dst hold 4'), (dict(crow_at=5), 'lies outside the control block'),
                      (dict(crow_at=2), 'crow_dst decreases'), (dict(col_dst=None), 'null crow_src / col_src / col_dst'),
                      (dict(n_src=0), 'bad CSR sizes')):
        rc, msg = call([_job(_lib, **dict(csr, **bad))])
        assert rc < 0 and word in msg, (bad, msg)
    # the job a refusal names is the one at fault
    rc, msg = call([_job(_lib, **rows), _job(_lib, **dict(rows, w=0))])
    assert rc == -2 and 'job 1' in msg
