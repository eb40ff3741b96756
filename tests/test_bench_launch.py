"""bench.py --gpus N without a launcher environment starts N ranks itself (torch.distributed.run as a child process) and relays
rank 0's single JSON line.  Run here on CPU through LAFF_BENCH_DRYRUN=1: gloo instead of RCCL, the oracle-backed stand-in
kernels of tests/dist_util.py on a toy problem -- the launch, rendezvous, collective and reporting path of an N > 1 run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, *extra):
    env = dict(os.environ, LAFF_BENCH_DRYRUN='1')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(n), '--steps', '2', '--warmup', '1'] + list(extra),
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout                     # ONE line on stdout, whatever the ranks printed elsewhere
    return json.loads(lines[0])


def test_self_launch_two_ranks_dryrun():
    line = _run(2)
    assert line['n_gpus'] == 2 and line['rccl_ranks'] == 2
    assert line['steps'] == 2 and line['warmup'] == 1 and line['scaling'] == 'strong'
    assert line['config']['shard'] == 'video'              # the decomposition BASELINE.json names is the headline
    assert line['alt_shard']['shard'] == 'text' and line['alt_shard']['ranks_equal']
    assert [a['shard'] for a in line['alt_shards']] == ['text', 'video16'] and all(a['ranks_equal'] for a in line['alt_shards'])
    b16, b32 = line['alt_shards'][1]['gathered_bytes_per_step'], line['gathered_bytes_per_step']
    assert b16['all_gather_text_16bit'] * 2 == b32['all_gather_text_fp32'] and b16['all_to_all_pairs'] > 0
    assert line['value'] > 0 and line['ms_per_step'] > 0


def test_self_launch_two_ranks_shard_auto_and_video_agree_dryrun():
    """`--shard auto` and `--shard video` through the self-launch (a child torch.distributed.run, never an exec): the default IS
    'video' (BASELINE.json's decomposition), 'auto' picks by the smaller side, every line names its scheme, reports the other two
    beside it with their gathered bytes, and all of them end with the same ranks and the same seven metrics."""
    from laff_amd.dist import choose_sharding
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from dist_util import problem
    xt, xv = problem()[:2]
    dflt, vid, auto = _run(2), _run(2, '--shard', 'video'), _run(2, '--shard', 'auto')
    assert dflt['config']['shard'] == 'video' and vid['config']['shard'] == 'video'
    assert auto['config']['shard'] == choose_sharding(len(xt), len(xv)) and auto['config']['shard_arg'] == 'auto'
    for line in (vid, auto):
        assert line['rccl_ranks'] == 2 and line['n_gpus'] == 2
        names = [line['config']['shard']] + [a['shard'] for a in line['alt_shards']]
        assert sorted(names) == ['text', 'video', 'video16']
        assert all(a['ranks_equal'] for a in line['alt_shards'])
        assert all(sum(a['gathered_bytes_per_step'].values()) > 0 for a in line['alt_shards'])
        assert sum(line['gathered_bytes_per_step'].values()) > 0
    assert vid['quality'] == auto['quality']
    # 'video' gathers the fp32 text rows, 'text' the fp32 video rows: the bytes follow the sides
    gv = vid['gathered_bytes_per_step']
    gt_ = (auto if auto['config']['shard'] == 'text' else vid)
    tb = gt_['gathered_bytes_per_step'] if gt_['config']['shard'] == 'text' else [a for a in vid['alt_shards'] if a['shard'] == 'text'][0]['gathered_bytes_per_step']
    assert gv['all_gather_text_fp32'] * len(xv) == tb['all_gather_video_fp32'] * len(xt)


def test_single_rank_needs_no_launcher_dryrun():
    line = _run(1)
    assert line['n_gpus'] == 1 and line['rccl_ranks'] == 1


def test_more_gpus_than_the_node_has_is_refused():
    """Without the dry-run switch the parent counts the visible GPUs before starting anything (0 in this container)."""
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip('this node has the GPUs')
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'LAFF_BENCH_DRYRUN')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and 'visible GPU' in out.stderr and out.stdout.strip() == ''


def test_dump_outputs_dryrun(tmp_path):
    """--dump-outputs DIR writes the result of the last timed step (float32 / float64 .npy), the same from run to run and -- for the
    replicated ranks and metrics -- the same on one rank and on two."""
    import numpy as np
    runs = []
    for name, n in (('a', 1), ('b', 1), ('c', 2)):
        line = _run(n, '--dump-outputs', str(tmp_path / name))
        runs.append((line, {f[:-4]: np.load(str(tmp_path / name / f)) for f in os.listdir(tmp_path / name)}))
    (line, a), (_, b), (_, c) = runs
    assert sorted(a) == ['S_local', 'metrics', 'ranks', 'txt_emb', 'vis_emb'] and sorted(b) == sorted(a) == sorted(c)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    q = line['quality']
    assert a['metrics'].tolist() == [q[k] for k in ('R@1', 'R@5', 'R@10', 'MedR', 'meanr', 'mir', 'mAP')]
    assert np.array_equal(a['ranks'], c['ranks']) and np.array_equal(a['metrics'], c['metrics'])
    assert c['S_local'].shape[1] < a['S_local'].shape[1]          # rank 0's video shard


def test_dump_outputs_samples_rows_within_the_budget(tmp_path):
    """An output larger than its share of the budget keeps a seeded sample of its rows (indices beside it); the rest goes whole."""
    import numpy as np
    import torch
    import bench
    g = np.random.default_rng(3)
    arrays = {'S': torch.from_numpy(g.normal(size=(1000, 64)).astype(np.float32)), 'E': g.normal(size=(10, 8)),
              'r': torch.arange(1, 101, dtype=torch.int32), 'm': (1.5, 2.0)}
    budget = 100000
    for d in ('x', 'y'):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    files = sorted(os.listdir(tmp_path / 'x'))
    assert files == ['E.npy', 'S.npy', 'S_rows.npy', 'm.npy', 'r.npy'] and sorted(os.listdir(tmp_path / 'y')) == files
    got = {f[:-4]: np.load(str(tmp_path / 'x' / f)) for f in files}
    assert sum(os.path.getsize(str(tmp_path / 'x' / f)) for f in files) <= budget
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(str(tmp_path / 'y' / f)))
    rows = got['S_rows'].astype(np.int64)
    assert got['S_rows'].dtype == np.float64 and len(rows) > 100 and np.all(np.diff(rows) > 0)
    assert got['S'].dtype == np.float32 and np.array_equal(got['S'], arrays['S'].numpy()[rows])
    assert got['E'].dtype == np.float64 and np.array_equal(got['E'], arrays['E'])
    assert got['r'].dtype == np.float64 and np.array_equal(got['r'], np.arange(1, 101))
    assert got['m'].dtype == np.float64 and got['m'].tolist() == [1.5, 2.0]


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], env=dict(os.environ, LAFF_BENCH_DRYRUN='1'),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and '--steps' in out.stderr and out.stdout.strip() == ''
