"""bench.py --gpus 2 without a launcher and without a GPU: the script starts its two ranks itself, they meet over gloo
(BENCH_SHARE_GPU), each takes its work-balanced slab, the timing is reduced and rank 0 prints ONE valid JSON line.  The
device patch is replaced by tests/_bench_stub.py -- this test is about the launcher, not about arithmetic."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def _run(args, extra_env=None, timeout=300):
    env = dict(os.environ, BENCH_PATCH_STUB=os.path.join(ROOT, 'tests', '_bench_stub.py'), BENCH_SHARE_GPU='1',
               BENCH_LAUNCH_TIMEOUT='120')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_self_launch_two_ranks_prints_one_valid_line():
    r = _run(['--gpus', '2', '--steps', '3', '--warmup', '1', '--config', 'tiny', '--no-cpu-baseline'])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1 and r.stdout.rstrip().splitlines()[-1] == lines[0]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['steps'] == 3 and d['warmup'] == 1 and d['scaling'] == 'strong' and d['unit'] == 'elements/s'
    assert d['value'] > 0 and d['ms_per_step'] > 0 and d['higher_is_better'] is True
    assert len(d['slab_ms']) == 2 and len(d['setup_s_ranks']) == 2 and len(d['cold_ms_ranks']) == 2
    assert d['config']['elements'] == 12 ** 3 and 'roofline' in d
    # the slabs tile the patch: nnz of the two ranks add up to the whole pattern
    N, p = 14, 2
    S = sum(min(i + p, N - 1) + 1 - max(i - p, 0) for i in range(N))
    assert d['config']['nnz'] == S ** 3


def test_single_rank_line_and_failed_rank_is_reported():
    r = _run(['--steps', '2', '--warmup', '0', '--config', 'tiny', '--no-cpu-baseline', '--no-api-call'])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.rstrip().splitlines()[-1])
    assert d['n_gpus'] == 1 and d['slab_ms'] and d['setup_s_ranks'] and d['api_call_s'] is None
    # a rank that dies takes the run down quickly (no hang in the rendezvous) and the parent says which one
    bad = _run(['--gpus', '2', '--steps', '1', '--config', 'tiny', '--no-cpu-baseline'],
               extra_env={'BENCH_PATCH_STUB': os.path.join(ROOT, 'tests', 'does_not_exist.py')}, timeout=120)
    assert bad.returncode != 0 and 'rank' in (bad.stderr + bad.stdout)


def test_self_launch_eight_ranks():
    """world size 8 (what the driver launches for the scaling curve): eight ranks meet, eight slabs tile the patch."""
    r = _run(['--gpus', '8', '--steps', '2', '--warmup', '1', '--config', 'tiny', '--no-cpu-baseline'], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 8 and len(d['slab_ms']) == 8 and len(d['setup_s_ranks']) == 8
    N, p = 14, 2
    S = sum(min(i + p, N - 1) + 1 - max(i - p, 0) for i in range(N))
    assert d['config']['nnz'] == S ** 3 and 'scaling_model' in d


def test_dump_outputs_are_reproducible(tmp_path):
    """--dump-outputs DIR: the CSR of the last timed step as float64 .npy files (at most 64 MB), the same for the same arguments;
    --steps sets the number of timed steps and the line carries ms_per_step."""
    import numpy as np
    files = {}
    for run in ('a', 'b'):
        d = tmp_path / run
        r = _run(['--steps', '3', '--warmup', '1', '--config', 'tiny', '--no-cpu-baseline', '--no-api-call', '--dump-outputs', str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.rstrip().splitlines()[-1])
        assert line['steps'] == 3 and line['ms_per_step'] > 0
        assert line['dump_outputs']['entries'] == line['config']['nnz'] and not line['dump_outputs']['sampled']
        files[run] = {p.name: np.load(p) for p in sorted(d.iterdir())}
    assert sorted(files['a']) == ['csr_cols.npy', 'csr_rows.npy', 'csr_values.npy']
    assert sum(a.nbytes for a in files['a'].values()) <= 64 << 20
    for name, a in files['a'].items():
        assert a.dtype == np.float64 and a.shape == (262144,)
        assert np.array_equal(a, files['b'][name])
    assert _run(['--steps', '0', '--config', 'tiny', '--no-cpu-baseline']).returncode != 0


def test_dump_outputs_of_two_ranks(tmp_path):
    r = _run(['--gpus', '2', '--steps', '2', '--warmup', '0', '--config', 'tiny', '--no-cpu-baseline', '--dump-outputs', str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted('rank%d_csr_%s.npy' % (k, a) for k in range(2) for a in ('cols', 'rows', 'values'))


def test_dump_outputs_sample_of_a_large_matrix(tmp_path):
    """A matrix above the entry budget is written as a fixed seeded sample of whole runs of consecutive entries."""
    import numpy as np
    import bench

    class Patch:
        nnz = 50 * bench.DUMP_RUN + 123
    indptr = np.arange(0, Patch.nnz + 1, 7, dtype=np.int32)
    indptr[-1] = Patch.nnz
    calls = []

    def read(which, k, n):
        calls.append((which, k, n))
        assert 0 <= k and k + n <= Patch.nnz
        pos = np.arange(k, k + n)
        return pos * 0.5 if which == 'values' else (pos % 11).astype(np.int32)
    out = [bench.dump_outputs(str(tmp_path / s), Patch(), (100, indptr, read), max_entries=8 * bench.DUMP_RUN) for s in 'ab']
    assert out[0]['sampled'] and out[0]['entries'] == 8 * bench.DUMP_RUN and out[0]['nnz'] == Patch.nnz
    v, rows, cols = (np.load(tmp_path / 'a' / ('csr_%s.npy' % n)) for n in ('values', 'rows', 'cols'))
    pos = (v * 2).astype(np.int64)
    assert np.array_equal(rows, 100 + np.searchsorted(indptr, pos, side='right') - 1) and np.array_equal(cols, pos % 11)
    assert np.all(pos % bench.DUMP_RUN == np.tile(np.arange(bench.DUMP_RUN), 8))
    for n in ('values', 'rows', 'cols'):
        assert np.array_equal(np.load(tmp_path / 'a' / ('csr_%s.npy' % n)), np.load(tmp_path / 'b' / ('csr_%s.npy' % n)))
