"""CPU: ``bench.py --dump-outputs DIR`` writes the last timed step's SDF arrays as float .npy files within its byte budget;
above it, a fixed seeded sample (the same for every run) together with the indices it kept."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('p2s_bench', os.path.join(REPO, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_within_budget_writes_the_arrays_unchanged(tmp_path):
    bench = _bench()
    a = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    b = np.arange(7, dtype=np.float64)
    files = bench.dump_outputs(str(tmp_path), [a, b])
    assert files == {'sdf_0.npy': [1000], 'sdf_1.npy': [7]}
    got = np.load(tmp_path / 'sdf_0.npy')
    assert got.dtype == np.float32 and np.array_equal(got, a)
    assert np.array_equal(np.load(tmp_path / 'sdf_1.npy'), b)
    assert sorted(os.listdir(tmp_path)) == ['sdf_0.npy', 'sdf_1.npy']


def test_dump_above_budget_is_a_fixed_sample_with_its_indices(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, 'DUMP_BYTES', 12000)
    a = np.random.default_rng(1).standard_normal(5000).astype(np.float32)
    b = np.random.default_rng(2).standard_normal(3000).astype(np.float32)
    d1, d2 = tmp_path / 'one', tmp_path / 'two'
    assert bench.dump_outputs(str(d1), [a, b]) == bench.dump_outputs(str(d2), [a, b])
    total = 0
    for k, src in enumerate((a, b)):
        idx = np.load(d1 / ('sdf_%d_index.npy' % k))
        val = np.load(d1 / ('sdf_%d.npy' % k))
        assert idx.dtype == np.float64 and val.dtype == np.float32 and 0 < idx.shape[0] == val.shape[0] < src.shape[0]
        assert np.all(np.diff(idx) > 0) and np.array_equal(val, src[idx.astype(np.int64)])
        assert np.array_equal(idx, np.load(d2 / ('sdf_%d_index.npy' % k)))          # the same sample every run
        total += idx.nbytes + val.nbytes
    assert total <= 12000


def test_dump_needs_a_timed_step():
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0', '--dump-outputs', 'unused'], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'at least one timed step' in r.stderr
