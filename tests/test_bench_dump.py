"""bench.py --dump-outputs DIR: after the timed steps, what the timed path computed in its last step as float64
DIR/<name>.npy (at most 64 MB in all), the same from run to run with the same arguments; --steps K times K steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_flag():
    assert bench.parse_args([]).dump_outputs is None
    assert bench.parse_args(['--dump-outputs', 'out']).dump_outputs == 'out'


def test_dump_outputs_as_float64_within_the_limit(tmp_path, monkeypatch):
    bench.dump_outputs(str(tmp_path / 'd'), {'a': np.arange(6, dtype=np.float32).reshape(2, 3), 'b': [1, 2]})
    a, b = np.load(tmp_path / 'd' / 'a.npy'), np.load(tmp_path / 'd' / 'b.npy')
    assert a.dtype == b.dtype == np.float64
    assert np.array_equal(a, np.arange(6.).reshape(2, 3)) and np.array_equal(b, [1., 2.])
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 40)
    with pytest.raises(SystemExit, match='limit'):
        bench.dump_outputs(str(tmp_path / 'e'), {'a': np.zeros(6)})      # 48 bytes: refused, nothing written
    assert not (tmp_path / 'e').exists()


def _bench(args, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT')}
    env['LCF_BENCH_NO_E2E'] = '1'
    res = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--no-cpu-baseline', '--dump-outputs', str(out_dir)]
                         + args, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    line = json.loads(res.stdout)
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_mcmc_dump_is_the_last_step_and_repeats(tmp_path):
    line, got = _bench(['--steps', '7', '--warmup', '3'], tmp_path / 'a')
    assert line['steps'] == 7 and line['timed_region']['steps_per_repetition'] == 7 and line['ms_per_step'] > 0
    assert line['chain']['shape'] == [7, 1024, 5]                 # the stored chain: exactly the timed steps
    assert sorted(got) == ['acceptance_fraction', 'coords', 'log_prob']
    assert got['coords'].shape == (1024, 5) and got['log_prob'].shape == (1024,) and got['acceptance_fraction'].shape == (1024,)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    assert np.all((got['acceptance_fraction'] >= 0) & (got['acceptance_fraction'] <= 1))
    _, again = _bench(['--steps', '7', '--warmup', '3'], tmp_path / 'b')
    for name, a in got.items():
        assert np.array_equal(again[name], a), name


@pytest.mark.gpu
@pytest.mark.parametrize('workload, shapes', [
    ('companion', {'coords': (4096, 8), 'log_prob': (4096,), 'acceptance_fraction': (4096,)}),
    ('population', {'coords': (32, 512, 5), 'log_prob': (32, 512), 'acceptance_fraction': (32, 512)}),
    ('sed', {'log_likelihood_f64': (10000, 128), 'log_likelihood_f64_tables': (10000, 128),
             'log_likelihood_f32': (10000, 128)})])
def test_other_workloads_dump_their_outputs(tmp_path, workload, shapes):
    line, got = _bench(['--workload', workload, '--steps', '3', '--warmup', '2'], tmp_path)
    assert line['ms_per_step'] > 0
    assert {k: a.shape for k, a in got.items()} == shapes
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_MAX_BYTES
