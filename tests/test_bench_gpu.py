"""bench.py end to end on the GPU at a reduced size: the JSON line the driver parses (keys, types, the accounting identities the judge recomputes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def run(*flags):
  r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), *flags], capture_output=True, text=True, timeout=1500)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
  assert len(lines) == 1 and r.stdout.rstrip().splitlines()[-1] == lines[0], r.stdout[-2000:]     # ONE JSON line, the last one
  assert len(lines[0]) < 4096                              # compact: the driver parses it
  full = [ln for ln in r.stderr.splitlines() if ln.startswith('bench_full: ')]
  assert len(full) == 1
  return json.loads(lines[0]), json.loads(full[0][len('bench_full: '):])


REDUCED = ('--steps', '20', '--warmup', '5', '--envs', '1024', '--horizon', '40', '--episodes-per-launch', '6', '--action-sets', '2')


def test_default_line_schema_and_accounting_at_a_reduced_size(tmp_path):
  d, full = run(*REDUCED, '--full', '--cpu-seconds', '0.5', '--no-sawyer', '--no-kitchen', '--no-minitaur', '--dump-outputs', str(tmp_path / 'full'))
  for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline',
            'cpu_baseline'):
    assert k in d, k
  assert d['n_gpus'] == 1 and d['steps'] == 20 and d['warmup'] == 5 and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
  assert d['dtype'] == 'f64' and d['data'] == 'synthetic' and d['unit'] == 'env-steps/s'
  c, r = d['config'], d['roofline']
  n, T, E = 1024, 40, 6
  assert c['envs_per_gpu'] == n and c['horizon'] == T and c['episodes_per_bench_step'] == E and c['env_steps_per_bench_step'] == E * n * T and len(c['workload']) < 128
  # value = env-steps of the timed region / its wall time; ms_per_step = that time / steps
  assert abs(d['value'] - c['env_steps_per_bench_step'] * 1e3 / d['ms_per_step']) < 1e-6 * d['value']
  # roofline: 66 B per env-step + the state once per launch, all of it crossing HBM (own actions per episode); frac = achieved / peak
  assert r['bound'] == 'hbm' and r['peak'] == 8000.0 and r['unit'] == 'GB/s' and r['bytes_per_env_step'] == 66
  assert r['algorithmic_bytes_per_launch'] == n * (E * T * 66 + 2 * (32 + 1 + 4) + 4)
  assert abs(r['achieved'] - r['algorithmic_bytes_per_launch'] / (r['kernel_ms_median'] * 1e-3) / 1e9) < 1e-4 * r['achieved']
  assert abs(r['frac'] - r['achieved'] / 8000.0) < 1e-5 * r['frac'] and 0 < r['frac'] < 1
  assert r['kernel_ms_median'] <= d['ms_per_step'] * 1.05                       # the kernel time of a launch fits inside the wall time of a bench step (launches of ~15 us
                                                                               # at this size: 2 % for the event clocks' granularity)
  assert abs(r['kernel_ms_mean'] - sum(full['roofline']['windows_ms']) / r['windows']) < 1e-4 * r['kernel_ms_mean']
  s = c['strict']
  assert s['value'] > 0 and s['single_episode_launch'] > 0      # (at this size the three regimes are within timing noise of each other: no ordering asserted)
  cb = d['cpu_baseline']
  assert cb['kind'] == 'port' and cb['cores'] >= 1 and cb['value'] > 0 and cb['sample'] and cb['value'] >= max(cb['oracle_c'], cb['host_build']) * (1 - 1e-5)
  assert 'host' in full['cpu_baseline_oracle_c'] and full['step_api']['value'] > 0 and full['value'] == d['value']
  assert json.load(open(os.path.join(REPO, 'bench_full.json')))['value'] == d['value']
  # the plain line: the headline alone, one roofline window; the outputs of its last timed launch are those of the --full run's headline, bit for bit
  p, pfull = run(*REDUCED, '--dump-outputs', str(tmp_path / 'plain'))
  assert p['steps'] == 20 and p['cpu_baseline'] is None and p['roofline']['windows'] == 1 and 'step_api' not in pfull and pfull['early_window'] is None
  assert abs(p['value'] - p['config']['env_steps_per_bench_step'] * 1e3 / p['ms_per_step']) < 1e-6 * p['value']
  for name, cols in (('obs', (12,)), ('reward', ()), ('done', ()), ('success', ())):
    got = np.load(tmp_path / 'plain' / f'{name}.npy')
    assert got.dtype == np.float32 and got.shape == (E * T * n,) + cols
    np.testing.assert_array_equal(got, np.load(tmp_path / 'full' / f'{name}.npy'))
  assert np.load(tmp_path / 'plain' / 'done.npy').reshape(E, T, n)[:, -1].all()


def test_minitaur_line(tmp_path):
  d, full = run('--workload', 'minitaur', '--steps', '1', '--warmup', '0', '--no-cpu', '--dump-outputs', str(tmp_path))
  assert d['config']['envs_global'] == 4096 and d['config']['horizon'] == 1000 and full['diverged_env_steps'] <= 4 and d['value'] > 1e5
  assert d['roofline']['bound'] == 'valu' and d['scaling'] == 'strong' and d['steps'] == 1
  # a fixed sample of the [T, N] rows (all of them would exceed the dump's budget): float64 observations, same rows in every file
  obs, done = np.load(tmp_path / 'obs.npy'), np.load(tmp_path / 'done.npy')
  assert obs.dtype == np.float64 and obs.shape[1] == 32 and done.dtype == np.float32 and done.shape == obs.shape[:1] < (1000 * 4096,)
  assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) < 64e6 and np.isfinite(obs).all()
