"""bench.py --dump-outputs / --full on CPU: a plain one-rank run writes the
last timed step's loss and updated parameters as float32 .npy files, two runs
with the same arguments write the same arrays, and the extra measurements
appear only with --full."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
  cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
         '--steps', '3', '--warmup', '1', '--device', 'cpu',
         '--batch_size', '2', '--unroll_length', '4', '--torso', 'shallow',
         '--height', '24', '--width', '32'] + list(extra)
  env = {k: v for k, v in os.environ.items()
         if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
  env.update(PYTHONPATH=ROOT, OMP_NUM_THREADS='2')
  r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
  assert r.returncode == 0, r.stderr[-3000:]
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert len(lines) == 1, r.stdout
  return json.loads(lines[0])


def test_dump_outputs_is_reproducible(tmp_path):
  outs = []
  for name in ('a', 'b'):
    d = tmp_path / name
    rec = _run('--dump-outputs', str(d))
    assert rec['steps'] == 3 and rec['ms_per_step'] > 0
    assert sorted(os.listdir(d)) == ['loss.npy', 'params.npy']
    outs.append({n: np.load(d / (n + '.npy')) for n in ('loss', 'params')})
  a, b = outs
  assert a['loss'].dtype == np.float32 and a['loss'].shape == (1,)
  assert a['params'].dtype == np.float32 and a['params'].ndim == 1
  assert a['params'].size > 1000 and np.isfinite(a['params']).all()
  assert a['params'].nbytes + a['loss'].nbytes <= 64 << 20
  for n in a:
    assert np.array_equal(a[n], b[n]), n


def test_plain_run_has_headline_fields_only():
  rec = _run()
  for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype',
            'ms_per_step'):
    assert k in rec, k
  assert 'bf16' not in rec['config'] and rec['config']['h2d_slab'] is None
