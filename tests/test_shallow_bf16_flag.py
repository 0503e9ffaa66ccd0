"""--inference_dtype=bf16 on the shallow torso, the parts that need no GPU:
what the agent reports, the frames the bf16 kernel takes, the start-up log
line, and the exactness of the kernel's x / 255 epilogue."""

import logging
import types

import numpy as np
import pytest
import torch

from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv

FRAMES = [(72, 96, 3), (84, 84, 4), (72, 128, 3), (72, 96, 1)]


def test_cpu_agents_report_torch_and_run_as_before():
  g = torch.Generator().manual_seed(0)
  frames = torch.randint(0, 256, (3, 72, 96, 3), generator=g,
                         dtype=torch.uint8)
  fresh = Agent(9, torso='shallow', seed=2, compute_dtype=torch.bfloat16)
  for backend in ('hip', 'torch'):
    ag = Agent(9, torso='shallow', seed=2, backend=backend,
               compute_dtype=torch.bfloat16)
    assert ag.inference_torso_precision(cuda=False) == 'torch'
    if backend == 'torch':
      assert ag.inference_torso_precision(cuda=True) == 'torch'
    with torch.no_grad():
      a, b = ag.conv_features(frames), fresh.conv_features(frames)
    assert a.dtype == torch.bfloat16 and torch.equal(a, b)
  from scalable_agent_amd.inference import InferenceModel
  model = InferenceModel(Agent(9, torso='shallow', seed=2,
                               compute_dtype=torch.bfloat16), 'cpu', False)
  assert model.torso_precision == 'torch'
  assert (model.agent._inference_cache or {}).get('wsh16') is None


def test_precision_of_hip_agents():
  mk = lambda dt, **kw: Agent(9, backend='hip', compute_dtype=dt, **kw)
  bf, fp = torch.bfloat16, torch.float32
  assert mk(bf, torso='shallow').inference_torso_precision() == 'bf16'
  assert mk(fp, torso='shallow').inference_torso_precision() == 'fp32'
  assert mk(bf, torso='shallow',
            frame_shape=(16, 16, 3)).inference_torso_precision() == 'fp32'
  assert mk(bf, torso='deep').inference_torso_precision() == 'bf16'
  assert mk(fp, torso='deep').inference_torso_precision() == 'fp32'
  # the learner's view is unchanged: no bf16 shallow learner
  from scalable_agent_amd.models.agent import torso_precision
  assert torso_precision(mk(bf, torso='shallow')) == 'fp32'
  assert not conv.supports(mk(bf, torso='shallow'))


def test_form():
  from scalable_agent_amd import ops
  ext = ops.ext() if ops.available() else None
  cases = [(s, n, True) for s in FRAMES for n in (1, 512)]
  cases += [((72, 96, 3), 513, False), ((72, 96, 3), 0, False),
            ((16, 16, 3), 1, False), ((72, 96, 5), 1, False)]
  for shape, n, want in cases:
    assert conv.shallow_bf16_form(shape, n) == want, (shape, n)
    if ext is not None:
      assert bool(ext.shallow_bf16_form(n, *shape)) == want, (shape, n)


@pytest.mark.parametrize('shape,used', [((72, 96, 3), 'bf16'),
                                        ((16, 16, 3), 'fp32')])
def test_startup_log_line(caplog, shape, used):
  from scalable_agent_amd import experiment
  agent = Agent(9, torso='shallow', frame_shape=shape, backend='hip',
                compute_dtype=torch.bfloat16)
  model = types.SimpleNamespace(
      agent=agent, torso_precision=agent.inference_torso_precision(cuda=True))
  assert model.torso_precision == used
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_precision(model)
  lines = [r.getMessage() for r in caplog.records
           if 'actor inference torso precision' in r.getMessage()]
  assert len(lines) == 1
  assert lines[0].startswith('actor inference torso precision: ' + used)
  if used == 'fp32':
    assert 'bf16 inference asked for' in lines[0] and '16x16x3' in lines[0]
  else:
    assert 'one bf16 MFMA launch' in lines[0]


def test_epilogue_scaling_is_exact_on_multiples_of_255():
  """The kernel stages bytes as exact bf16 integers and applies 1 / 255 to the
  fp32 accumulator as a correctly rounded fp32 division, then adds the bias
  in fp32: for acc = 255 k (a frame of bytes 0 / 255 under integer weights)
  that is exactly k + bias.  A multiply by fl(1 / 255) is NOT exact (the
  constant rounds upward by more than half an ulp of some k), which is why
  the kernel divides."""
  k = np.arange(-256, 257, dtype=np.float32)
  acc = np.float32(255.0) * k
  assert np.array_equal(acc.astype(np.float64), 255.0 * k.astype(np.float64))
  for bias in range(0, 9):
    got = acc / np.float32(255.0) + np.float32(bias)
    assert got.dtype == np.float32
    assert np.array_equal(got, k + np.float32(bias)), bias
  s = np.float32(1.0) / np.float32(255.0)
  assert float(s) > 1.0 / 255.0
  assert not np.array_equal(acc * s, k)
