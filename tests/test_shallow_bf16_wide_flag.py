"""--inference_dtype=bf16 on a shallow agent with 5-16 channel frames, the
parts that need no GPU: the frames the wide kernel takes (the host mirror
against the binding), what the agent reports and the start-up log line."""

import logging
import types

import torch

from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv

FRAMES = [(72, 96), (84, 84), (72, 128)]
CASES = [(hw + (c,), n, True) for hw in FRAMES for c in (5, 16)
         for n in (1, 512)]
CASES += [((72, 96, 4), 1, False), ((72, 96, 17), 1, False),
          ((72, 96, 12), 0, False), ((72, 96, 12), 513, False),
          ((16, 16, 12), 1, False)]


def _mk(shape):
  return Agent(9, backend='hip', torso='shallow', frame_shape=shape,
               compute_dtype=torch.bfloat16)


def test_wide_form():
  from scalable_agent_amd import ops
  ext = ops.ext() if ops.available() else None
  for shape, n, want in CASES:
    assert conv.shallow_bf16_wide_form(shape, n) == want, (shape, n)
    if ext is not None:
      assert bool(ext.shallow_bf16w_form(n, *shape)) == want, (shape, n)


def test_precision_and_startup_log_line(caplog):
  from scalable_agent_amd import experiment
  from scalable_agent_amd.models.agent import torso_precision
  agent = _mk((72, 96, 12))
  assert agent.inference_torso_precision() == 'bf16'
  assert _mk((16, 16, 12)).inference_torso_precision() == 'fp32'
  assert torso_precision(agent) == 'fp32'  # no bf16 shallow learner
  assert not conv.supports(agent)
  model = types.SimpleNamespace(
      agent=agent, torso_precision=agent.inference_torso_precision(cuda=True))
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_precision(model)
  lines = [r.getMessage() for r in caplog.records
           if 'actor inference torso precision' in r.getMessage()]
  assert len(lines) == 1
  assert lines[0].startswith('actor inference torso precision: bf16')
  assert 'one bf16 MFMA launch on 72x96x12 frames' in lines[0]
