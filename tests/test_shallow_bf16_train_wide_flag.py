"""--torso_dtype=bf16 on a shallow agent with 5-16 channel frames, the parts
that need no GPU: the frames the wide training kernels take (the host mirror
against the binding), what the agent reports and the start-up log line."""

import logging
import types

import pytest
import torch

from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv

CASES = [((72, 96, 4), 1, False), ((72, 96, 5), 1, True), ((84, 84, 16), 8192, True),
         ((72, 128, 17), 1, False), ((16, 16, 12), 1, False),
         ((72, 96, 12), 0, False), ((72, 96, 12), 8193, False)]


@pytest.mark.parametrize('shape,n,want', CASES)
def test_wide_train_form(shape, n, want):
  from scalable_agent_amd import ops
  if 1 <= n <= 8192:  # the host predicate has no frame count
    assert conv.shallow_bf16_train_wide_form(shape) is want
  if ops.available():
    assert bool(ops.ext().shallow_bf16w_train_form(n, *shape)) is want


def test_agent_and_startup_log_line(caplog):
  from scalable_agent_amd import experiment
  agent = Agent(9, backend='hip', torso='shallow', frame_shape=(72, 96, 12),
                torso_dtype='bf16')
  assert agent.shallow_torso_bf16_train() is False
  assert agent.shallow_torso_bf16_train_wide() is True
  assert not agent.shallow_torso_bf16_train_wide(cuda=False)
  assert not Agent(9, backend='hip', frame_shape=(72, 96, 12)).shallow_torso_bf16_train_wide()
  assert not Agent(9, backend='hip', frame_shape=(72, 96, 3),
                   torso_dtype='bf16').shallow_torso_bf16_train_wide()
  flags = types.SimpleNamespace(torso_dtype='bf16')
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_learner_torso(flags, agent, torch.device('cuda'))
  lines = [r.getMessage() for r in caplog.records if 'learner torso' in r.getMessage()]
  assert len(lines) == 1
  assert lines[0].startswith('learner torso: bf16 convs, fp32 features')
  assert '72x96x12 frames, the wide kernels' in lines[0]
