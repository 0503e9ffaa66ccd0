"""The bf16 deep torso takes uint8 frames of 3 to 16 channels (host side)."""

import types

import pytest
import torch

from scalable_agent_amd.experiment import frame_shape_for
from scalable_agent_amd.flags import parse_flags
from scalable_agent_amd.models import Agent
from scalable_agent_amd.models.agent import hip_ops_in_use
from scalable_agent_amd.ops import conv


@pytest.mark.parametrize('c,ok', [(1, False), (2, False), (3, True), (4, True),
                                  (5, True), (16, True), (17, False)])
def test_supports_deep(c, ok):
  agent = types.SimpleNamespace(torso_kind='deep', frame_shape=(72, 96, c))
  assert conv.supports(agent) is ok


@pytest.mark.parametrize('c', [3, 4, 12])
def test_supports_shallow_stays_false(c):
  agent = types.SimpleNamespace(torso_kind='shallow', frame_shape=(72, 96, c))
  assert conv.supports(agent) is False


def test_wide_bf16_agent_lists_bf16_torso():
  flags = parse_flags(['--obs_shape=72x96x12', '--dtype=bf16', '--torso=deep'])
  shape = frame_shape_for(flags, 'synthetic')
  assert shape == (72, 96, 12)
  agent = Agent(9, torso='deep', frame_shape=shape, backend='hip',
                compute_dtype=torch.bfloat16)
  assert 'conv_torso_bf16' in hip_ops_in_use(agent)
