"""Wide frames (5..16 channels) on the HIP backend: what the shape checks and
the flag parser say, without a GPU."""

import types

import pytest

from scalable_agent_amd.flags import parse_flags
from scalable_agent_amd.experiment import frame_shape_for
from scalable_agent_amd.models import Agent
from scalable_agent_amd.models.agent import hip_ops_in_use
from scalable_agent_amd.ops import conv_f32


@pytest.mark.parametrize('torso', ['deep', 'shallow'])
@pytest.mark.parametrize('c,ok', [(0, False), (5, True), (16, True), (17, False)])
def test_supports_wide(torso, c, ok):
  agent = types.SimpleNamespace(torso_kind=torso, frame_shape=(72, 96, c))
  assert conv_f32.supports(agent) is ok


def test_obs_shape_flag_builds_hip_agent():
  flags = parse_flags(['--obs_shape=72x96x12'])
  shape = frame_shape_for(flags, 'synthetic')
  assert shape == (72, 96, 12)
  agent = Agent(9, torso='deep', frame_shape=shape, backend='hip')
  assert 'conv_torso_fp32' in hip_ops_in_use(agent)
