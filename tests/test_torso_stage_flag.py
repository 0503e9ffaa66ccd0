"""--torso_blocks=stage / Agent(torso_blocks='stage') without a GPU: the value
parses, an unknown one still raises, and where the fp32 HIP deep torso does
not run (shallow torso, torch backend) the torso runs as with 'ops' and the
start-up log line says so."""

import logging

import pytest
import torch

from scalable_agent_amd import experiment
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent


def test_stage_parses_and_the_default_stays_ops():
  assert flags_lib.parse_flags(['--torso_blocks=stage']).torso_blocks == 'stage'
  assert flags_lib.parse_flags(['--torso_blocks=fused']).torso_blocks == 'fused'
  assert flags_lib.parse_flags([]).torso_blocks == 'ops'
  assert flags_lib.default_flags().torso_blocks == 'ops'
  assert Agent(9, torso_blocks='stage').torso_blocks == 'stage'


def test_unknown_value_still_raises():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--torso_blocks=bogus'])
  with pytest.raises(ValueError):
    Agent(9, torso_blocks='bogus')


@pytest.mark.parametrize('kw', [
    dict(torso='shallow', backend='hip'),
    dict(torso='shallow', backend='torch'),
    dict(torso='deep', backend='torch', frame_shape=(24, 32, 3)),
])
def test_stage_is_not_honoured_off_the_fp32_hip_deep_torso(kw):
  ag = Agent(9, seed=3, torso_blocks='stage', **kw)
  assert not ag.torso_blocks_fused()
  assert not ag.torso_blocks_fused(cuda=False)
  assert ag.torso_stage_form() is None
  assert ag.torso_stage_form(cuda=False) is None


def test_stage_on_the_torch_backend_equals_ops():
  shape = (24, 32, 3)
  mk = lambda blocks: Agent(9, torso='deep', frame_shape=shape, seed=3,
                            backend='torch', torso_blocks=blocks)
  g = torch.Generator().manual_seed(7)
  frames = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
  with torch.no_grad():
    a, b = mk('stage').conv_features(frames), mk('ops').conv_features(frames)
  assert torch.equal(a, b)


def test_start_up_log_line_says_where_stage_cannot_apply(caplog):
  flags = flags_lib.parse_flags(['--torso_blocks=stage'])
  model = inference.InferenceModel(
      Agent(9, torso='shallow', seed=3, torso_blocks='stage'), 'cpu')
  assert model.torso_blocks == 'ops'
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_blocks(flags, model)
  lines = [r.getMessage() for r in caplog.records
           if 'torso blocks' in r.getMessage()]
  assert len(lines) == 1
  assert lines[0].startswith('actor inference torso blocks: ops (')
  assert '--torso_blocks=stage does not apply' in lines[0]
