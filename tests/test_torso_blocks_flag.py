"""--torso_blocks / Agent(torso_blocks=...) without a GPU: the flag parses,
'fused' on the torch backend runs the torso unchanged, and the start-up log
line names the form in use."""

import logging

import pytest
import torch

from scalable_agent_amd import experiment
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent


def test_torso_blocks_flag_parses_and_defaults_to_ops():
  assert flags_lib.parse_flags([]).torso_blocks == 'ops'
  assert flags_lib.parse_flags(['--torso_blocks=fused']).torso_blocks == 'fused'
  assert flags_lib.parse_flags(['--torso_blocks', 'ops']).torso_blocks == 'ops'
  assert flags_lib.default_flags().torso_blocks == 'ops'


def test_torso_blocks_flag_rejects_unknown_value():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--torso_blocks=banded'])
  with pytest.raises(ValueError):
    Agent(9, torso_blocks='banded')


@pytest.mark.parametrize('torso,shape', [('deep', (24, 32, 3)),
                                         ('shallow', (72, 96, 3))])
def test_fused_on_the_torch_backend_equals_ops(torso, shape):
  mk = lambda blocks: Agent(9, torso=torso, frame_shape=shape, seed=3,
                            backend='torch', torso_blocks=blocks)
  fused, ops = mk('fused'), mk('ops')
  assert fused.torso_blocks == 'fused' and ops.torso_blocks == 'ops'
  assert not fused.torso_blocks_fused(cuda=False)
  g = torch.Generator().manual_seed(7)
  frames = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
  with torch.no_grad():
    a, b = fused.conv_features(frames), ops.conv_features(frames)
  assert torch.equal(a, b)


def _log_line(caplog, asked, agent):
  flags = flags_lib.parse_flags(['--torso_blocks=' + asked])
  model = inference.InferenceModel(agent, 'cpu')
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_blocks(flags, model)
  lines = [r.getMessage() for r in caplog.records
           if 'torso blocks' in r.getMessage()]
  assert len(lines) == 1
  return model, lines[0]


def test_start_up_log_line_names_the_form_in_use(caplog):
  model, line = _log_line(caplog, 'ops', Agent(9, torso='deep', seed=3))
  assert model.torso_blocks == 'ops'
  assert line == 'actor inference torso blocks: ops'


def test_start_up_log_line_says_where_the_flag_cannot_apply(caplog):
  model, line = _log_line(
      caplog, 'fused', Agent(9, torso='shallow', seed=3, torso_blocks='fused'))
  assert model.torso_blocks == 'ops'
  assert line.startswith('actor inference torso blocks: ops (')
  assert '--torso_blocks=fused does not apply' in line
