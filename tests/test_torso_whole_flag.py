"""--torso_blocks=whole / Agent(torso_blocks='whole') without a GPU: the value
parses, an unknown one still raises, the default stays 'ops', the torch
backend runs as with 'ops' (shallow and deep), an inference model on the CPU
reports 'ops' and the start-up line says why, and the host arithmetic that
says whether the one-launch shallow torso runs (whole_form /
cf32_shallow_form) gives the right answers."""

import logging

import pytest
import torch

from scalable_agent_amd import experiment
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent


def test_whole_parses_and_the_default_stays_ops():
  assert flags_lib.parse_flags(['--torso_blocks=whole']).torso_blocks == 'whole'
  assert flags_lib.parse_flags([]).torso_blocks == 'ops'
  assert flags_lib.default_flags().torso_blocks == 'ops'
  assert Agent(9, torso_blocks='whole').torso_blocks == 'whole'
  assert Agent(9).torso_blocks == 'ops'


def test_unknown_value_still_raises():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--torso_blocks=all'])
  with pytest.raises(ValueError):
    Agent(9, torso_blocks='all')


@pytest.mark.parametrize('torso', ['shallow', 'deep'])
def test_whole_on_the_torch_backend_equals_ops(torso):
  shape = (24, 32, 3)
  mk = lambda blocks: Agent(9, torso=torso, frame_shape=shape, seed=3,
                            backend='torch', torso_blocks=blocks)
  whole, ops = mk('whole'), mk('ops')
  assert whole.torso_whole_form() is None
  assert whole.torso_whole_form(cuda=False) is None
  assert not whole.torso_blocks_fused()
  assert whole.torso_head_form() is None and whole.torso_stage_form() is None
  g = torch.Generator().manual_seed(7)
  frames = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
  with torch.no_grad():
    assert torch.equal(whole.conv_features(frames), ops.conv_features(frames))


def test_shallow_answers_of_the_older_forms_are_unchanged():
  ag = Agent(9, torso='shallow', backend='hip', torso_blocks='whole')
  assert ag.torso_blocks_fused() is False
  assert ag.torso_stage_form() is None and ag.torso_head_form() is None
  assert ag.torso_whole_form(cuda=False) is None


def _log_lines(caplog, flags, model):
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_blocks(flags, model)
  return [r.getMessage() for r in caplog.records
          if 'torso blocks' in r.getMessage()]


def test_start_up_log_line_says_why_whole_does_not_apply(caplog):
  flags = flags_lib.parse_flags(['--torso_blocks=whole'])
  model = inference.InferenceModel(
      Agent(9, torso='shallow', seed=3, torso_blocks='whole'), 'cpu')
  assert model.torso_blocks == 'ops'
  lines = _log_lines(caplog, flags, model)
  assert len(lines) == 1
  assert lines[0].startswith('actor inference torso blocks: ops (')
  assert '--torso_blocks=whole does not apply' in lines[0]
  assert 'torch backend' in lines[0]


def test_start_up_log_line_of_the_older_values_is_unchanged(caplog):
  flags = flags_lib.parse_flags(['--torso_blocks=fused'])
  model = inference.InferenceModel(
      Agent(9, torso='shallow', seed=3, torso_blocks='fused'), 'cpu')
  lines = _log_lines(caplog, flags, model)
  assert lines == ['actor inference torso blocks: ops (--torso_blocks=fused '
                   'does not apply: the torch backend has no block kernel)']


def test_whole_form_host_arithmetic():
  from scalable_agent_amd import ops
  if not ops.available():
    pytest.skip('the HIP extension is not built')
  from scalable_agent_amd.ops import conv_f32
  C = ops.ext()
  for shape in [(72, 96, 3), (84, 84, 4), (72, 128, 3), (72, 96, 1)]:
    assert conv_f32.whole_form(shape) == 'shallow', shape
    assert conv_f32.whole_form(shape, frames=512) == 'shallow', shape
    assert C.cf32_shallow_form(1, *shape) == 1, shape
    assert C.cf32_shallow_form(150, *shape) == 1, shape
  assert conv_f32.whole_form((16, 16, 3)) is None
  assert conv_f32.whole_form((72, 96, 3), frames=513) is None
  assert C.cf32_shallow_form(5, 16, 16, 3) == 0
  assert C.cf32_shallow_form(513, 72, 96, 3) == 0
  assert C.cf32_shallow_form(0, 72, 96, 3) == 0
  assert C.cf32_shallow_form(5, 72, 96, 5) == 0
  # an fp32 HIP shallow agent asks the same function
  ag = Agent(9, torso='shallow', backend='hip', torso_blocks='whole')
  assert ag.torso_whole_form() == 'shallow'
  assert Agent(9, torso='shallow', backend='hip', frame_shape=(16, 16, 3),
               torso_blocks='whole').torso_whole_form() is None
  assert Agent(9, torso='shallow', backend='hip',
               torso_blocks='ops').torso_whole_form() is None
  assert Agent(9, torso='deep', backend='hip',
               torso_blocks='whole').torso_whole_form() is None
