"""--torso_blocks=heads / Agent(torso_blocks='heads') without a GPU: the value
parses, an unknown one still raises, the torch backend runs as with 'ops', and
the host arithmetic that says which form runs (head_form / stage_form) gives
the right answers for the three supported frames and for a declined shape."""

import logging

import pytest
import torch

from scalable_agent_amd import experiment
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent


def test_heads_parses_and_the_default_stays_ops():
  assert flags_lib.parse_flags(['--torso_blocks=heads']).torso_blocks == 'heads'
  assert flags_lib.parse_flags(['--torso_blocks', 'stage']).torso_blocks == 'stage'
  assert flags_lib.parse_flags([]).torso_blocks == 'ops'
  assert flags_lib.default_flags().torso_blocks == 'ops'
  assert Agent(9, torso_blocks='heads').torso_blocks == 'heads'


def test_unknown_value_still_raises():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--torso_blocks=head'])
  with pytest.raises(ValueError):
    Agent(9, torso_blocks='head')


def test_heads_on_the_torch_backend_builds_and_equals_ops():
  shape = (24, 32, 3)
  mk = lambda blocks: Agent(9, torso='deep', frame_shape=shape, seed=3,
                            backend='torch', torso_blocks=blocks)
  heads, ops = mk('heads'), mk('ops')
  assert not heads.torso_blocks_fused() and not heads.torso_blocks_fused(cuda=False)
  assert heads.torso_head_form() is None and heads.torso_stage_form() is None
  g = torch.Generator().manual_seed(7)
  frames = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
  with torch.no_grad():
    assert torch.equal(heads.conv_features(frames), ops.conv_features(frames))


def test_start_up_log_line_says_where_heads_cannot_apply(caplog):
  flags = flags_lib.parse_flags(['--torso_blocks=heads'])
  model = inference.InferenceModel(
      Agent(9, torso='shallow', seed=3, torso_blocks='heads'), 'cpu')
  assert model.torso_blocks == 'ops'
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_blocks(flags, model)
  lines = [r.getMessage() for r in caplog.records
           if 'torso blocks' in r.getMessage()]
  assert len(lines) == 1
  assert lines[0].startswith('actor inference torso blocks: ops (')
  assert '--torso_blocks=heads does not apply' in lines[0]


def test_head_form_and_stage_form_host_arithmetic():
  from scalable_agent_amd import ops
  if not ops.available():
    pytest.skip('the HIP extension is not built')
  from scalable_agent_amd.ops import conv_f32
  C = ops.ext()
  # the three supported frames: both heads fuse; the last stage as 'stage'
  for shape, last in [((72, 96, 3), 'stage'), ((84, 84, 4), 'tail'),
                      ((72, 128, 3), 'tail'), ((72, 96, 1), 'stage')]:
    assert conv_f32.head_form(shape) == (0, 1), shape
    assert conv_f32.head_form(shape, frames=150) == (0, 1), shape
    assert conv_f32.stage_form(shape) == last, shape
  # declined: a frame no instance covers, and too many frames for a launch
  assert conv_f32.head_form((20, 28, 3)) == ()
  assert conv_f32.stage_form((20, 28, 3)) is None
  assert conv_f32.head_form((72, 96, 3), frames=513) == ()
  # the binding's own answers: (N, H, W, cin, cout, uint8 frames)
  assert C.cf32_head_form(5, 72, 96, 3, 16, True) == 1
  assert C.cf32_head_form(5, 36, 48, 16, 32, False) == 1
  assert C.cf32_head_form(5, 42, 42, 16, 32, False) == 1
  assert C.cf32_head_form(5, 71, 96, 3, 16, True) == 0   # odd H
  assert C.cf32_head_form(5, 72, 94, 3, 16, True) == 0   # W * 3 % 4 != 0
  assert C.cf32_head_form(5, 18, 24, 32, 32, False) == 0  # stage 2's channels
  assert C.cf32_head_form(5, 72, 96, 3, 16, False) == 0  # fp32 frames
  # band heights (pooled rows per workgroup) divide into >= 6 bands per image
  for (H, W, cin) in [(72, 96, 3), (84, 84, 4), (72, 128, 3), (36, 48, 16),
                      (42, 42, 16), (36, 64, 16)]:
    bp = C.cf32_head_band(H, W, cin)
    assert bp >= 2 and (H // 2 + bp - 1) // bp >= 6, (H, W, cin, bp)
  assert C.cf32_head_band(72, 100, 3) == 0 and C.cf32_head_band(71, 96, 3) == 0
