"""--torso_stages / Agent(torso_stages=...) without a GPU: the value parses and
defaults to 'ops', an unknown one is rejected, the torch backend runs as with
'ops', the host arithmetic that picks each stage's one-launch form
(deep_stage_bf16_form) gives the right answers and agrees with the binding's
stage_bf16_form, the start-up line names the forms or says why the flag does
not apply, and an fp32 deep agent keeps its --torso_blocks behaviour."""

import logging

import pytest
import torch

from scalable_agent_amd import experiment
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv

FRAMES = {(72, 96, 3): ('tail', 'stage', 'stage'),
          (84, 84, 4): ('tail', 'stage', 'stage'),
          # the 36x64x16 maps of stage 0 exceed the LDS: its blocks stay launches
          (72, 128, 3): (None, 'stage', 'stage')}


def test_flag_parses_and_defaults_to_ops():
  assert flags_lib.parse_flags(['--torso_stages=fused']).torso_stages == 'fused'
  assert flags_lib.parse_flags([]).torso_stages == 'ops'
  assert flags_lib.default_flags().torso_stages == 'ops'
  assert Agent(9, torso_stages='fused').torso_stages == 'fused'
  assert Agent(9).torso_stages == 'ops'


def test_unknown_value_is_rejected():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--torso_stages=all'])
  with pytest.raises(ValueError):
    Agent(9, torso_stages='all')
  with pytest.raises(ValueError):
    Agent(9, torso_stages='stage')


@pytest.mark.parametrize('torso', ['shallow', 'deep'])
def test_fused_on_the_torch_backend_equals_ops(torso):
  shape = (24, 32, 3)
  mk = lambda stages: Agent(9, torso=torso, frame_shape=shape, seed=3,
                            backend='torch', torso_stages=stages)
  fused, ops = mk('fused'), mk('ops')
  assert fused.torso_stages_form(cuda=False) is None
  assert fused.torso_stages_form() is None
  assert ops.torso_stages_form() is None
  g = torch.Generator().manual_seed(7)
  frames = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
  with torch.no_grad():
    assert torch.equal(fused.conv_features(frames), ops.conv_features(frames))


def test_deep_stage_form_host_arithmetic():
  for shape, forms in FRAMES.items():
    assert conv.deep_stage_bf16_form(shape) == forms, shape
    assert conv.deep_stage_bf16_form(shape, frames=512) == forms, shape
    assert conv.deep_stage_bf16_form(shape, frames=0) == (None,) * 3, shape
    assert conv.deep_stage_bf16_form(shape, frames=513) == (None,) * 3, shape
  assert conv.deep_stage_bf16_form((72, 96)) == (None,) * 3
  # the kernel's LDS against the 160 KB of a CU
  assert conv.stage_bf16_lds_bytes(36, 48, 16, 16) == 134208
  assert conv.stage_bf16_lds_bytes(42, 42, 16, 16) == 136512
  assert conv.stage_bf16_lds_bytes(36, 64, 16, 16) == 173120 > 160 * 1024
  # channels the kernel is not built for
  assert conv.stage_bf16_form(3, 36, 48, 32, 16) == 0
  assert conv.stage_bf16_form(3, 36, 48, 16, 8) == 0
  assert conv.stage_bf16_form(3, 36, 48, 3, 16) == 0


def test_form_agrees_with_the_binding():
  from scalable_agent_amd import ops
  if not ops.available():
    pytest.skip('the HIP extension is not built')
  C = ops.ext()
  sizes = [(36, 48), (42, 42), (36, 64), (18, 24), (21, 21), (18, 32), (12, 16),
           (10, 14), (5, 7), (6, 8), (1, 1), (72, 96), (84, 84), (72, 128),
           (40, 60), (3, 600), (200, 30), (64, 64), (50, 300), (9, 1100)]
  for h, w in sizes:
    for cin, cout in [(16, 16), (16, 32), (32, 32), (32, 16), (3, 16)]:
      for n in (0, 1, 150, 512, 513):
        assert (C.stage_bf16_form(n, h, w, cin, cout) ==
                conv.stage_bf16_form(n, h, w, cin, cout)), (n, h, w, cin, cout)
  assert C.stage_bf16_form(3, 36, 48, 16, 16) == 2
  assert C.stage_bf16_form(3, 36, 48, 16, 32) == 1
  assert C.stage_bf16_form(3, 18, 24, 32, 32) == 1
  assert C.stage_bf16_form(3, 36, 64, 16, 16) == 0
  assert C.stage_bf16_form(0, 36, 48, 16, 16) == 0
  assert C.stage_bf16_form(513, 36, 48, 16, 32) == 0


def _hip_agent(**kw):
  kw.setdefault('torso', 'deep')
  kw.setdefault('compute_dtype', torch.bfloat16)
  return Agent(9, backend='hip', seed=3, torso_stages='fused', **kw)


def test_agent_form():
  for shape, forms in FRAMES.items():
    assert _hip_agent(frame_shape=shape).torso_stages_form() == forms
    assert _hip_agent(frame_shape=shape).torso_stages_form(cuda=False) is None
  assert _hip_agent(compute_dtype=torch.float32).torso_stages_form() is None
  assert _hip_agent(torso='shallow').torso_stages_form() is None
  # a frame the bf16 kernels do not cover (conv.supports)
  assert _hip_agent(frame_shape=(72, 96, 1)).torso_stages_form() is None
  assert Agent(9, torso='deep', backend='hip', compute_dtype=torch.bfloat16
               ).torso_stages_form() is None


class _Model(object):
  """What _log_torso_stages reads of an InferenceModel on a GPU."""

  def __init__(self, agent):
    self.agent = agent
    self.device = torch.device('cuda')
    self.torso_stages = agent.torso_stages_form(True)


def _log_lines(caplog, flags, model):
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_stages(flags, model)
  return [r.getMessage() for r in caplog.records
          if 'torso stages' in r.getMessage()]


def test_start_up_log_line(caplog):
  flags = flags_lib.parse_flags(['--torso_stages=fused'])
  lines = _log_lines(caplog, flags, _Model(_hip_agent(frame_shape=(72, 128, 3))))
  assert lines == [
      'actor inference torso stages: fused on 72x128x3 frames: '
      'stage 0 ops (declines), '
      'stage 1 stage (head, max-pool and both blocks in one launch), '
      'stage 2 stage (head, max-pool and both blocks in one launch)']
  caplog.clear()
  lines = _log_lines(caplog, flags, _Model(_hip_agent()))
  assert len(lines) == 1 and 'stage 0 tail (both blocks in one launch)' in lines[0]
  caplog.clear()
  lines = _log_lines(caplog, flags,
                     _Model(_hip_agent(compute_dtype=torch.float32)))
  assert lines == ['actor inference torso stages: ops (--torso_stages=fused does '
                   'not apply: the one-launch stages are bf16 only (see '
                   '--torso_blocks for fp32))']
  caplog.clear()
  lines = _log_lines(caplog, flags, _Model(_hip_agent(torso='shallow')))
  assert lines == ['actor inference torso stages: ops (--torso_stages=fused does '
                   'not apply: the shallow torso has no stages)']
  caplog.clear()
  # a real inference model on the CPU: the torch backend
  model = inference.InferenceModel(
      Agent(9, torso='deep', seed=3, torso_stages='fused'), 'cpu')
  assert model.torso_stages is None
  lines = _log_lines(caplog, flags, model)
  assert lines == ['actor inference torso stages: ops (--torso_stages=fused does '
                   'not apply: the torch backend has no stage kernel)']
  caplog.clear()
  lines = _log_lines(caplog, flags_lib.parse_flags([]), model)
  assert lines == ['actor inference torso stages: ops']


def test_fp32_deep_agent_keeps_its_torso_blocks_behaviour():
  for blocks in ('ops', 'fused', 'stage', 'heads'):
    with_flag = Agent(9, torso='deep', backend='hip', torso_blocks=blocks,
                      torso_stages='fused')
    without = Agent(9, torso='deep', backend='hip', torso_blocks=blocks)
    assert with_flag.torso_stages_form() is None
    assert with_flag.torso_blocks_fused() == without.torso_blocks_fused()
    assert with_flag.torso_stage_form() == without.torso_stage_form()
    assert with_flag.torso_head_form() == without.torso_head_form()
  # and the bf16 agent's --torso_blocks answers stay false
  bf = _hip_agent(torso_blocks='heads')
  assert not bf.torso_blocks_fused() and bf.torso_stage_form() is None
