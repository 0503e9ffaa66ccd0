"""--torso_blocks=whole on 5-16 channel frames without a GPU: the launcher's
host arithmetic, Agent.torso_whole_form and the start-up log line."""
import logging

import pytest
import torch

from scalable_agent_amd import experiment, inference, ops
from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd.models import Agent

pytestmark = pytest.mark.skipif(not ops.available(),
                                reason='the HIP extension is not built')

YES = [(h, w, c) for h, w in [(72, 96), (84, 84), (72, 128)]
       for c in (5, 8, 9, 12, 13, 16) if w != 128 or c in (9, 12)]  # no ops tile: 72x128 at Cp 8 / 16
NO = [((72, 96, 12), 0), ((72, 96, 12), 513), ((72, 96, 4), 1), ((72, 96, 17), 1),
      ((64, 64, 12), 1), ((72, 128, 8), 1), ((72, 128, 13), 1)]


@pytest.mark.parametrize('shape,n', [(s, n) for s in YES for n in (1, 512)] + NO)
def test_form(shape, n):
  from scalable_agent_amd.ops import conv_f32
  want = 'shallow_wide' if shape in YES and n in (1, 512) else None
  assert conv_f32.whole_wide_form(shape, frames=n) == want
  assert ops.ext().cf32_shallow_wide_form(n, *shape) == (want is not None)
  rows, lds = ops.ext().cf32_shallow_wide_band(*shape)
  assert (rows >= 1 and 0 < lds <= 160 * 1024) if shape in YES else rows == 0


def _agent(**kw):
  return Agent(9, **dict(dict(torso='shallow', backend='hip', seed=3,
                              frame_shape=(72, 96, 12), torso_blocks='whole'), **kw))


def test_agent_form():
  assert _agent().torso_whole_form() == 'shallow_wide'
  assert _agent().torso_whole_form(cuda=False) is None
  assert _agent(torso_blocks='ops').torso_whole_form() is None
  assert _agent(torso='deep').torso_whole_form() is None
  assert _agent(compute_dtype=torch.bfloat16).torso_whole_form() is None


def test_start_up_log_line_names_the_wide_form(caplog, monkeypatch):
  flags = flags_lib.parse_flags(['--torso_blocks=whole'])
  model = inference.InferenceModel(_agent(), 'cpu')  # a CUDA model reports:
  monkeypatch.setattr(inference.InferenceModel, 'torso_blocks', 'whole')
  with caplog.at_level(logging.INFO, logger='scalable_agent_amd'):
    experiment._log_torso_blocks(flags, model)
  lines = [r.getMessage() for r in caplog.records if 'torso blocks' in r.getMessage()]
  assert len(lines) == 1 and '72x96x12' in lines[0]
  assert lines[0].startswith('actor inference torso blocks: whole (shallow_wide:')
