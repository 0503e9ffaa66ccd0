"""--actor_core=fused for bf16 inference: the flag help, what a CPU / fp32
agent reports, and the padded-K arithmetic of the bf16 packing (no GPU)."""

import pytest
import torch

from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import actor_core


def _help_of(name):
  parser = flags_lib.build_parser()
  for a in parser._actions:
    if '--' + name in a.option_strings:
      return ' '.join(a.help.split())
  raise AssertionError(name)


def test_help_mentions_bf16():
  text = _help_of('actor_core')
  assert 'bf16' in text and 'fused' in text
  assert 'bf16 inference runs ops' not in text
  assert 'not bitwise' in text


def _model(dtype, core, backend='torch'):
  agent = Agent(9, torso='shallow', frame_shape=(72, 96, 3), seed=1,
                backend=backend, compute_dtype=dtype, actor_core=core)
  return inference.InferenceModel(agent, 'cpu', use_instruction=False, seed=3)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('backend', ['torch', 'hip'])
def test_cpu_agent_reports_ops_and_steps(dtype, backend):
  """'fused' on the CPU runs the ops path and says so, for bf16 as for fp32."""
  model = _model(dtype, 'fused', backend)
  assert model.actor_core == 'ops'
  assert model.agent.actor_core == 'fused'
  assert model.agent._inference_cache is None
  assert not model.agent.actor_core_fused(model._gen, cuda=False)
  if backend == 'hip':  # HIP ops take GPU tensors only: nothing to step here
    return
  import numpy as np
  B = 3
  out = model.infer(np.zeros(B, np.int64), np.zeros(B, np.float32),
                    np.zeros(B, bool), np.zeros((B, 72, 96, 3), np.uint8),
                    np.zeros((B, 16), np.int64), np.zeros(B, np.int64),
                    np.zeros((B, 256), np.float32),
                    np.zeros((B, 256), np.float32))
  assert out[1].shape == (B, 9) and np.isfinite(out[1]).all()


def test_fused_condition_by_dtype():
  """What actor_core_fused() asks of the agent, a GPU assumed: fp32 as before,
  bf16 now too, nothing else; a torch.Generator or > 63 actions decline."""
  from scalable_agent_amd.ops.heads import PhiloxStream
  stream = PhiloxStream(1)
  mk = lambda dt, A=9, core='fused': Agent(
      A, torso='shallow', frame_shape=(72, 96, 3), seed=1, backend='hip',
      compute_dtype=dt, actor_core=core)
  for dt in (torch.float32, torch.bfloat16):
    agent = mk(dt)
    want = agent.fused_core_ready()
    assert agent.actor_core_fused(stream) == want
    assert not agent.actor_core_fused(torch.Generator())
    assert not agent.actor_core_fused(stream, cuda=False)
    assert not mk(dt, A=64).actor_core_fused(stream)
    assert not mk(dt, core='ops').actor_core_fused(stream)


@pytest.mark.parametrize('A', [31, 32])
@pytest.mark.parametrize('instr', [False, True])
def test_padded_k(A, instr):
  K = 257 + A + (64 if instr else 0)
  kpad = actor_core.padded_k_bf16(K)
  assert kpad % 32 == 0 and 0 <= kpad - K < 32
  assert kpad == {(31, False): 288, (32, False): 320, (31, True): 352,
                  (32, True): 384}[(A, instr)]
  kmax = actor_core.packed_rows_bf16(A)
  assert kmax % 32 == 0 and kmax >= kpad and kmax >= 257 + A + 64
  assert actor_core.packed_rows(A) % 16 == 0  # the fp32 packing is unchanged
  assert actor_core.packed_rows(A) == (257 + A + 64 + 15) // 16 * 16
  try:
    from scalable_agent_amd import ops
    ops.load()
    info = actor_core.actor_core_bf16_info(76, K, A)
  except Exception as e:  # the extension is not importable here
    pytest.skip('HIP extension not importable: %r' % (e,))
  assert info['kpad'] == kpad and info['ksteps'] == kpad // 32 + 8
  assert info['grid'] == (32, 5) and info['width'] == 32
  assert kmax <= info['max_k']
