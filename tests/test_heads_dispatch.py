"""Which head kernel learner.compute_loss selects (no GPU: a stub stands in
for the extension and the ops are spied on).

  (T = 100, A = 9)             the whole-column kernel: time_tile=None
  T = limit + 1 (A = 9, 31)    the time-tiled kernel: time_tile='auto'
  A = 40 (any T)               the time-tiled kernel; the unroll limit is not
                               asked (the helper rejects A > 31)
  A = 64                       the unfused path (ops.vtrace_loss)
"""

import types

import pytest
import torch

from scalable_agent_amd import learner as learner_lib
from scalable_agent_amd.structs import ActorOutput, AgentOutput, StepOutput

_LIMITS = {9: 1334, 31: 436}


class _StubExt(object):
  """The extension's unroll-limit helper, with the real kernel's limits."""

  def learner_head_max_unroll(self, num_actions):
    if not 1 <= num_actions <= 31:
      raise RuntimeError('1 <= num_actions <= 31')
    return _LIMITS[num_actions]


def _agent(A, K=1):
  def unroll_core(actions, env_outputs, state):
    return torch.zeros(actions.shape[0], actions.shape[1], 256), state

  def unroll(actions, env_outputs, state, sample=False, task_ids=None):
    T1, B = actions.shape
    return AgentOutput(actions, torch.zeros(T1, B, A), torch.zeros(T1, B)), state

  return types.SimpleNamespace(
      num_actions=A, num_value_heads=K, fused_core_ready=lambda instr=None: True,
      unroll_core=unroll_core, unroll=unroll, policy_w=torch.zeros(256, A),
      policy_b=torch.zeros(A), baseline_w=torch.zeros(256, K),
      baseline_b=torch.zeros(K))


def _batch(T, A, B=2):
  T1 = T + 1
  return ActorOutput(
      level_name=None, agent_state=None,
      env_outputs=StepOutput(torch.zeros(T1, B), None,
                             torch.zeros(T1, B, dtype=torch.bool), (None, None)),
      agent_outputs=AgentOutput(torch.zeros(T1, B, dtype=torch.int64),
                                torch.zeros(T1, B, A), None))


@pytest.fixture
def calls(monkeypatch):
  from scalable_agent_amd import ops
  from scalable_agent_amd.ops import heads as heads_mod
  monkeypatch.setattr(heads_mod, 'ext', lambda: _StubExt())
  seen = []

  def heads_spy(core_out, *args, **kw):
    seen.append(('heads', core_out.shape[0] - 1, kw['time_tile']))
    return torch.zeros(())

  def vtrace_spy(*args, **kw):
    seen.append(('vtrace_loss',))
    return torch.zeros(())

  monkeypatch.setattr(ops, 'heads_vtrace_loss', heads_spy)
  monkeypatch.setattr(ops, 'vtrace_loss', vtrace_spy)
  return seen


_FLAGS = types.SimpleNamespace(discounting=0.99, reward_clipping='abs_one',
                               baseline_cost=0.5, entropy_cost=0.01)


@pytest.mark.parametrize('T,A,tile', [
    (100, 9, None), (1334, 9, None), (1335, 9, 'auto'), (436, 31, None),
    (437, 31, 'auto'), (8, 40, 'auto'), (100, 63, 'auto')])
def test_compute_loss_selects_head_kernel(calls, T, A, tile):
  learner_lib.compute_loss(_agent(A), _batch(T, A), _FLAGS, use_fused=True)
  assert calls == [('heads', T, tile)]


def test_compute_loss_leaves_fused_path_at_64_actions(calls):
  learner_lib.compute_loss(_agent(64), _batch(8, 64), _FLAGS, use_fused=True)
  assert calls == [('vtrace_loss',)]


def test_lds_limits_of_the_built_extension():
  """The unroll limits and default tiles that follow from the kernels' LDS
  layouts (160 KB a workgroup, 8400 bytes of static arrays): pinned, since
  a layout that moves a tile moves the bits of every tiled run.  The tiles
  are the ones recorded in profiles/experiments.md."""
  from scalable_agent_amd import ops
  if not ops.available():
    pytest.skip('the HIP extension is not built')
  ext = ops.ext()
  unroll = {9: 1334, 31: 436}
  assert {A: ext.learner_head_max_unroll(A) for A in unroll} == unroll
  tiles = {9: 1024, 18: 672, 31: 416, 40: 240, 63: 160}
  assert {A: ext.learner_head_tile_auto(A) for A in tiles} == tiles


def test_value_heads_count_against_the_64_columns(calls):
  """A + K <= 64 holds for the tiled kernel's callers too."""
  data = _batch(8, 40)._replace(level_name=torch.zeros(2, dtype=torch.int64))
  popart = types.SimpleNamespace(mu=torch.zeros(24), nu=torch.ones(24))
  learner_lib.compute_loss(_agent(40, K=24), data, _FLAGS, use_fused=True,
                           popart=popart, aux={})
  assert calls == [('heads', 8, 'auto')]
