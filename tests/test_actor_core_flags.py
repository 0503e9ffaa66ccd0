"""--actor_core / Agent(actor_core=...) without a GPU: the flag parses, and
'fused' on the CPU or the torch backend runs the ops path unchanged."""

import pytest
import torch

from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent
from scalable_agent_amd.structs import StepOutput


def test_actor_core_flag_parses_and_defaults_to_ops():
  assert flags_lib.parse_flags([]).actor_core == 'ops'
  assert flags_lib.parse_flags(['--actor_core=fused']).actor_core == 'fused'
  assert flags_lib.parse_flags(['--actor_core', 'ops']).actor_core == 'ops'
  assert flags_lib.default_flags().actor_core == 'ops'


def test_actor_core_flag_rejects_unknown_value():
  with pytest.raises(SystemExit):
    flags_lib.parse_flags(['--actor_core=megakernel'])
  with pytest.raises(ValueError):
    Agent(9, actor_core='megakernel')


def _step(agent, B=5):
  g = torch.Generator().manual_seed(11)
  frame = torch.randint(0, 255, (B, 72, 96, 3), generator=g, dtype=torch.uint8)
  done = torch.tensor([False, True, False, False, True])
  eo = StepOutput(3.0 * torch.randn(B, generator=g), None, done, (frame, None))
  last = torch.randint(0, 9, (B,), generator=g)
  state = (torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g))
  with torch.no_grad():
    out, (c2, h2) = agent.step(last, eo, state,
                               generator=torch.Generator().manual_seed(5))
  return out.action, out.policy_logits, out.baseline, c2, h2


@pytest.mark.parametrize('heads', [1, 5])
def test_fused_on_cpu_runs_the_ops_path(heads):
  mk = lambda core: Agent(9, torso='shallow', seed=3, backend='torch',
                          num_value_heads=heads, actor_core=core)
  fused, ops = mk('fused'), mk('ops')
  assert fused.actor_core == 'fused' and ops.actor_core == 'ops'
  assert not fused.actor_core_fused(torch.Generator(), cuda=False)
  for a, b in zip(_step(fused), _step(ops)):
    assert torch.equal(a, b)
  # no fused-core entry is packed for an agent that cannot run it
  fused.inference_cache()
  assert fused._inference_cache is None


def test_inference_model_reports_its_core_on_cpu():
  model = inference.InferenceModel(
      Agent(9, torso='shallow', seed=3, actor_core='fused'), 'cpu')
  assert model.actor_core == 'ops'
  with pytest.raises(ValueError):
    model.agent.step(
        torch.zeros(1, dtype=torch.int64),
        StepOutput(torch.zeros(1), None, torch.zeros(1, dtype=torch.bool),
                   (torch.zeros(1, 72, 96, 3, dtype=torch.uint8), None)),
        model.agent.initial_state(1), epilogue=object())
