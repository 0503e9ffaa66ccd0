"""Agent(torso_stages='fused') on the GPU: a bf16 HIP deep agent's no-grad conv
features come from the one-launch stages (stage_fwd_kernel) and are bitwise
those of 'ops' - through conv_features, Agent.step and a captured graph of an
inference step; under autograd and above 512 frames the launches of 'ops'
run."""

import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent
from scalable_agent_amd.structs import StepOutput

pytestmark = pytest.mark.gpu

FRAMES = [((72, 96, 3), ('tail', 'stage', 'stage')),
          ((84, 84, 4), ('tail', 'stage', 'stage')),
          ((72, 128, 3), (None, 'stage', 'stage'))]


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _agent(cuda, shape, stages, seed=3):
  ag = Agent(9, torso='deep', frame_shape=shape, seed=seed, backend='hip',
             compute_dtype=torch.bfloat16, torso_stages=stages).to(cuda)
  # non-zero biases (the initialiser's are zero)
  g = torch.Generator().manual_seed(seed + 1)
  with torch.no_grad():
    for name, p in ag.convnet.items():
      if name.endswith('__b'):
        p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(cuda))
  return ag


def _frames(cuda, n, shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8).to(cuda)


def _last_family():
  return _C().conv_launch_info('')['family']


@pytest.mark.parametrize('shape,forms', FRAMES)
def test_conv_features_and_step_are_bitwise_ops(cuda, shape, forms):
  fused, plain = _agent(cuda, shape, 'fused'), _agent(cuda, shape, 'ops')
  assert fused.torso_stages_form() == forms
  assert plain.torso_stages_form() is None
  assert not fused.torso_blocks_fused()
  frames = _frames(cuda, 3, shape, 5)
  with torch.no_grad():
    a = fused.conv_features(frames)
    assert _last_family() == 'stage_bf16'
    assert _C().conv_launch_info('stage_bf16')['ntiles'] == 3
    b = plain.conv_features(frames)
    assert _last_family() == 'res_block_fwd'
  assert a.dtype == torch.bfloat16 and a.shape == (3, fused.flat_size)
  assert a.float().abs().max().item() > 0
  assert torch.equal(a, b)
  g = torch.Generator().manual_seed(4)
  eo = StepOutput(torch.randn(3, generator=g).to(cuda), None,
                  torch.tensor([False, True, False], device=cuda), (frames, None))
  last = torch.randint(0, 9, (3,), generator=g).to(cuda)
  state = (torch.randn(3, 256, generator=g).to(cuda),
           torch.randn(3, 256, generator=g).to(cuda))
  outs = []
  for ag in (fused, plain):
    with torch.no_grad():
      out, (c2, h2) = ag.step(last, eo, state,
                              generator=torch.Generator(cuda).manual_seed(0))
    outs.append((out.policy_logits, out.baseline, c2, h2))
  for name, x, y in zip(('logits', 'baseline', 'c', 'h'), *outs):
    assert torch.equal(x, y), name


def test_autograd_and_large_batches_run_the_launches_of_ops(cuda):
  shape = (72, 96, 3)
  fused, plain = _agent(cuda, shape, 'fused'), _agent(cuda, shape, 'ops')
  frames = _frames(cuda, 3, shape, 7)
  with torch.no_grad():
    eager = fused.conv_features(frames)
    assert _last_family() == 'stage_bf16'
  with torch.enable_grad():
    feats = fused.conv_features(frames)
    assert _last_family() == 'res_conv_fwd'  # the learner's two convs per block
    assert feats.requires_grad and torch.equal(feats.detach(), eager)
  big = _frames(cuda, 513, shape, 8)
  with torch.no_grad():
    a = fused.conv_features(big)
    assert _last_family() == 'res_conv_fwd'
    assert torch.equal(a, plain.conv_features(big))
    assert torch.equal(a[:3], fused.conv_features(big[:3]))
    assert _last_family() == 'stage_bf16'


def test_inference_model_reports_and_graph_replays(cuda):
  """One captured InferenceModel step on static buffers, replayed on new
  inputs, against the same model's eager steps."""
  shape, B = (72, 96, 3), 3
  model = inference.InferenceModel(_agent(cuda, shape, 'fused'), cuda,
                                   use_instruction=False, seed=3)
  assert model.torso_stages == ('tail', 'stage', 'stage')
  assert model.torso_blocks == 'ops'
  plain = inference.InferenceModel(_agent(cuda, shape, 'ops'), cuda,
                                   use_instruction=False, seed=3)
  assert plain.torso_stages is None

  def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    frame = torch.randint(0, 256, (B,) + shape, generator=g, dtype=torch.uint8)
    reward = 2.0 * torch.randn(B, generator=g)
    done = torch.arange(B) % 2 == 1
    last = torch.randint(0, 9, (B,), generator=g)
    c, h = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
    ids = torch.zeros(B, 16, dtype=torch.int64)
    ln = torch.zeros(B, dtype=torch.int64)
    return [t.to(cuda) for t in (last, reward, done, frame, ids, ln, c, h)]

  batches = [inputs(10 + k) for k in range(3)]
  s = model.stream
  s.wait_stream(torch.cuda.current_stream(cuda))
  with model._lock, torch.cuda.stream(s):
    eager = []
    for ins in batches:
      outs = model.step_device(*ins, has_instr=False)
      assert _last_family() == 'stage_bf16'
      eager.append([o.clone() for o in outs[1:]])
    assert not torch.equal(eager[1][0], eager[2][0])
    bufs = [t.clone() for t in batches[0]]
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
      out = model.step_device(*bufs, has_instr=False)
    for k in (1, 2):
      for dst, src in zip(bufs, batches[k]):
        dst.copy_(src)
      g.replay()
      s.synchronize()
      for name, x, y in zip(('logits', 'baseline', 'c', 'h'), out[1:], eager[k]):
        assert torch.equal(x, y), (k, name)
  torch.cuda.current_stream(cuda).wait_stream(s)
