"""Agent(torso_blocks='whole') on the GPU: an fp32 HIP shallow agent's no-grad
conv features come from the one-launch torso (cf32_shallow_fwd) and are
bitwise those of 'ops', through conv_features, an InferenceModel step (with
either actor core) and a captured graph; a frame the kernel does not take and
any call under autograd run the launches of 'ops'; a deep agent built with
'whole' runs as 'heads'."""

import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent

pytestmark = pytest.mark.gpu


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _agent(cuda, shape, blocks, torso='shallow', core='ops', seed=3):
  ag = Agent(9, torso=torso, frame_shape=shape, seed=seed, backend='hip',
             compute_dtype=torch.float32, torso_blocks=blocks,
             actor_core=core).to(cuda)
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


def _family_of(fn):
  C = _C()
  C.cf32_launch_info(True)
  out = fn()
  return out, C.cf32_launch_info(True)['family']


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_conv_features_are_bitwise_ops(cuda, shape):
  whole, plain = _agent(cuda, shape, 'whole'), _agent(cuda, shape, 'ops')
  assert whole.torso_whole_form() == 'shallow'
  assert plain.torso_whole_form() is None
  assert not whole.torso_blocks_fused() and whole.torso_head_form() is None
  frames = _frames(cuda, 3, shape, 5)
  with torch.no_grad():
    a, fam = _family_of(lambda: whole.conv_features(frames))
    b, fam_ops = _family_of(lambda: plain.conv_features(frames))
  assert fam == 'shallow_whole' and fam_ops == 'conv_fwd'
  assert a.shape == (3, whole.flat_size) and a.abs().max().item() > 0
  assert torch.equal(a, b)


def _model(cuda, shape, blocks, core):
  return inference.InferenceModel(_agent(cuda, shape, blocks, core=core), cuda,
                                  use_instruction=False, seed=3)


def _step(model, cuda, B, shape):
  g = torch.Generator().manual_seed(4)
  frame = torch.randint(0, 256, (B,) + shape, generator=g, dtype=torch.uint8)
  reward = 2.0 * torch.randn(B, generator=g)
  done = torch.arange(B) % 4 == 2
  last = torch.randint(0, 9, (B,), generator=g)
  c, h = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
  ids = torch.zeros(B, 16, dtype=torch.int64)
  ln = torch.zeros(B, dtype=torch.int64)
  ins = [t.to(cuda) for t in (last, reward, done, frame, ids, ln, c, h)]
  with model._lock, torch.cuda.stream(model.stream):
    outs = model.step_device(*ins, has_instr=False)
    model.stream.synchronize()
  return [o.cpu() for o in outs]


@pytest.mark.parametrize('core', ['ops', 'fused'])
@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_inference_step_equals_ops(cuda, shape, core):
  """Same Philox seed, same weights: actions, logits, baseline and state of a
  step with the one-launch torso equal those with the ops torso, with either
  actor core after it."""
  whole, plain = _model(cuda, shape, 'whole', core), _model(cuda, shape, 'ops', core)
  assert whole.torso_blocks == 'whole' and plain.torso_blocks == 'ops'
  assert whole.actor_core == core and plain.actor_core == core
  a, b = _step(whole, cuda, 3, shape), _step(plain, cuda, 3, shape)
  for name, x, y in zip(('action', 'logits', 'baseline', 'c', 'h'), a, b):
    assert torch.equal(x, y), name


def test_a_frame_the_kernel_does_not_take_runs_ops(cuda):
  shape = (16, 16, 3)
  whole, plain = _agent(cuda, shape, 'whole'), _agent(cuda, shape, 'ops')
  assert whole.torso_whole_form() is None
  model = inference.InferenceModel(whole, cuda, use_instruction=False, seed=3)
  assert model.torso_blocks == 'ops'
  frames = _frames(cuda, 3, shape, 6)
  with torch.no_grad():
    a, fam = _family_of(lambda: whole.conv_features(frames))
    assert fam == 'conv_fwd'
    assert torch.equal(a, plain.conv_features(frames))


def test_under_autograd_the_learner_path_runs(cuda):
  shape = (72, 96, 3)
  whole, plain = _agent(cuda, shape, 'whole'), _agent(cuda, shape, 'ops')
  frames = _frames(cuda, 3, shape, 7)
  with torch.no_grad():
    eager = whole.conv_features(frames)
  grads = []
  for ag in (whole, plain):
    with torch.enable_grad():
      feats = ag.conv_features(frames)
      assert feats.requires_grad
      assert torch.equal(feats.detach(), eager)
      (feats * feats).sum().backward()
    grads.append({k: p.grad.clone() for k, p in ag.convnet.items()
                  if p.grad is not None})
  assert grads[0] and grads[0].keys() == grads[1].keys()
  for k in grads[0]:
    assert torch.equal(grads[0][k], grads[1][k]), k


def test_graph_capture_and_replay(cuda):
  """A linear graph: conv_features captured on a static frame buffer, replayed
  after new frames are written into it."""
  shape = (72, 96, 3)
  whole = _agent(cuda, shape, 'whole')
  batches = [_frames(cuda, 3, shape, 8 + k) for k in range(3)]
  with torch.no_grad():
    eager = [whole.conv_features(f).clone() for f in batches]
  assert not torch.equal(eager[1], eager[2])
  buf = batches[0].clone()
  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side), torch.no_grad():
    whole.conv_features(buf)  # warm-up
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      out = whole.conv_features(buf)
    for k in (1, 2):
      buf.copy_(batches[k])
      g.replay()
      side.synchronize()
      assert torch.equal(out, eager[k]), k
  torch.cuda.current_stream(cuda).wait_stream(side)


def test_whole_on_a_deep_torso_is_heads(cuda):
  shape = (72, 96, 3)
  whole = _agent(cuda, shape, 'whole', torso='deep')
  heads = _agent(cuda, shape, 'heads', torso='deep')
  assert whole.torso_whole_form() is None
  assert whole.torso_blocks_fused() and whole.torso_head_form() == (0, 1)
  assert whole.torso_stage_form() == heads.torso_stage_form() == 'stage'
  model = inference.InferenceModel(whole, cuda, use_instruction=False, seed=3)
  assert model.torso_blocks == 'heads'
  frames = _frames(cuda, 3, shape, 9)
  with torch.no_grad():
    assert torch.equal(whole.conv_features(frames), heads.conv_features(frames))
