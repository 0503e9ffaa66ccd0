"""bf16 actor inference on the shallow torso (--inference_dtype=bf16
--torso=shallow): Agent._conv_features takes the one-launch bf16 MFMA torso
(csrc/kernels/conv_shallow_bf16.hip) for a no-grad forward of frames the
kernel accepts, and the bf16 FC GEMM and core follow; everything else - the
learner, any call under autograd, frames the kernel declines - runs the
exact-fp32 kernels as before."""

import numpy as np
import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


def _mk(dtype, shape=(72, 96, 3), seed=1, torso='shallow'):
  return Agent(9, torso=torso, frame_shape=shape, seed=seed, backend='hip',
               compute_dtype=dtype)


def _frames(cuda, n, shape, seed=4):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8).to(cuda)


def test_dispatch(cuda):
  ops = _ops()
  C = ops.ext()
  from scalable_agent_amd.ops.conv_f32 import shallow_param_list
  bf, fp = _mk(BF).to(cuda), _mk(F32).to(cuda)
  assert bf.inference_torso_precision() == 'bf16'
  assert fp.inference_torso_precision() == 'fp32'
  frames = _frames(cuda, 7, (72, 96, 3))
  with torch.no_grad():
    got = bf.conv_features(frames)
    want32 = fp.conv_features(frames)
  p = [t.detach() for t in shallow_param_list(bf)]
  wp = C.shallow_bf16_pack(p[0], p[2], p[4])
  direct = C.shallow_bf16_fwd(frames, wp[0], p[1], wp[1], p[3], wp[2], p[5])
  assert C.conv_launch_info('shallow_bf16')['ntiles'] == 7
  assert got.dtype == BF and torch.equal(got, direct.reshape(7, -1))
  assert want32.dtype == F32
  # under autograd: the fp32 kernels, bitwise an fp32 agent's features
  with_grad = bf.conv_features(frames)
  assert with_grad.dtype == F32 and with_grad.requires_grad
  assert torch.equal(with_grad.detach(), want32)
  # a frame the kernel declines: fp32 both ways
  small_bf, small_fp = (_mk(d, (16, 16, 3)).to(cuda) for d in (BF, F32))
  assert small_bf.inference_torso_precision() == 'fp32'
  fs = _frames(cuda, 3, (16, 16, 3))
  with torch.no_grad():
    a, b = small_bf.conv_features(fs), small_fp.conv_features(fs)
  assert a.dtype == F32 and torch.equal(a, b)
  assert torch.equal(small_bf.conv_features(fs).detach(), b)


@pytest.mark.parametrize('dtype', [BF, F32])
def test_inference_weight_cache_tracks_publish(cuda, dtype):
  """test_actor_gpu's test on a shallow agent: a cached InferenceModel step is
  bitwise an uncached agent's step, before and after a publish of other
  weights; the packed conv weights (cache['wsh16']) exist for bf16 only."""
  _ops()
  from scalable_agent_amd.optim import FlatParams
  from scalable_agent_amd.structs import StepOutput
  model = inference.InferenceModel(_mk(dtype, seed=1), cuda, False, seed=3)
  cache = model.agent._inference_cache
  assert cache['w4'] is not None
  assert (cache['w16'] is not None) == (dtype == BF)
  assert (cache.get('wsh16') is not None) == (dtype == BF)
  assert model.torso_precision == ('bf16' if dtype == BF else 'fp32')
  ref, other = _mk(dtype, seed=1).to(cuda), _mk(dtype, seed=2).to(cuda)
  assert ref._inference_cache is None
  B = 10
  g = torch.Generator().manual_seed(4)
  frame = _frames(cuda, B, (72, 96, 3))
  eo = StepOutput(torch.randn(B, generator=g).to(cuda), None,
                  torch.zeros(B, dtype=torch.bool, device=cuda), (frame, None))
  last = torch.randint(0, 9, (B,), generator=g).to(cuda)
  state = (torch.randn(B, 256, generator=g).to(cuda),
           torch.randn(B, 256, generator=g).to(cuda))

  def run(agent):
    with torch.no_grad():
      out, (c2, h2) = agent.step(last, eo, state,
                                 generator=torch.Generator(cuda).manual_seed(0))
    torch.cuda.synchronize()
    return out.policy_logits, out.baseline, c2, h2

  before = run(model.agent)
  for a, b in zip(before, run(ref)):
    assert torch.equal(a, b)
  model.publish(FlatParams(other).params)
  torch.cuda.synchronize()
  after = run(model.agent)
  for a, b in zip(after, run(other)):
    assert torch.equal(a, b)
  assert not torch.equal(before[0], after[0])


def test_vector_infer_graph(cuda):
  """The captured VectorInfer graph on a shallow bf16 agent against the eager
  per-batch InferenceModel.infer of an identical agent."""
  _ops()
  from scalable_agent_amd.inference import InferenceModel, VectorInfer
  M, shape, A = 6, (72, 96, 3), 9
  mk = lambda: _mk(BF, shape, seed=3)
  model = InferenceModel(mk(), 'cuda', use_instruction=False, seed=5)
  ref_model = InferenceModel(mk(), 'cuda', use_instruction=False, seed=5)
  assert model.torso_precision == 'bf16'
  vi = VectorInfer(model, M, shape, A)
  assert vi.use_graph
  rng = np.random.RandomState(0)
  c = np.zeros((M, 256), np.float32)
  h = np.zeros((M, 256), np.float32)
  tol = 2e-2
  for step in range(4):
    frame = rng.randint(0, 256, (M,) + shape).astype(np.uint8)
    reward = rng.randn(M).astype(np.float32)
    done = np.array([step == 0, False, step == 2, False, True, False])
    la = rng.randint(0, A, M).astype(np.int64)
    vi.inputs['frame'][:] = frame
    vi.inputs['reward'][:] = reward
    vi.inputs['done'][:] = done
    vi.inputs['last_action'][:] = la
    _, logits, baseline, c2, h2 = [x.copy() for x in vi.run()]
    _, rl, rb, rc, rh = ref_model.infer(
        la, reward, done, frame, np.zeros((M, 16), np.int64),
        np.zeros(M, np.int64), c, h)
    np.testing.assert_allclose(logits, rl, rtol=tol, atol=tol)
    np.testing.assert_allclose(baseline, rb, rtol=tol, atol=tol)
    np.testing.assert_allclose(h2, rh, rtol=tol, atol=tol)
    c, h = rc, rh


def _step_logit_cos(cuda, torso):
  from scalable_agent_amd.structs import StepOutput
  B = 12
  g = torch.Generator().manual_seed(8)
  frame = _frames(cuda, B, (72, 96, 3), seed=9)
  eo = StepOutput(torch.randn(B, generator=g).to(cuda), None,
                  (torch.rand(B, generator=g) < 0.3).to(cuda), (frame, None))
  last = torch.randint(0, 9, (B,), generator=g).to(cuda)
  state = (torch.randn(B, 256, generator=g).to(cuda),
           torch.randn(B, 256, generator=g).to(cuda))
  logits = []
  for dtype in (BF, F32):
    agent = _mk(dtype, seed=1, torso=torso).to(cuda)
    with torch.no_grad():
      out, _ = agent.step(last, eo, state,
                          generator=torch.Generator(cuda).manual_seed(0))
    logits.append(out.policy_logits.double().flatten())
  a, b = logits
  return (a @ b / (a.norm() * b.norm())).item()


def test_step_logits_track_fp32_like_the_deep_torso(cuda):
  """Step logits of a bf16 shallow agent against its fp32 twin: the cosine is
  no lower than that of the deep bf16 agent (the accepted precedent) against
  its fp32 twin, minus 0.01."""
  _ops()
  shallow = _step_logit_cos(cuda, 'shallow')
  deep = _step_logit_cos(cuda, 'deep')
  print('step-logit cosine bf16 vs fp32: shallow %.6f deep %.6f' %
        (shallow, deep))
  assert shallow >= deep - 0.01
