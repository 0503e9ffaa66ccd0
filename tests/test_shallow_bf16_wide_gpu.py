"""The one-launch bf16 shallow torso on uint8 frames of 5-16 channels
(shallow_bf16w_kernel: channels padded to Cp = 8 / 12 / 16, layer 1 in bands
of output rows), held to the checks of test_shallow_bf16_gpu.py."""

import pytest
import torch

from scalable_agent_amd import ops
from scalable_agent_amd.models import Agent

from . import _shallow_bf16_oracle as O
from .test_shallow_bf16_wide_flag import CASES

pytestmark = pytest.mark.gpu

FAMILY = 'shallow_bf16w'
CHANNELS = (5, 8, 12, 16)
BF, F32 = torch.bfloat16, torch.float32
_PARAMS = {}


def _fwd(C, frames, ws, bs):
  dev = frames.device
  wp = C.shallow_bf16w_pack(*[w.to(dev) for w in ws])
  b = [x.to(dev) for x in bs]
  return C.shallow_bf16w_fwd(frames, wp[0], b[0], wp[1], b[1], wp[2], b[2])


def _params(shape):
  """The agent's own conv initialisation with non-zero biases; CPU, once."""
  if shape not in _PARAMS:
    ag = Agent(9, torso='shallow', frame_shape=shape, seed=5)
    g = torch.Generator().manual_seed(6)
    ws = [ag._conv_params(sp['name'])[0].detach().clone() for sp in ag.specs]
    _PARAMS[shape] = (ws, [torch.randn(w.shape[3], generator=g) * 0.1
                           for w in ws])
  return _PARAMS[shape]


def _frames(n, shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8)


def _cos(a, b):
  a, b = a.double().flatten(), b.double().flatten()
  return (a @ b / (a.norm() * b.norm())).item()


@pytest.mark.parametrize('shape', [(72, 96, c) for c in CHANNELS] +
                         [(84, 84, 12), (72, 128, 12)])
def test_exact_integers_against_float64(cuda, shape):
  """Bytes 0 / 255 and +-1 taps: every stored value is an integer bf16 holds
  (bounds (4, 26, 242) for any C).  The phases put a weight on every layer-1
  tap; the frames run 3, 3 and 5 bands."""
  C = ops.ext()
  frames = O.binary_frames(shape, 3)
  for phase in range(-(-64 * shape[2] // 96)):
    ws, bs = O.integer_weights(shape[2], phase)
    bounds = O.running_bounds(ws, bs)
    assert all(b <= want <= 256 for b, want in zip(bounds, O.BOUNDS)), bounds
    ref = O.chain64(frames, ws, bs)
    assert torch.equal(ref, ref.round()) and ref.max().item() <= 256 and (
        (ref != 0).double().mean().item() > 0.5)
    out = _fwd(C, frames.to(cuda), ws, bs)
    assert out.dtype == BF and tuple(out.shape) == (3,) + O.out_shape(shape)
    assert torch.equal(out.double().cpu(), ref), phase


@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('c', CHANNELS)
def test_capped_grid_is_bitwise_the_uncapped(cuda, c, N):
  """Capped at 2, a workgroup walks images 0, 2, 4 through the same LDS;
  image 0 (zeros) and the last (all 255) give the rows they give alone."""
  C = ops.ext()
  ws, bs = _params((72, 96, c))
  frames = _frames(N, (72, 96, c), 11 + N).clone()
  frames[0], frames[N - 1] = 0, 255
  frames = frames.to(cuda)
  outs = []
  for cap in (0, 2, 0):
    old = C.conv_tune('shallow_bf16_grid', cap)
    outs.append(_fwd(C, frames, ws, bs))
    C.conv_tune('shallow_bf16_grid', old)
    info = C.conv_launch_info(FAMILY)
    assert info['family'] == FAMILY == C.conv_launch_info()['family']
    assert info['grid'] == (min(N, cap) if cap else N)
    assert info['ntiles'] == N and info['rows'] == 3
  assert outs[0].float().abs().max().item() > 0
  assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
  for i in (0, N - 1):
    alone = _fwd(C, frames[i:i + 1].contiguous(), ws, bs)
    assert torch.equal(outs[1][i:i + 1], alone), i


@pytest.mark.parametrize('shape', [(72, 96, 12), (84, 84, 8)])
def test_realistic_weights_track_the_oracle(cuda, shape):
  """test_shallow_bf16_gpu's rule on 6 frames (max |err| / max |ref| against
  float64 <= 1.5 x torch's bf16 chain, cosine to fp32 > 0.999).  Measured:
  72x96x12 4.11e-03 against 8.38e-03, cosine 0.999995; 84x84x8 4.27e-03
  against 8.79e-03, 0.999992: the margin is no narrower than at 3 channels."""
  ws, bs = _params(shape)
  frames = _frames(6, shape, 41)
  ref64 = O.chain64(frames, ws, bs).reshape(6, -1)
  feats = []
  for dt in (F32, BF):
    ag = Agent(9, torso='shallow', frame_shape=shape, seed=5,
               compute_dtype=dt).to(cuda)
    with torch.no_grad():
      for sp, b in zip(ag.specs, bs):
        ag._conv_params(sp['name'])[1].copy_(b)
      feats.append(ag.conv_features(frames.to(cuda)))
  f32, tbf = feats
  out = _fwd(ops.ext(), frames.to(cuda), ws, bs).reshape(6, -1)
  scale = ref64.abs().max().item()
  err = lambda t: (t.double().cpu() - ref64).abs().max().item() / scale
  e_hip, e_torch, cos = err(out), err(tbf), _cos(out.cpu(), f32.cpu())
  print('shallow bf16w %s: err hip %.4e torch-bf16 %.4e cos(fp32) %.6f' %
        (shape, e_hip, e_torch, cos))
  assert tbf.dtype == BF and err(f32) < 1e-4 and cos > 0.999
  assert e_hip <= 1.5 * e_torch, (e_hip, e_torch)


def test_declines_and_forms(cuda):
  C = ops.ext()
  for shape, n, want in CASES:
    assert bool(C.shallow_bf16w_form(n, *shape)) == want, (shape, n)
  ws, bs = _params((72, 96, 12))
  wp = C.shallow_bf16w_pack(*[w.to(cuda) for w in ws])
  wp16 = C.shallow_bf16w_pack(*[w.to(cuda) for w in _params((72, 96, 16))[0]])
  b = [x.to(cuda) for x in bs]
  args = lambda p=wp: (p[0], b[0], p[1], b[1], p[2], b[2])
  z = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.uint8)
  # declined shapes, a 4-channel frame, then weights packed for Cp = 16
  for bad, p in ((z(2, 16, 16, 12), wp), (z(0, 72, 96, 12), wp),
                 (z(513, 72, 96, 12), wp), (z(2, 72, 96, 4), wp),
                 (z(2, 72, 96, 12), wp16)):
    with pytest.raises(RuntimeError):
      C.shallow_bf16w_fwd(bad, *args(p))
  assert C.shallow_bf16w_fwd(z(2, 72, 96, 12), *args()).shape == (2, 5, 6, 128)


def _step_logits(cuda, agent, B=12):
  from scalable_agent_amd.structs import StepOutput
  g = torch.Generator().manual_seed(8)
  frame = _frames(B, agent.frame_shape, 9).to(cuda)
  eo = StepOutput(torch.randn(B, generator=g).to(cuda), None,
                  (torch.rand(B, generator=g) < 0.3).to(cuda), (frame, None))
  last = torch.randint(0, 9, (B,), generator=g).to(cuda)
  state = (torch.randn(B, 256, generator=g).to(cuda),
           torch.randn(B, 256, generator=g).to(cuda))
  with torch.no_grad():
    out, _ = agent.step(last, eo, state,
                        generator=torch.Generator(cuda).manual_seed(0))
  return out.policy_logits


def test_agent_takes_the_wide_kernel(cuda):
  """No-grad features are the direct binding call's and follow a weight
  change through refresh_inference_cache; step logits meet
  test_shallow_bf16_infer_gpu's bar; under autograd the fp32 torso runs."""
  from scalable_agent_amd.ops.conv_f32 import shallow_param_list
  ops.load()
  C = ops.ext()
  mk = lambda dt, torso='shallow': Agent(
      9, torso=torso, frame_shape=(72, 96, 12), seed=1, backend='hip',
      compute_dtype=dt).to(cuda)
  bf = mk(BF)
  frames = _frames(7, (72, 96, 12), 4).to(cuda)

  def direct():
    p = [t.detach() for t in shallow_param_list(bf)]
    return _fwd(C, frames, p[0::2], p[1::2]).reshape(7, -1)

  with torch.no_grad():
    got = bf.conv_features(frames)
  assert C.conv_launch_info(FAMILY)['ntiles'] == 7
  assert got.dtype == BF and torch.equal(got, direct())
  bf.inference_cache()
  assert bf._inference_cache['wsh16'][0].numel() == 24 * 32 * 32
  with torch.no_grad():
    for t in shallow_param_list(bf):
      t.mul_(0.5).add_(0.01)
    bf.refresh_inference_cache()
    after = bf.conv_features(frames)
  assert torch.equal(after, direct()) and not torch.equal(after, got)
  with_grad = bf.conv_features(frames)
  assert with_grad.dtype == F32 and with_grad.requires_grad
  cos = [_cos(_step_logits(cuda, mk(BF, t)), _step_logits(cuda, mk(F32, t)))
         for t in ('shallow', 'deep')]
  print('step-logit cosine at 72x96x12: shallow %.6f deep %.6f' % tuple(cos))
  assert cos[0] >= cos[1] - 0.01
