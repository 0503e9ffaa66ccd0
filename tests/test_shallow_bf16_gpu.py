"""The one-launch bf16 MFMA shallow torso for actor inference (csrc/kernels/
conv_shallow_bf16.hip): shallow_bf16_fwd computes x / 255 and the three
TF-SAME convs (8x8/4, 4x4/2, 3x3/2; bias + ReLU each) of uint8 frames with
one workgroup per image, bf16 maps in LDS, fp32 accumulation.

An exact integer case (every stored value an integer <= 256, which bf16
holds) must EQUAL a float64 conv chain with explicit pads: a misplaced pad,
tap, channel pad, partial pixel tile or pack index shows as a wrong integer.
The grid walk (capped grid) must be bitwise the uncapped launch with no image
leaking into the next.  On realistic weights the error against the float64
oracle is held to 1.5 x that of torch's own bf16 chain on the same GPU.
"""

import pytest
import torch

from scalable_agent_amd.models import Agent

from . import _shallow_bf16_oracle as O

pytestmark = pytest.mark.gpu

FAMILY = 'shallow_bf16'
CAP_KEY = 'shallow_bf16_grid'


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _fwd(C, frames, ws, bs):
  dev = frames.device
  wp = C.shallow_bf16_pack(*[w.to(dev) for w in ws])
  b = [x.to(dev) for x in bs]
  return C.shallow_bf16_fwd(frames, wp[0], b[0], wp[1], b[1], wp[2], b[2])


class _cap(object):
  def __init__(self, C, cap):
    self.C, self.cap = C, cap

  def __enter__(self):
    self.old = self.C.conv_tune(CAP_KEY, self.cap)
    assert self.old >= 0

  def __exit__(self, *a):
    self.C.conv_tune(CAP_KEY, self.old)
    return False


# ------------------------------------------------------------ exact integers
def test_integer_taps_cover_every_tap():
  for c in (1, 3, 4):
    seen = None
    for phase in range(3):
      ws, _ = O.integer_weights(c, phase)
      nz = [(w != 0).any(dim=3) for w in ws]
      seen = nz if seen is None else [a | b for a, b in zip(seen, nz)]
    assert all(bool(s.all()) for s in seen), c


@pytest.mark.parametrize('phase', [0, 1, 2])
@pytest.mark.parametrize('shape', O.FRAMES)
def test_exact_integers_against_float64(cuda, shape, phase):
  """Frame bytes in {0, 255}, NNZ = (3, 6, 9) taps of +-1 per output channel,
  integer biases in [0, (1, 2, 8)]: the running bound is (4, 26, 242) <= 256,
  so the frame, both LDS maps and the features are integers bf16 holds
  exactly and the result equals the float64 chain."""
  C = _C()
  ws, bs = O.integer_weights(shape[2], phase)
  bounds = O.running_bounds(ws, bs)
  assert all(b <= want <= 256 for b, want in zip(bounds, O.BOUNDS)), bounds
  frames = O.binary_frames(shape, 3)
  ref = O.chain64(frames, ws, bs)
  assert torch.equal(ref, ref.round()) and ref.max().item() <= 256
  assert (ref != 0).double().mean().item() > 0.5
  out = _fwd(C, frames.to(cuda), ws, bs)
  assert out.dtype == torch.bfloat16
  assert tuple(out.shape) == (3,) + O.out_shape(shape)
  assert torch.equal(out.double().cpu(), ref)


# --------------------------------------------------- grid walk, independence
_PARAMS = {}


def _params(shape):
  """The agent's own initialisation of the conv weights with non-zero biases
  (the initialiser's are zero); CPU, made once per shape."""
  if shape not in _PARAMS:
    ag = Agent(9, torso='shallow', frame_shape=shape, seed=5)
    g = torch.Generator().manual_seed(6)
    ws, bs = [], []
    for sp in ag.specs:
      w, b = ag._conv_params(sp['name'])
      ws.append(w.detach().clone())
      bs.append(torch.randn(b.shape, generator=g) * 0.1)
    _PARAMS[shape] = (ws, bs)
  return _PARAMS[shape]


def _frames(n, shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8)


@pytest.mark.parametrize('N', [1, 2, 5])
@pytest.mark.parametrize('shape', O.FRAMES)
def test_capped_grid_is_bitwise_the_uncapped(cuda, shape, N):
  """Capped at 2: at N = 5 a workgroup walks images 0, 2, 4 - the next
  image's staging follows the previous image's layer 3 in the same LDS."""
  C = _C()
  ws, bs = _params(shape)
  frames = _frames(N, shape, 11 + N).to(cuda)
  outs = []
  for cap in (0, 2):
    with _cap(C, cap):
      out = _fwd(C, frames, ws, bs)
      info = C.conv_launch_info(FAMILY)
      last = C.conv_launch_info()
    assert info['family'] == FAMILY and last['family'] == FAMILY
    assert info['grid'] == (min(N, cap) if cap else N)
    assert info['ntiles'] == N
    outs.append(out)
  again = _fwd(C, frames, ws, bs)
  assert outs[0].float().abs().max().item() > 0
  assert torch.equal(outs[0], outs[1])
  assert torch.equal(outs[0], again)  # deterministic


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_images_are_independent(cuda, shape):
  """N = 5 under a cap of 2: image 0 all zeros and image 4 all 255 (the
  first and the last image of one workgroup's walk) give the rows they give
  alone."""
  C = _C()
  ws, bs = _params(shape)
  frames = _frames(5, shape, 21).clone()
  frames[0] = 0
  frames[4] = 255
  frames = frames.to(cuda)
  with _cap(C, 2):
    out = _fwd(C, frames, ws, bs)
  for i in (0, 4):
    alone = _fwd(C, frames[i:i + 1].contiguous(), ws, bs)
    assert torch.equal(out[i:i + 1], alone), i
  assert not torch.equal(out[0], out[4])


# ---------------------------------------------------------- realistic weights
def _cos(a, b):
  a, b = a.double().flatten(), b.double().flatten()
  return (a @ b / (a.norm() * b.norm())).item()


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_realistic_weights_track_the_oracle(cuda, shape):
  """Error in test_conv_gpu.close's metric (max |err| / max |ref|) against the
  float64 chain: at most 1.5 x that of torch's own bf16 chain (torch backend,
  compute_dtype=bf16, same GPU), which rounds the same five kinds of value
  (weights, x / 255, two maps, the features); 1.5 covers where the rounding
  points differ.  Cosine to the fp32 torch features > 0.999, the bar of
  test_deep_torso_matches_fp32_reference."""
  C = _C()
  ws, bs = _params(shape)
  frames = _frames(6, shape, 41)
  ref64 = O.chain64(frames, ws, bs).reshape(6, -1)
  mk = lambda dt: Agent(9, torso='shallow', frame_shape=shape, seed=5,
                        compute_dtype=dt).to(cuda)
  agents = [mk(torch.float32), mk(torch.bfloat16)]
  for ag in agents:
    with torch.no_grad():
      for sp, b in zip(ag.specs, bs):
        ag._conv_params(sp['name'])[1].copy_(b)
  with torch.no_grad():
    f32, tbf = [ag.conv_features(frames.to(cuda)) for ag in agents]
  out = _fwd(C, frames.to(cuda), ws, bs).reshape(6, -1)
  assert tbf.dtype == torch.bfloat16
  scale = ref64.abs().max().item()
  err = lambda t: (t.double().cpu() - ref64).abs().max().item() / scale
  e_hip, e_torch = err(out), err(tbf)
  cos = _cos(out.cpu(), f32.cpu())
  print('shallow bf16 %s: err hip %.4e torch-bf16 %.4e (max|ref| %.4g) '
        'cos(fp32) %.6f' % ('x'.join(map(str, shape)), e_hip, e_torch, scale,
                            cos))
  assert err(f32) < 1e-4  # the oracle and the fp32 torch chain agree
  assert cos > 0.999
  assert e_hip <= 1.5 * e_torch, (e_hip, e_torch)


# -------------------------------------------------------------------- declines
def test_declines(cuda):
  C = _C()
  ws, bs = _params((72, 96, 3))
  wp = C.shallow_bf16_pack(*[w.to(cuda) for w in ws])
  b = [x.to(cuda) for x in bs]
  args = lambda p=wp: (p[0], b[0], p[1], b[1], p[2], b[2])
  z = lambda *s, **kw: torch.zeros(*s, device=cuda,
                                   dtype=kw.get('dtype', torch.uint8))
  assert C.shallow_bf16_form(5, 72, 96, 3) == 1
  assert C.shallow_bf16_form(5, 16, 16, 3) == 0
  assert C.shallow_bf16_form(0, 72, 96, 3) == 0
  assert C.shallow_bf16_form(513, 72, 96, 3) == 0
  assert C.shallow_bf16_form(5, 72, 96, 5) == 0
  for bad in (z(5, 16, 16, 3), z(0, 72, 96, 3), z(513, 72, 96, 3),
              z(2, 72, 96, 5), z(2, 72, 96, 3, dtype=torch.float32)):
    with pytest.raises(RuntimeError):
      C.shallow_bf16_fwd(bad, *args())
  for i in range(3):
    short = list(wp)
    short[i] = wp[i][:-8].contiguous()
    with pytest.raises(RuntimeError):
      C.shallow_bf16_fwd(z(2, 72, 96, 3), *args(short))
  assert C.shallow_bf16_fwd(z(2, 72, 96, 3), *args()).shape == (2, 5, 6, 128)
