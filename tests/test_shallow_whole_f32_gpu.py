"""The one-launch shallow conv torso for actor inference (csrc/kernels/
conv_f32.hip shallow_torso_kernel): cf32_shallow_fwd computes x / 255 and the
three TF-SAME convs (8x8/4, 4x4/2, 3x3/2; bias + ReLU each) of uint8 frames
with one workgroup per image, every intermediate in LDS.

It must be BITWISE the launches it replaces (cf32_frames_f32 + three
cf32_conv_fwd(relu_out=True) with w1 zero-padded to the image's 4 channels),
also when a workgroup walks several images (grid cap), with no image leaking
into the next one.  An exact integer case is held to a float64 F.conv2d chain
with explicit pads, independent of the ops kernels: every partial sum is an
integer below 2^24, so fp32 is exact whatever the summation order, and any
misplaced pad or tap shows as a wrong integer.
"""

import pytest
import torch
import torch.nn.functional as F

from scalable_agent_amd.models import Agent

pytestmark = pytest.mark.gpu

FRAMES = [(72, 96, 3), (84, 84, 4), (72, 128, 3), (72, 96, 1)]
LAYERS = ((8, 4), (4, 2), (3, 2))  # (kernel, stride)


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _pads(n, k, s):
  """TF SAME: (output size, pad before, pad after)."""
  out = -(-n // s)
  total = max((out - 1) * s + k - n, 0)
  return out, total // 2, total - total // 2


def test_pads_are_the_asymmetric_ones():
  assert _pads(21, 4, 2) == (11, 1, 2)   # 84x84: layer 2
  assert _pads(12, 3, 2) == (6, 0, 1)    # 72x96: layer 3, W
  assert _pads(16, 3, 2) == (8, 0, 1)    # 72x128: layer 3, W
  assert _pads(9, 3, 2) == (5, 1, 1)
  assert _pads(72, 8, 4) == (18, 2, 2)


_PARAMS = {}


def _params(dev, shape):
  """The agent's own initialisation of the conv weights (HWIO, w1 unpadded),
  with non-zero biases (the initialiser's are zero).  Made once per shape."""
  if shape not in _PARAMS:
    ag = Agent(9, torso='shallow', frame_shape=shape, seed=5)
    g = torch.Generator().manual_seed(6)
    out = []
    for sp in ag.specs:
      w, b = ag._conv_params(sp['name'])
      out += [w.detach().clone().to(dev),
              (torch.randn(b.shape, generator=g) * 0.1).to(dev)]
    assert [tuple(t.shape) for t in out[::2]] == [
        (8, 8, shape[2], 32), (4, 4, 32, 64), (3, 3, 64, 128)]
    _PARAMS[shape] = out
  return _PARAMS[shape]


def _frames(dev, n, shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8).to(dev)


def _ops_chain(C, frames, params):
  """What _ShallowTorsoF32.forward launches."""
  x = C.cf32_frames_f32(frames)
  for i, (k, s) in enumerate(LAYERS):
    w, b = params[2 * i], params[2 * i + 1]
    if i == 0 and w.shape[2] != 4:
      z = torch.zeros(8, 8, 4 - w.shape[2], 32, device=w.device)
      w = torch.cat([w, z], dim=2).contiguous()
    Ho, pt, _ = _pads(x.shape[1], k, s)
    Wo, pl, _ = _pads(x.shape[2], k, s)
    x = C.cf32_conv_fwd(x, w, b, s, pt, pl, Ho, Wo, relu_out=True)
  return x


_REF = {}


def _case(cuda, shape, N):
  key = (shape, N)
  if key not in _REF:
    frames = _frames(cuda, N, shape, 11 + N)
    _REF[key] = (frames, _ops_chain(_C(), frames, _params(cuda, shape)))
  return _REF[key]


@pytest.mark.parametrize('cap', [0, 2])
@pytest.mark.parametrize('N', [1, 2, 5])
@pytest.mark.parametrize('shape', FRAMES)
def test_bitwise_the_ops_chain(cuda, shape, N, cap):
  """Uncapped: one workgroup per image.  Capped at 2: at N = 5 a workgroup
  walks images 0, 2, 4 - the next image's staging follows the previous
  image's layer 3 in the same LDS."""
  C = _C()
  frames, ref = _case(cuda, shape, N)
  old = C.cf32_grid_cap(cap)
  try:
    C.cf32_launch_info(True)
    out = C.cf32_shallow_fwd(frames, *_params(cuda, shape))
    info = C.cf32_launch_info(True)
  finally:
    C.cf32_grid_cap(old)
  assert info['family'] == 'shallow_whole'
  assert info['grid_x'] == (min(N, cap) if cap else N) and info['grid_y'] == 1
  assert info['ntiles'] == N
  assert out.shape == ref.shape and out.dtype == torch.float32
  assert ref.abs().max().item() > 0
  assert torch.equal(out, ref)


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_images_are_independent(cuda, shape):
  """N = 5 under a cap of 2: image 0 all zeros and image 4 all 255 (the
  first and the last image of one workgroup's walk) give the rows they give
  alone."""
  C = _C()
  p = _params(cuda, shape)
  frames = _frames(cuda, 5, shape, 21).clone()
  frames[0] = 0
  frames[4] = 255
  old = C.cf32_grid_cap(2)
  try:
    out = C.cf32_shallow_fwd(frames, *p)
  finally:
    C.cf32_grid_cap(old)
  for i in (0, 4):
    alone = C.cf32_shallow_fwd(frames[i:i + 1].contiguous(), *p)
    assert torch.equal(out[i:i + 1], alone), i
  assert not torch.equal(out[0], out[4])


@pytest.mark.parametrize('shape', [(84, 84, 4), (72, 96, 3)])
def test_exact_integers_against_float64(cuda, shape):
  """Frame bytes in {0, 255} (x / 255 exactly 0 or 1), integer biases, w1 in
  {-1, 0, 1}, w2 and w3 in {-1, 0, 1} with 1/8 of the entries non-zero: with
  bound_l = max_cout sum|w_l| * bound_{l-1} + max|b_l| below 2^24 every
  partial sum is an integer fp32 holds exactly, so the result equals a
  float64 conv chain with explicit TF-SAME pads (84x84x4 and 72x96x3 use
  every asymmetric pad: 1/2 for 4x4/2 on 21, 0/1 for 3x3/2 on 12)."""
  C = _C()
  g = torch.Generator().manual_seed(31)
  c = shape[2]
  frames = (torch.randint(0, 2, (3,) + shape, generator=g) * 255).to(torch.uint8)

  def sparse(shp, keep):
    sign = torch.randint(0, 2, shp, generator=g) * 2 - 1
    on = torch.randint(0, keep, shp, generator=g) == 0
    return (sign * on).to(torch.float32)

  ws = [torch.randint(-1, 2, (8, 8, c, 32), generator=g).to(torch.float32),
        sparse((4, 4, 32, 64), 8), sparse((3, 3, 64, 128), 8)]
  bs = [torch.randint(-3, 4, (n,), generator=g).to(torch.float32)
        for n in (32, 64, 128)]
  bound = 1.0
  for w, b in zip(ws, bs):
    bound = w.abs().sum(dim=(0, 1, 2)).max().item() * bound + b.abs().max().item()
  print('exact-integer bound_3 = %.3e' % bound)
  assert bound < 2 ** 24

  x = (frames.double() / 255.0).permute(0, 3, 1, 2)
  assert set(x.unique().tolist()) == {0.0, 1.0}
  for (k, s), w, b in zip(LAYERS, ws, bs):
    _, pt, pb = _pads(x.shape[2], k, s)
    _, pl, pr = _pads(x.shape[3], k, s)
    x = F.relu(F.conv2d(F.pad(x, (pl, pr, pt, pb)),
                        w.double().permute(3, 2, 0, 1), b.double(), stride=s))
  ref = x.permute(0, 2, 3, 1).contiguous()
  assert ref.abs().max().item() > 0 and torch.equal(ref, ref.round())

  args = []
  for w, b in zip(ws, bs):
    args += [w.to(cuda), b.to(cuda)]
  out = C.cf32_shallow_fwd(frames.to(cuda), *args)
  assert torch.equal(out.double().cpu(), ref)


def test_declines(cuda):
  C = _C()
  p = _params(cuda, (72, 96, 3))
  assert C.cf32_shallow_form(5, 16, 16, 3) == 0
  with pytest.raises(RuntimeError):
    C.cf32_shallow_fwd(torch.zeros(5, 16, 16, 3, dtype=torch.uint8, device=cuda), *p)
  with pytest.raises(RuntimeError):
    C.cf32_shallow_fwd(torch.zeros(2, 72, 96, 3, device=cuda), *p)
  assert C.cf32_shallow_form(5, 72, 96, 3) == 1
