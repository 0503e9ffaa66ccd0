"""cf32_shallow_wide_fwd (conv_f32.hip shallow_wide_kernel), the one-launch
fp32 shallow torso on 5-16 channel frames: bitwise the no-grad 'ops' forward
at both edges of every Cp, an exact integer case against a float64 conv
chain, the public path.  72x128 frames run at C 9..12 only: at Cp = 8 and 16
the ops launches have no layer-1 tile (cf32_conv_fwd raises)."""
import functools
import pytest
import torch
import torch.nn.functional as F

from scalable_agent_amd.models import Agent
from scalable_agent_amd.ops import conv_f32, ext

pytestmark = pytest.mark.gpu

SIZES = [(72, 96), (84, 84), (72, 128)]
CHANNELS = {hw: (9, 12) if hw == (72, 128) else (5, 8, 9, 12, 13, 16)
            for hw in SIZES}


@functools.lru_cache(maxsize=None)
def _agent(cuda, shape, blocks='ops'):
  """A same-seed fp32 HIP shallow agent with non-zero biases, made once."""
  ag = Agent(9, torso='shallow', frame_shape=shape, seed=3, backend='hip',
             compute_dtype=torch.float32, torso_blocks=blocks).to(cuda)
  g = torch.Generator().manual_seed(4)
  with torch.no_grad():
    for name, p in ag.convnet.items():
      if name.endswith('__b'):
        p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(cuda))
  return ag


def _frames(cuda, n, shape, seed):  # random frames inside a buffer of 255s
  numel = n * shape[0] * shape[1] * shape[2]
  buf = torch.full((64 + numel + 64,), 255, dtype=torch.uint8)
  buf[64:64 + numel] = torch.randint(
      0, 256, (numel,), generator=torch.Generator().manual_seed(seed),
      dtype=torch.uint8)
  return buf.to(cuda)[64:64 + numel].view((n,) + tuple(shape))


def _family_of(fn):
  ext().cf32_launch_info(True)
  out = fn()
  return out, ext().cf32_launch_info(True)


@pytest.mark.parametrize(
    'shape,N,cap',
    [(hw + (c,), n, 0) for hw in SIZES for c in CHANNELS[hw] for n in (1, 3)] +
    [(hw + (12,), 5, 2) for hw in SIZES])  # cap 2: a workgroup walks 0, 2, 4
def test_bitwise_the_ops_forward(cuda, shape, N, cap):
  ag = _agent(cuda, shape)
  frames = _frames(cuda, N, shape, 11 + N)
  with torch.no_grad():
    ref = ag.conv_features(frames)
    old = ext().cf32_grid_cap(cap)
    try:
      out, info = _family_of(lambda: ext().cf32_shallow_wide_fwd(
          frames, *conv_f32.shallow_param_list(ag)))
    finally:
      ext().cf32_grid_cap(old)
  assert info['family'] == 'shallow_whole_wide'
  assert info['grid_x'] == (min(N, cap) if cap else N) and info['ntiles'] == N
  assert ref.abs().max().item() > 0 and torch.equal(out.reshape(N, -1), ref)


def _pads(n, k, s):  # TF SAME: (pad before, pad after)
  total = max((-(-n // s) - 1) * s + k - n, 0)
  return total // 2, total - total // 2


@pytest.mark.parametrize('hw,c', [(hw, c) for hw in SIZES
                                  for c in (12, CHANNELS[hw][0])])
def test_exact_integers_against_float64(cuda, hw, c):
  """Bytes in {0, 255}, weights in {-1, 0, 1} (1/2, 1/8, 1/8 non-zero),
  integer biases: bound_l = max_cout sum|w_l| * bound_{l-1} + max|b_l|."""
  g = torch.Generator().manual_seed(31)
  frames = (torch.randint(0, 2, (3,) + hw + (c,), generator=g) * 255).to(torch.uint8)
  # every row its own pattern: a wrong band seam or halo row changes the sums
  assert len(torch.unique(frames.reshape(3 * hw[0], -1), dim=0)) == 3 * hw[0]
  def sparse(shp, keep):
    sign = torch.randint(0, 2, shp, generator=g) * 2 - 1
    return (sign * (torch.randint(0, keep, shp, generator=g) == 0)).float()
  ws = [sparse((8, 8, c, 32), 2), sparse((4, 4, 32, 64), 8), sparse((3, 3, 64, 128), 8)]
  bs = [torch.randint(-3, 4, (n,), generator=g).float() for n in (32, 64, 128)]
  bound = 1.0
  for w, b in zip(ws, bs):
    bound = w.abs().sum(dim=(0, 1, 2)).max().item() * bound + b.abs().max().item()
  assert bound < 2 ** 24
  x = (frames.double() / 255.0).permute(0, 3, 1, 2)
  for (k, s), w, b in zip(((8, 4), (4, 2), (3, 2)), ws, bs):
    pads = _pads(x.shape[3], k, s) + _pads(x.shape[2], k, s)
    x = F.relu(F.conv2d(F.pad(x, pads), w.double().permute(3, 2, 0, 1),
                        b.double(), stride=s))
  ref = x.permute(0, 2, 3, 1).contiguous()
  assert ref.abs().max().item() > 0
  out = ext().cf32_shallow_wide_fwd(
      frames.to(cuda), *[t.to(cuda) for pair in zip(ws, bs) for t in pair])
  assert torch.equal(out.double().cpu(), ref)


def test_public_path(cuda):
  shape = (72, 96, 12)
  whole, plain = _agent(cuda, shape, 'whole'), _agent(cuda, shape)
  assert whole.torso_whole_form() == 'shallow_wide' == conv_f32.whole_wide_form(shape)
  frames, many = _frames(cuda, 3, shape, 5), _frames(cuda, 513, shape, 6)
  with torch.no_grad():
    a, info = _family_of(lambda: whole.conv_features(frames))
    b = plain.conv_features(frames)
    c, info_many = _family_of(lambda: whole.conv_features(many))
    d = plain.conv_features(many)
  assert info['family'] == 'shallow_whole_wide' and torch.equal(a, b)
  assert info_many['family'] == 'conv_fwd' and torch.equal(c, d)
  with torch.enable_grad():
    e, info_grad = _family_of(lambda: whole.conv_features(frames))
  assert info_grad['family'] == 'conv_fwd' and torch.equal(e.detach(), b)


@pytest.mark.parametrize('shape', [(72, 96, 4), (72, 96, 17), (64, 64, 12),
                                   (72, 128, 8), (72, 128, 13)])
def test_declines(cuda, shape):
  assert ext().cf32_shallow_wide_form(2, *shape) == 0
  p = conv_f32.shallow_param_list(_agent(cuda, (72, 96, 12)))
  w1 = torch.zeros(8, 8, shape[2], 32, device=cuda)
  with pytest.raises(RuntimeError):
    ext().cf32_shallow_wide_fwd(
        torch.zeros((2,) + shape, dtype=torch.uint8, device=cuda), w1, *p[1:])
