"""The fused fp32 residual block (csrc/kernels/conv_wino.hip
wino_res_block_kernel, cf32_res_block_fwd): one launch computes
t = relu(conv1(relu(x)) + b1), y = conv2(t) + b2 + x [relu], t only in LDS.

It must be BITWISE the two-launch form it replaces in actor inference
(cf32_conv_fwd(relu_in, relu_out) then cf32_conv_fwd(add=x, relu_out=last)) on
every map of the three frame ladders, across every band seam, with the
zero padding of t (not conv1 of padded x) at the image border; it declines
where the two-launch form would leave the Winograd forward; the whole fp32
torso with Agent(torso_blocks='fused') equals the 'ops' torso bitwise, eagerly
and in a captured graph.  One case is also held to a float64 oracle with the
project's parity rule, max(2e-5, 1.5 x the two-launch form's own error), so a
mistake shared by both forms would still show.
"""

import pytest
import torch

from scalable_agent_amd.models import Agent, layers

pytestmark = pytest.mark.gpu

# (C, H, W): the residual maps of the 72x96, 84x84 and 72x128 frames
MAPS = [(16, 36, 48), (32, 18, 24), (32, 9, 12),
        (16, 42, 42), (32, 21, 21), (32, 11, 11),
        (16, 36, 64), (32, 18, 32), (32, 9, 16)]


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _case(dev, N, C, H, W, seed=0, b1=None):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(N, H, W, C, generator=g)  # negative entries: both ReLUs act
  w1 = torch.randn(3, 3, C, C, generator=g) * 0.2
  w2 = torch.randn(3, 3, C, C, generator=g) * 0.2
  bias1 = torch.randn(C, generator=g) * 0.1
  bias2 = torch.randn(C, generator=g) * 0.1
  if b1 is not None:
    bias1 = torch.full((C,), float(b1))
  return [t.to(dev) for t in (x, w1, bias1, w2, bias2)]


def _two_launch(C, x, w1, b1, w2, b2, last):
  H, W = x.shape[1], x.shape[2]
  t = C.cf32_conv_fwd(x, w1, b1, 1, 1, 1, H, W, relu_in=True, relu_out=True)
  return C.cf32_conv_fwd(t, w2, b2, 1, 1, 1, H, W, add=x, relu_out=last)


def _fused(C, x, w1, b1, w2, b2, last):
  out = C.cf32_res_block_fwd(x, w1, b1, w2, b2, last)
  assert out, 'the fused block declined %r' % (tuple(x.shape),)
  return out[0]


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('C_,H,W', MAPS)
def test_block_is_bitwise_the_two_launches(cuda, C_, H, W, last):
  C = _C()
  args = _case(cuda, 3, C_, H, W, seed=H * W + C_)
  y = _fused(C, *args, last)
  ref = _two_launch(C, *args, last)
  assert y.shape == ref.shape and y.dtype == torch.float32
  assert torch.equal(y, ref)
  if last:
    assert float(y.min()) >= 0.0
  else:
    assert float(y.min()) < 0.0  # the residual operand is the un-ReLU'd x


@pytest.mark.parametrize('N', [77, 90])
def test_grid_beyond_one_wave_of_workgroups(cuda, N):
  """A board's worth of images.  With 12-row bands 77 images are 231
  workgroups, just under the 256 CUs; 90 images (270) need a second wave."""
  C = _C()
  args = _case(cuda, N, 16, 36, 48, seed=5)
  bands = -(-36 // C.cf32_res_block_band(16, 48))
  assert N < 90 or N * bands > 256  # more workgroups than CUs
  assert torch.equal(_fused(C, *args, False), _two_launch(C, *args, False))


@pytest.mark.parametrize('C_,H,W', [(16, 42, 42), (32, 9, 12), (32, 18, 32)])
def test_t_outside_the_image_is_zero_not_relu_b1(cuda, C_, H, W):
  """b1 = +1: conv1 applied to the zero padding would give t = relu(b1) = 1
  around the image (and in the row / column an odd map's last tiles overhang)
  and change y's border; conv2's SAME padding pads t with zeros."""
  C = _C()
  args = _case(cuda, 3, C_, H, W, seed=9, b1=1.0)
  for last in (False, True):
    assert torch.equal(_fused(C, *args, last), _two_launch(C, *args, last))


def test_every_instance_crosses_a_band_seam(cuda):
  """Per (channels, band height) instance one of MAPS has a height that is no
  multiple of the band: its last band is partial and every seam between bands
  (t halo rows recomputed by both neighbours) lies inside a compared map."""
  C = _C()
  seen = {}
  for C_, H, W in MAPS:
    R = C.cf32_res_block_band(C_, W)
    assert R > 0 and R % 2 == 0, (C_, H, W, R)
    seen.setdefault((C_, R), []).append(H)
  assert {c for c, _ in seen} == {16, 32}
  for (C_, R), heights in seen.items():
    assert any(h % R != 0 and h > R for h in heights), (C_, R, heights)
  assert C.cf32_res_block_band(16, 4096) == 0  # no band fits the LDS
  assert C.cf32_res_block_band(64, 24) == 0    # no such instance


def test_declined_shapes_return_empty(cuda):
  C = _C()
  # 5x7: 12 tiles per image, a 64-tile range of the two-launch form would
  # span more images than its stager handles, so it runs the direct kernel
  assert C.cf32_res_block_fwd(*_case(cuda, 3, 32, 5, 7), False) == []
  # above the inference bound
  assert C.cf32_res_block_fwd(*_case(cuda, 513, 32, 9, 12), False) == []
  # no instance for the channel count
  g = torch.Generator().manual_seed(0)
  x = torch.randn(2, 9, 12, 64, generator=g).to(cuda)
  w = torch.randn(3, 3, 64, 64, generator=g).to(cuda)
  b = torch.zeros(64, device=cuda)
  assert C.cf32_res_block_fwd(x, w, b, w, b, False) == []


def _agent(cuda, shape, blocks, seed=3):
  ag = Agent(9, torso='deep', frame_shape=shape, seed=seed, backend='hip',
             compute_dtype=torch.float32, torso_blocks=blocks).to(cuda)
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


def test_declined_map_in_the_torso_matches_the_two_launch_path(cuda):
  """A 20x28 frame: the last stage's map is 5x7, whose blocks the fused kernel
  declines; torso_forward_f32 runs the two launches there."""
  from scalable_agent_amd import ops
  shape = (20, 28, 3)
  fused, plain = _agent(cuda, shape, 'fused'), _agent(cuda, shape, 'ops')
  frames = _frames(cuda, 5, shape, 2)
  with torch.no_grad():
    a = ops.torso_forward_f32(fused, frames)
    b = ops.torso_forward_f32(plain, frames)
  assert torch.equal(a, b)


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_whole_torso(cuda, shape):
  fused, plain = _agent(cuda, shape, 'fused'), _agent(cuda, shape, 'ops')
  assert fused.torso_blocks_fused() and not plain.torso_blocks_fused()
  frames = _frames(cuda, 37, shape, 4)
  with torch.no_grad():
    feats = fused.conv_features(frames)
    feats_ops = plain.conv_features(frames)
  with torch.enable_grad():
    feats_grad = fused.conv_features(frames)
  assert feats_grad.requires_grad and not feats.requires_grad
  assert torch.equal(feats, feats_grad.detach())
  assert torch.equal(feats, feats_ops)


def test_graph_replay_matches_eager(cuda):
  shape = (72, 96, 3)
  ag = _agent(cuda, shape, 'fused')
  batches = [_frames(cuda, 37, shape, 10 + k) for k in range(3)]
  with torch.no_grad():
    eager = [ag.conv_features(f).clone() for f in batches]
  assert not torch.equal(eager[1], eager[2])
  buf = batches[0].clone()
  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side), torch.no_grad():
    ag.conv_features(buf)  # warm-up
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      out = ag.conv_features(buf)
    for k in (1, 2):
      buf.copy_(batches[k])
      g.replay()
      side.synchronize()
      assert torch.equal(out, eager[k]), k


def test_float64_oracle(cuda):
  """(32, 9, 12), last: against a float64 conv reference on the CPU the fused
  block's max-abs error is <= max(2e-5, 1.5 x the two-launch form's)."""
  C = _C()
  args = _case(cuda, 3, 32, 9, 12, seed=21)
  x, w1, b1, w2, b2 = [a.double().cpu() for a in args]
  t = layers.conv2d_same_nhwc(x.clamp(min=0), w1, b1, 1).clamp(min=0)
  ref = (layers.conv2d_same_nhwc(t, w2, b2, 1) + x).clamp(min=0)
  err = lambda y: (y.double().cpu() - ref).abs().max().item()
  e_two = err(_two_launch(C, *args, True))
  e_fused = err(_fused(C, *args, True))
  print('float64 oracle: fused %.3e, two launches %.3e (output scale %.2f)' %
        (e_fused, e_two, ref.abs().max().item()))
  assert e_fused <= max(2e-5, 1.5 * e_two)
