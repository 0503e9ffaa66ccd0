"""The one-launch last stage of the fp32 inference torso (csrc/kernels/
conv_wino.hip wino_stage_tail_kernel): cf32_stage_tail_fwd runs both residual
blocks of a 32-channel stage whose whole map fits one workgroup's LDS,
cf32_stage_fwd also the stage head (conv + bias + 3x3/2 max-pool) at 18x24.

Both must be BITWISE the launches they replace (two cf32_res_block_fwd, i.e.
four cf32_conv_fwd, after cf32_wino_conv_pool_fwd), with zeros (not relu(b1))
around t and in the row / column an odd map's last tiles overhang; they
decline where a replaced launch would not be the Winograd one; the whole fp32
torso with Agent(torso_blocks='stage') equals 'ops' and 'fused' bitwise,
eagerly and in a captured graph.  The whole-stage kernel is also held to a
float64 oracle with the project's parity rule, max(2e-5, 1.5 x the ops
path's own error), so a mistake shared by every form would still show.
"""

import pytest
import torch
import torch.nn.functional as F

from scalable_agent_amd.models import Agent, layers

pytestmark = pytest.mark.gpu

# the last residual maps of the 72x96, 84x84 and 72x128 frames
MAPS = [(9, 12), (11, 11), (9, 16)]
CH = 32


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _case(dev, N, H, W, seed=0, b1=None, C=CH):
  """x with negative entries (every ReLU acts), then (w, b) of conv1a, conv2a,
  conv1b, conv2b, biases non-zero."""
  g = torch.Generator().manual_seed(seed)
  out = [torch.randn(N, H, W, C, generator=g)]
  for k in range(4):
    out.append(torch.randn(3, 3, C, C, generator=g) * 0.2)
    bias = torch.randn(C, generator=g) * 0.1
    if b1 is not None and k % 2 == 0:
      bias = torch.full((C,), float(b1))
    out.append(bias)
  return [t.to(dev) for t in out]


def _four_convs(C, x, w1a, b1a, w2a, b2a, w1b, b1b, w2b, b2b, last):
  H, W = x.shape[1], x.shape[2]
  t = C.cf32_conv_fwd(x, w1a, b1a, 1, 1, 1, H, W, relu_in=True, relu_out=True)
  x1 = C.cf32_conv_fwd(t, w2a, b2a, 1, 1, 1, H, W, add=x, relu_out=False)
  t = C.cf32_conv_fwd(x1, w1b, b1b, 1, 1, 1, H, W, relu_in=True, relu_out=True)
  return C.cf32_conv_fwd(t, w2b, b2b, 1, 1, 1, H, W, add=x1, relu_out=last)


def _two_blocks(C, x, w1a, b1a, w2a, b2a, w1b, b1b, w2b, b2b, last):
  x1 = C.cf32_res_block_fwd(x, w1a, b1a, w2a, b2a, False)
  assert x1, 'the fused block declined %r' % (tuple(x.shape),)
  y = C.cf32_res_block_fwd(x1[0], w1b, b1b, w2b, b2b, last)
  assert y
  return y[0]


def _tail(C, args, last):
  out = C.cf32_stage_tail_fwd(*args, last)
  assert out, 'the stage tail declined %r' % (tuple(args[0].shape),)
  return out[0]


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('H,W', MAPS)
def test_tail_is_bitwise_the_launches_it_replaces(cuda, H, W, last):
  C = _C()
  args = _case(cuda, 3, H, W, seed=H * W)
  y = _tail(C, args, last)
  assert y.shape == args[0].shape and y.dtype == torch.float32
  assert torch.equal(y, _two_blocks(C, *args, last))
  assert torch.equal(y, _four_convs(C, *args, last))
  if last:
    assert float(y.min()) >= 0.0
  else:
    assert float(y.min()) < 0.0  # the residual operand is the un-ReLU'd x'


@pytest.mark.parametrize('H,W', [(11, 11), (9, 12)])
def test_t_outside_the_image_is_zero_not_relu_b1(cuda, H, W):
  """b1a = b1b = +1: conv1 applied to the zero padding would give t =
  relu(b1) = 1 around the image and in the row / column the last tiles of an
  odd map overhang, and change y's border; conv2's SAME padding pads t with
  zeros."""
  C = _C()
  args = _case(cuda, 3, H, W, seed=9, b1=1.0)
  for last in (False, True):
    y = _tail(C, args, last)
    assert torch.equal(y, _two_blocks(C, *args, last))
    assert torch.equal(y, _four_convs(C, *args, last))


def _stage_case(dev, N, seed):
  g = torch.Generator().manual_seed(seed)
  x_in = torch.randn(N, 18, 24, CH, generator=g).to(dev)
  wh = (torch.randn(3, 3, CH, CH, generator=g) * 0.2).to(dev)
  bh = (torch.randn(CH, generator=g) * 0.1).to(dev)
  return x_in, wh, bh, _case(dev, N, 9, 12, seed=seed + 1)[1:]


@pytest.mark.parametrize('N', [1, 5])
def test_whole_stage_is_bitwise_head_then_tail(cuda, N):
  C = _C()
  x_in, wh, bh, tail = _stage_case(cuda, N, 30 + N)
  head = C.cf32_wino_conv_pool_fwd(x_in, wh, bh)
  assert head, 'the whole-image stage head declined'
  pooled = head[0]
  assert float(pooled.min()) < 0.0
  for last in (False, True):
    out = C.cf32_stage_fwd(x_in, wh, bh, *tail, last)
    assert out, 'the whole stage declined'
    assert out[0].shape == (N, 9, 12, CH)
    assert torch.equal(out[0], _four_convs(C, pooled, *tail, last))
    assert torch.equal(out[0], _tail(C, [pooled] + tail, last))


def test_grid_beyond_one_wave_of_workgroups(cuda):
  """300 images: one workgroup each, more than the 256 CUs."""
  C = _C()
  args = _case(cuda, 300, 9, 12, seed=5)
  assert torch.equal(_tail(C, args, False), _two_blocks(C, *args, False))


def test_declined_shapes_return_empty(cuda):
  C = _C()
  # above the inference bound
  assert C.cf32_stage_tail_fwd(*_case(cuda, 513, 9, 12), False) == []
  # no instance for the channel count
  assert C.cf32_stage_tail_fwd(*_case(cuda, 2, 9, 12, C=64), False) == []
  # 5x7: the two-launch form leaves the Winograd forward there
  assert C.cf32_stage_tail_fwd(*_case(cuda, 3, 5, 7), False) == []
  # 18x32 (the 72x128 frame): no whole-image head
  g = torch.Generator().manual_seed(0)
  x_in = torch.randn(2, 18, 32, CH, generator=g).to(cuda)
  p = _case(cuda, 2, 9, 16)[1:]
  assert C.cf32_stage_fwd(x_in, p[0], p[1], *p, False) == []
  assert C.cf32_stage_form(2, 18, 32, CH) == 1  # its two blocks still fuse
  assert C.cf32_stage_form(2, 18, 24, CH) == 2
  assert C.cf32_stage_form(2, 10, 14, CH) == 0
  assert C.cf32_stage_form(513, 18, 24, CH) == 0


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


@pytest.mark.parametrize('shape,form', [((72, 96, 3), 'stage'),
                                        ((84, 84, 4), 'tail'),
                                        ((20, 28, 3), None)])
def test_whole_torso(cuda, shape, form):
  """72x96: the whole last stage in one launch; 84x84: its two blocks (11x11);
  20x28: the last map is 5x7 and everything declines.  With grad enabled the
  agent takes the learner path and still matches."""
  stage, fused, plain = (_agent(cuda, shape, b) for b in ('stage', 'fused', 'ops'))
  assert stage.torso_blocks_fused() and stage.torso_stage_form() == form
  assert fused.torso_stage_form() is None and not plain.torso_blocks_fused()
  frames = _frames(cuda, 37, shape, 4)
  with torch.no_grad():
    feats = stage.conv_features(frames)
    feats_fused = fused.conv_features(frames)
    feats_ops = plain.conv_features(frames)
  with torch.enable_grad():
    feats_grad = stage.conv_features(frames)
  assert feats_grad.requires_grad and not feats.requires_grad
  assert torch.equal(feats, feats_ops)
  assert torch.equal(feats, feats_fused)
  assert torch.equal(feats, feats_grad.detach())


def test_graph_replay_matches_eager(cuda):
  shape = (72, 96, 3)
  ag = _agent(cuda, shape, 'stage')
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
    for k in (0, 1, 2):
      buf.copy_(batches[k])
      g.replay()
      side.synchronize()
      assert torch.equal(out, eager[k]), k


def test_float64_oracle(cuda):
  """The whole stage at N = 3, last: against a float64 reference on the CPU
  (conv, SAME 3x3/2 max-pool, the two blocks) the one-launch form's max-abs
  error is <= max(2e-5, 1.5 x the ops path's)."""
  C = _C()
  x_in, wh, bh, tail = _stage_case(cuda, 3, 21)
  d = lambda t: t.double().cpu()
  conv = layers.conv2d_same_nhwc(d(x_in), d(wh), d(bh), 1)
  # SAME 3x3/2 on an even map: pad-before 0, one padding row / column after
  x = F.max_pool2d(F.pad(conv.permute(0, 3, 1, 2), (0, 1, 0, 1),
                         value=float('-inf')), 3, 2).permute(0, 2, 3, 1)
  for k in range(2):
    w1, b1, w2, b2 = [d(t) for t in tail[4 * k:4 * k + 4]]
    t = layers.conv2d_same_nhwc(x.clamp(min=0), w1, b1, 1).clamp(min=0)
    x = layers.conv2d_same_nhwc(t, w2, b2, 1) + x
  ref = x.clamp(min=0)
  err = lambda y: (d(y) - ref).abs().max().item()
  pooled = C.cf32_wino_conv_pool_fwd(x_in, wh, bh)[0]
  e_ops = err(_four_convs(C, pooled, *tail, True))
  e_stage = err(C.cf32_stage_fwd(x_in, wh, bh, *tail, True)[0])
  print('float64 oracle: stage %.3e, ops %.3e (output scale %.2f)' %
        (e_stage, e_ops, ref.abs().max().item()))
  assert e_stage <= max(2e-5, 1.5 * e_ops)
