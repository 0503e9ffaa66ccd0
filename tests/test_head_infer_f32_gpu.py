"""The one-launch inference stage heads of the fp32 deep torso (csrc/kernels/
conv_wino.hip wino_head_infer_kernel): cf32_head_fwd computes conv3x3/1 SAME +
bias + max-pool 3x3/2 SAME of the uint8 frames (stage 0, 1-4 channels -> 16)
or of a 16-channel fp32 map (stage 1, -> 32) and writes only the pooled map.

It must be BITWISE the launches it replaces (cf32_frames_f32 +
cf32_wino_conv_pool_fwd, whose pooled values are those of the Winograd conv +
cf32_maxpool_fwd) at every band seam, with the pool's padding taps losing and
no overhanging tile row leaking in; it declines every other shape; the whole
fp32 torso with Agent(torso_blocks='heads') equals 'ops', 'fused' and 'stage'
bitwise, eagerly and replayed from a captured graph.  The kernel is also held
to a float64 oracle with the project's parity rule, max(2e-5, 1.5 x the old
path's own error), so a mistake shared by both forms would still show.
"""

import pytest
import torch

from scalable_agent_amd.models import Agent, layers

pytestmark = pytest.mark.gpu

FRAMES = [(72, 96, 3), (84, 84, 4), (72, 128, 3), (72, 96, 1)]
MAPS1 = [(36, 48), (42, 42), (36, 64)]  # the stage-1 inputs of the three frames


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _wb(dev, cin, cout, seed, scale=0.3, bias=None):
  g = torch.Generator().manual_seed(seed)
  w = torch.randn(3, 3, cin, cout, generator=g) * scale
  b = (torch.randn(cout, generator=g) * 0.1 if bias is None
       else torch.full((cout,), float(bias)))
  return w.to(dev), b.to(dev)


def _pad4(w):
  z = torch.zeros(3, 3, 4 - w.shape[2], w.shape[3], dtype=w.dtype, device=w.device)
  return torch.cat([w, z], dim=2).contiguous()


def _frames(dev, n, shape, seed):
  """Random bytes; the top of frame 0 (row 0, and as many more rows as 256
  bytes need: three of a one-channel 96-wide frame) walks every byte value."""
  g = torch.Generator().manual_seed(seed)
  f = torch.randint(0, 256, (n,) + tuple(shape), generator=g, dtype=torch.uint8)
  per_row = shape[1] * shape[2]
  rows = -(-256 // per_row)
  f[0, :rows] = (torch.arange(rows * per_row) % 256).to(torch.uint8).reshape(
      f[0, :rows].shape)
  assert f[0, :rows].unique().numel() == 256
  return f.to(dev)


def _old0(C, frames, w, b):
  """frames_f32 + the Winograd conv + pool (+ its fix-up) on the fp32 image."""
  out = C.cf32_wino_conv_pool_fwd(C.cf32_frames_f32(frames), _pad4(w), b)
  assert out, 'the stage-0 Winograd conv + pool declined %r' % (tuple(frames.shape),)
  return out[0]


def _old1(C, x, w, b):
  """The Winograd conv + pool of a 16-channel map (every width enabled: the
  42-wide instance is opt-in), and the conv + maxpool_fwd pair the torso runs
  where it is off: one set of pooled values."""
  out = C.cf32_wino_conv_pool_fwd(x, w, b, 15)
  assert out, 'the stage-1 Winograd conv + pool declined %r' % (tuple(x.shape),)
  H, W = x.shape[1], x.shape[2]
  pair = C.cf32_maxpool_fwd(C.cf32_conv_fwd(x, w, b, 1, 1, 1, H, W), 0, 0)[0]
  assert torch.equal(out[0], pair)
  return out[0]


def _head(C, x, w, b):
  out = C.cf32_head_fwd(x, w, b)
  assert out, 'the inference head declined %r' % (tuple(x.shape),)
  assert len(out) == 1 and out[0].dtype == torch.float32
  return out[0]


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('shape', FRAMES)
def test_stage0_is_bitwise_the_launches_it_replaces(cuda, shape, N):
  C = _C()
  frames = _frames(cuda, N, shape, seed=sum(shape) + N)
  w, b = _wb(cuda, shape[2], 16, seed=shape[1])
  ref = _old0(C, frames, w, b)
  y = _head(C, frames, w, b)
  assert y.shape == (N, shape[0] // 2, shape[1] // 2, 16)
  assert torch.equal(y, ref)
  assert torch.equal(_head(C, frames, _pad4(w), b), ref)
  assert float(ref.min()) < 0.0 < float(ref.max())


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('H,W', MAPS1)
def test_stage1_is_bitwise_wino_conv_pool(cuda, H, W, N):
  C = _C()
  g = torch.Generator().manual_seed(H * W + N)
  x = torch.randn(N, H, W, 16, generator=g).to(cuda)
  w, b = _wb(cuda, 16, 32, seed=W)
  y = _head(C, x, w, b)
  assert y.shape == (N, H // 2, W // 2, 32)
  assert torch.equal(y, _old1(C, x, w, b))


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4), (72, 128, 3)])
def test_padding_taps_lose_stage0(cuda, shape):
  """Bias -10, small weights: every pre-pool value is negative, so a pool
  padded with 0 (or an overhanging tile row of zeros) would win at the last
  pooled row / column."""
  C = _C()
  frames = _frames(cuda, 2, shape, seed=5)
  w, b = _wb(cuda, shape[2], 16, seed=6, scale=0.05, bias=-10.0)
  y = _head(C, frames, w, b)
  assert torch.equal(y, _old0(C, frames, w, b))
  assert float(y.max()) < 0.0


@pytest.mark.parametrize('H,W', MAPS1)
def test_padding_taps_lose_stage1(cuda, H, W):
  C = _C()
  g = torch.Generator().manual_seed(H + W)
  x = torch.randn(2, H, W, 16, generator=g).to(cuda)
  w, b = _wb(cuda, 16, 32, seed=8, scale=0.02, bias=-10.0)
  y = _head(C, x, w, b)
  assert torch.equal(y, _old1(C, x, w, b))
  assert float(y.max()) < 0.0


def _seam_rows(C, H, W, cin):
  """Pixel rows just below each band boundary: the row a band recomputes as
  its halo (the first of the next band's) and the one after."""
  bp = C.cf32_head_band(H, W, cin)
  assert bp > 0
  rows = [r for k in range(1, (H // 2 + bp - 1) // bp)
          for r in (2 * bp * k, 2 * bp * k + 1)]
  assert rows and max(rows) < H
  return rows


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4), (72, 128, 3)])
def test_band_seams_stage0(cuda, shape):
  C = _C()
  H, W, c = shape
  g = torch.Generator().manual_seed(11)
  f = torch.randint(0, 4, (2, H, W, c), generator=g, dtype=torch.uint8)
  rows = _seam_rows(C, H, W, c)
  f[:, rows] = torch.randint(200, 256, (2, len(rows), W, c), generator=g,
                             dtype=torch.uint8)
  f = f.to(cuda)
  w, b = _wb(cuda, c, 16, seed=12)
  assert torch.equal(_head(C, f, w, b), _old0(C, f, w, b))


@pytest.mark.parametrize('H,W', MAPS1)
def test_band_seams_stage1(cuda, H, W):
  C = _C()
  g = torch.Generator().manual_seed(13)
  x = torch.randn(2, H, W, 16, generator=g) * 0.01
  rows = _seam_rows(C, H, W, 16)
  x[:, rows] = torch.randn(2, len(rows), W, 16, generator=g) * 10.0
  x = x.to(cuda)
  w, b = _wb(cuda, 16, 32, seed=14)
  assert torch.equal(_head(C, x, w, b), _old1(C, x, w, b))


def _oracle(x64, w, b):
  conv = layers.conv2d_same_nhwc(x64, w.double().cpu(), b.double().cpu(), 1)
  return layers.maxpool_same_nhwc(conv)


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4), (72, 128, 3)])
def test_float64_oracle_stage0(cuda, shape):
  """conv + bias + max-pool in float64 on the CPU from the same frames: the
  head's max-abs error is <= max(2e-5, 1.5 x the old path's)."""
  C = _C()
  frames = _frames(cuda, 2, shape, seed=21)
  w, b = _wb(cuda, shape[2], 16, seed=22)
  ref = _oracle(frames.cpu().double() / 255.0, w, b)
  err = lambda y: (y.double().cpu() - ref).abs().max().item()
  e_ops, e_head = err(_old0(C, frames, w, b)), err(_head(C, frames, w, b))
  print('float64 oracle %r: head %.3e, old path %.3e (output scale %.2f)' %
        (shape, e_head, e_ops, ref.abs().max().item()))
  assert e_head <= max(2e-5, 1.5 * e_ops)


@pytest.mark.parametrize('H,W', MAPS1)
def test_float64_oracle_stage1(cuda, H, W):
  C = _C()
  g = torch.Generator().manual_seed(23)
  x = torch.randn(2, H, W, 16, generator=g).to(cuda)
  w, b = _wb(cuda, 16, 32, seed=24, scale=0.2)
  ref = _oracle(x.cpu().double(), w, b)
  err = lambda y: (y.double().cpu() - ref).abs().max().item()
  e_ops, e_head = err(_old1(C, x, w, b)), err(_head(C, x, w, b))
  print('float64 oracle %dx%d: head %.3e, old path %.3e (output scale %.2f)' %
        (H, W, e_head, e_ops, ref.abs().max().item()))
  assert e_head <= max(2e-5, 1.5 * e_ops)


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


def _plain_frames(cuda, n, shape, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.randint(0, 256, (n,) + tuple(shape), generator=g,
                       dtype=torch.uint8).to(cuda)


def test_declines(cuda):
  from scalable_agent_amd.ops.conv import FUSED_BLOCK_MAX_FRAMES
  C = _C()
  w3, b16 = _wb(cuda, 3, 16, seed=1)
  w16, b32 = _wb(cuda, 16, 32, seed=2)
  w32, _ = _wb(cuda, 32, 32, seed=3)
  u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=cuda)
  big = FUSED_BLOCK_MAX_FRAMES + 1
  # odd H; Cs = 3 with W * 3 % 4 != 0; too many frames; stage 2's channels
  assert C.cf32_head_fwd(u8(2, 71, 96, 3), w3, b16) == []
  assert C.cf32_head_form(2, 71, 96, 3, 16, True) == 0
  assert C.cf32_head_fwd(u8(2, 72, 94, 3), w3, b16) == []
  assert C.cf32_head_form(2, 72, 94, 3, 16, True) == 0
  assert C.cf32_head_fwd(u8(big, 72, 96, 3), w3, b16) == []
  assert C.cf32_head_form(big, 72, 96, 3, 16, True) == 0
  assert C.cf32_head_fwd(torch.zeros(2, 18, 24, 32, device=cuda), w32, b32) == []
  assert C.cf32_head_form(2, 18, 24, 32, 32, False) == 0
  # stage 1: odd H, a width with no instance
  assert C.cf32_head_fwd(torch.zeros(2, 35, 48, 16, device=cuda), w16, b32) == []
  assert C.cf32_head_form(2, 35, 48, 16, 32, False) == 0
  assert C.cf32_head_fwd(torch.zeros(2, 36, 50, 16, device=cuda), w16, b32) == []
  # ... and takes the shapes it covers
  assert C.cf32_head_form(2, 72, 96, 3, 16, True) == 1
  assert C.cf32_head_form(FUSED_BLOCK_MAX_FRAMES, 36, 48, 16, 32, False) == 1


@pytest.mark.parametrize('shape,n', [((37, 48, 3), 3), ((36, 50, 3), 3),
                                     ((20, 28, 3), 3), ((72, 96, 3), 513)])
def test_declined_frames_in_the_torso_equal_ops(cuda, shape, n):
  """Odd H, W * 3 % 4 != 0, a frame with no instance, and more frames than an
  inference launch takes: the torso runs what 'stage' / 'ops' run there."""
  heads, plain = _agent(cuda, shape, 'heads'), _agent(cuda, shape, 'ops')
  frames = _plain_frames(cuda, n, shape, 2)
  with torch.no_grad():
    assert torch.equal(heads.conv_features(frames), plain.conv_features(frames))


@pytest.mark.parametrize('shape,last', [((72, 96, 3), 'stage'),
                                        ((84, 84, 4), 'tail'),
                                        ((72, 128, 3), 'tail')])
def test_whole_torso(cuda, shape, last):
  """N = 5: 'heads' equals 'ops', 'fused' and 'stage' bitwise, eagerly and
  replayed from a captured graph (two replays, new frames in between); with
  grad enabled the agent takes the learner path and its gradients are those
  of an 'ops' agent."""
  heads, stage, fused, plain = (_agent(cuda, shape, b)
                                for b in ('heads', 'stage', 'fused', 'ops'))
  assert heads.torso_blocks_fused() and heads.torso_head_form() == (0, 1)
  assert heads.torso_stage_form() == last
  assert stage.torso_head_form() is None and plain.torso_head_form() is None
  batches = [_plain_frames(cuda, 5, shape, 4 + k) for k in range(3)]
  with torch.no_grad():
    eager = [heads.conv_features(f).clone() for f in batches]
    for other in (stage, fused, plain):
      assert torch.equal(eager[0], other.conv_features(batches[0]))
    assert torch.equal(eager[2], plain.conv_features(batches[2]))
  assert not torch.equal(eager[1], eager[2])

  buf = batches[0].clone()
  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side), torch.no_grad():
    heads.conv_features(buf)  # warm-up
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      out = heads.conv_features(buf)
    for k in (1, 2):
      buf.copy_(batches[k])
      g.replay()
      side.synchronize()
      assert torch.equal(out, eager[k]), k
  torch.cuda.current_stream(cuda).wait_stream(side)

  grads = []
  for ag in (heads, plain):
    with torch.enable_grad():
      feats = ag.conv_features(batches[0])
      assert feats.requires_grad
      assert torch.equal(feats.detach(), eager[0])
      (feats * feats).sum().backward()
    grads.append({k: p.grad.clone() for k, p in ag.convnet.items()
                  if p.grad is not None})
  assert grads[0] and grads[0].keys() == grads[1].keys()
  for k in grads[0]:
    assert torch.equal(grads[0][k], grads[1][k]), k
