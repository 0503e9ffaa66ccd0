"""Deep-ResNet conv torso on the fused gfx950 kernels (csrc/kernels/conv_torso.hip).

Forward per stage s (reference experiment.py:156-176):
  conv_pool_fwd      conv3x3 + bias + maxpool3x3/2 SAME (stage 1 straight from
                     the uint8 frame, x/255 folded into the weights)
  2 x [res_conv_fwd  t = relu(conv(relu(x)) + b)     (stored ReLU'd)
       res_conv_fwd  y = conv(t) + b + x   (+ final ReLU on the last)]
Backward per residual block: two fused dgrad+wgrad+bias passes; per stage head
one pass that gathers the pooled gradient through the saved argmax in LDS.
All activations NHWC bf16; weights/biases fp32 master copies (TF HWIO); their
gradients accumulate in fp32 directly inside the kernels.

torso_forward_stages (Agent(torso_stages='fused'), no autograd) runs each
stage whose maps fit a workgroup's LDS as ONE launch (stage_fwd_kernel:
stage_bf16_fwd, or stage_tail_bf16_fwd after conv1_pool_fwd), bitwise the
launches above.

The SHALLOW torso has one bf16 kernel, for actor inference only
(csrc/kernels/conv_shallow_bf16.hip, torso_forward_shallow_bf16): x / 255 and
the three convs (8x8/4, 4x4/2, 3x3/2) of a no-grad forward in one launch on
bf16 MFMA, uint8 frames in, bf16 features out.  It has no backward: the
learner, and supports() / TORSO_READY, stay deep-only.
"""

import os

import torch

from . import grad_sink
from ._ext import ext
from ..models import layers
from ..utils.knobs import measure_env

TORSO_READY = True
# whole-residual-block forward kernel (res_block_fwd) instead of two
# res_conv_fwd launches - bitwise identical.  At the learner's batch it
# measured slower (206 vs 169 us at 36x48x16, 143 vs 102 at 18x24x32: the
# convs are latency/issue bound, not HBM bound); at actor-inference batches
# (no autograd, <= FUSED_BLOCK_MAX_FRAMES frames) the launch it saves is
# worth more: a board launch 21 -> 15 kernels, 210 -> 190 us of kernels
# (profiles/experiments.md round 6).  SA_FUSED_BLOCK=1 (measurement runs)
# forces it everywhere.
FUSED_BLOCK = measure_env('SA_FUSED_BLOCK', '0') == '1'
FUSED_BLOCK_MAX_FRAMES = 512


def supports(agent):
  """Shapes the fused bf16 kernels cover: the deep ResNet on uint8 frames
  with 3 (RGB: DMLab, Doom) or 4 (stacked Atari frames, BASELINE config #2)
  channels - conv1 packs a pixel's channels into one bf16x4 MFMA operand;
  other inputs take the fp32 kernels, ops/conv_f32.py."""
  return agent.torso_kind == 'deep' and agent.frame_shape[2] in (3, 4)


def _pool_pads(h, w):
  return layers.same_pads(h, 3, 2)[0], layers.same_pads(w, 3, 2)[0]


def deep_param_list(agent):
  """[w, b, (w1, b1, w2, b2) x 2] per stage, in spec order."""
  out = []
  for sp in agent.specs:
    if sp['kind'] == 'conv':
      out += list(agent._conv_params(sp['name']))
    elif sp['kind'] == 'res':
      for sub in ('conv_2d', 'conv_2d_1'):
        out += list(agent._conv_params(sp['name'] + '__' + sub))
  return out


class _DeepTorso(torch.autograd.Function):

  @staticmethod
  def forward(ctx, frames, *params):
    return _deep_forward(ctx, FUSED_BLOCK, frames, params)

  @staticmethod
  def backward(ctx, grad_out):
    return _deep_backward(ctx, grad_out)


class _DeepTorsoInfer(_DeepTorso):
  """Small no-grad batches (actor inference): fused residual blocks."""

  @staticmethod
  def forward(ctx, frames, *params):
    return _deep_forward(ctx, True, frames, params)


def _deep_forward(ctx, fused_block, frames, params):
  C = ext()
  frames = frames.contiguous()
  x = frames
  saved = [frames]
  shapes = []
  p = 0
  for s in range(3):
    w, b = params[p], params[p + 1]
    p += 2
    H, W = x.shape[1], x.shape[2]
    pb_h, pb_w = _pool_pads(H, W)
    if s == 0:
      pooled, arg = C.conv1_pool_fwd(x, w, b, pb_h, pb_w)
    else:
      pooled, arg = C.conv_pool_fwd(x, w, b, pb_h, pb_w)
    shapes.append((H, W, pb_h, pb_w))
    saved += [arg]
    xa = pooled
    for blk in range(2):
      w1, b1, w2, b2 = params[p:p + 4]
      p += 4
      # t is stored ReLU'd: it is only ever consumed as relu(t) (conv 2's
      # input, and the (t > 0) mask in backward), so conv 2 skips its
      # input ReLU and its backward skips the activation ReLU.
      last = (s == 2 and blk == 1)
      if fused_block:
        # both convs of the block in one pass (t never re-read from HBM)
        t, y = C.res_block_fwd(xa, w1, b1, w2, b2, last)
      else:
        t = C.res_conv_fwd(xa, w1, b1, None, True, True)
        y = C.res_conv_fwd(t, w2, b2, xa, last, False)
      saved += [xa, t]
      xa = y
    if s < 2:
      saved += [xa]  # input of the next stage's conv
    x = xa
  ctx.save_for_backward(*saved, x, *params)
  ctx.shapes = shapes
  ctx.nparams = len(params)
  return x.reshape(x.shape[0], -1)


def _deep_backward(ctx, grad_out):
  C = ext()
  t = ctx.saved_tensors
  params = t[-ctx.nparams:]
  out = t[-ctx.nparams - 1]
  saved = list(t[:-ctx.nparams - 1])
  frames = saved[0]
  # unpack per stage: arg, (xa, t) x2, [stage_out]
  stages = []
  k = 1
  for s in range(3):
    arg = saved[k]
    k += 1
    blocks = []
    for _ in range(2):
      blocks.append((saved[k], saved[k + 1]))
      k += 2
    stage_out = None
    if s < 2:
      stage_out = saved[k]
      k += 1
    stages.append((arg, blocks, stage_out))
  # The kernels ACCUMULATE weight/bias gradients: inside
  # grad_sink.direct_grads() straight into the learner's flat gradient
  # buffer (None is returned for those parameters), else into fresh zeros.
  gviews, direct = grad_sink.sinks(params)
  # the torso's final ReLU: dy *= (out > 0), in place on our own bf16 copy
  dy = grad_out.reshape(out.shape)
  if dy.dtype != torch.bfloat16 or not dy.is_contiguous():
    dy = dy.to(torch.bfloat16).contiguous()
  else:
    dy = dy.clone()  # grad_out belongs to autograd: never masked in place
  C.relu_mask_bf16_(dy, out)
  p_base = [0, 10, 20]
  for s in reversed(range(3)):
    arg, blocks, _ = stages[s]
    pb = p_base[s]
    for blk in reversed(range(2)):
      xa, tt = blocks[blk]
      i1 = pb + 2 + 4 * blk
      w1, w2 = params[i1], params[i1 + 2]
      dt = C.res_conv_bwd(dy, tt, None, w2, gviews[i1 + 2], gviews[i1 + 3],
                          False)
      dy = C.res_conv_bwd(dt, xa, dy, w1, gviews[i1], gviews[i1 + 1], True)
    H, W, pb_h, pb_w = ctx.shapes[s]
    if s == 0:
      C.conv1_pool_bwd(dy, arg, frames, gviews[pb], gviews[pb + 1], pb_h,
                       pb_w)
    else:
      x_in = stages[s - 1][2]
      dy = C.pool_conv_bwd(dy, arg, x_in, params[pb], gviews[pb],
                           gviews[pb + 1], True, pb_h, pb_w)
  return (None,) + grad_sink.returned(gviews, direct)


def torso_forward(agent, frames):
  """uint8 frames [N,H,W,C] (C = 3 or 4) -> relu'd conv features [N, flat]
  (bf16).  Batches above conv_f32.MAX_FRAMES frames run in equal chunks."""
  if not supports(agent):
    raise NotImplementedError(
        'bf16 HIP torso: deep ResNet on 3/4-channel uint8 frames only (got %r, %r)' %
        (agent.torso_kind, agent.frame_shape))
  from .conv_f32 import _chunked
  fn = (_DeepTorsoInfer if (not torch.is_grad_enabled() and
                            frames.shape[0] <= FUSED_BLOCK_MAX_FRAMES)
        else _DeepTorso)
  return _chunked(fn, frames.contiguous(), deep_param_list(agent))


# ---- one-launch stages of the no-grad forward (stage_fwd_kernel) ----
# Host mirror of the launcher's arithmetic (conv_torso.hip: row_pitch,
# tile_groups, rows_pool_fwd, stage_lds_bytes): the binding's stage_bf16_form
# says the same (tests/test_torso_stages_flag.py).
_STAGE_LDS_LIMIT = 160 * 1024
_STAGE_FORMS = (None, 'stage', 'tail')


def _row_pitch(c, w):
  return (w + 2) * c + (16 if c == 32 else 0)


def _tile_groups(c, rows, w):
  if c == 32:
    return -(-rows // 2) * -(-w // 8)
  return -(-(rows * w) // 16)


def _max_tile_px(c):
  return 4 * 256 * 8 // c


def _w_lds_elems(cin, cout):
  return 192 * cout if cin == 16 else 9 * cin * cout


def _rows_pool_fwd(h, w, cin, px=400):
  hp = (h + 1) // 2
  rp = max((px // w - 1) // 2, 1)
  while rp > 1 and ((2 * rp + 3) * w * cin // 8 > 1024 or
                    _tile_groups(cin, 2 * rp + 1, w) > _max_tile_px(cin) // 16):
    rp -= 1
  rp = min(rp, hp)
  if 1 <= rp < hp:  # balance_rows
    n = -(-hp // rp)
    if 4 * (hp - (n - 1) * rp) < rp:
      rp = -(-hp // n)
  return rp


def stage_bf16_lds_bytes(h, w, cin, cout):
  """LDS bytes of the one-launch stage kernel: a [h, w, cin] stage input
  (cin -> cout = 32 head, pool, two blocks) or, cin == cout == 16, a pooled
  [h, w, 16] map (the two blocks)."""
  tail = cin == cout == 16
  hm, wm = (h, w) if tail else ((h + 1) // 2, (w + 1) // 2)
  img = (hm + 2) * _row_pitch(cout, wm) + cout
  union = 2 * _w_lds_elems(cout, cout) + img
  if not tail:
    rp = _rows_pool_fwd(h, w, cin)
    union = max(union, _w_lds_elems(cin, cout) +
                (2 * rp + 3) * _row_pitch(cin, w) + cin +
                (2 * rp + 1) * (w + 2) * cout)
  return 256 + (img + union) * 2


def stage_bf16_form(frames, h, w, cin, cout):
  """0, 1 (stage) or 2 (tail): the binding's stage_bf16_form in host Python."""
  frames, h, w = int(frames), int(h), int(w)
  if not (1 <= frames <= FUSED_BLOCK_MAX_FRAMES and 1 <= h <= 4096 and
          1 <= w <= 4096):
    return 0
  tail = cin == cout == 16
  if not tail and not (cin in (16, 32) and cout == 32):
    return 0
  wm = w if tail else (w + 1) // 2
  band = 2 * (16 // -(-wm // 8)) if cout == 32 else 512 // wm
  if band < 1:
    return 0
  if not tail:
    rp = _rows_pool_fwd(h, w, cin)
    if ((2 * rp + 3) * w * cin // 8 > 1024 or
        _tile_groups(cin, 2 * rp + 1, w) > _max_tile_px(cin) // 16):
      return 0
  if stage_bf16_lds_bytes(h, w, cin, cout) > _STAGE_LDS_LIMIT:
    return 0
  return 2 if tail else 1


def deep_stage_bf16_form(frame_shape, frames=1):
  """Per stage of the deep torso on `frames` uint8 frames of [H, W, C]:
  'stage' (head conv, max-pool and both blocks in one launch), 'tail' (stage
  0: both blocks in one launch after conv1_pool_fwd) or None (today's
  launches).  Host arithmetic only."""
  if len(frame_shape) != 3:
    return (None, None, None)
  h, w, _ = (int(d) for d in frame_shape)
  if h < 1 or w < 1:
    return (None, None, None)
  h1, w1 = (h + 1) // 2, (w + 1) // 2
  h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
  return (_STAGE_FORMS[stage_bf16_form(frames, h1, w1, 16, 16)],
          _STAGE_FORMS[stage_bf16_form(frames, h1, w1, 16, 32)],
          _STAGE_FORMS[stage_bf16_form(frames, h2, w2, 32, 32)])


def torso_forward_stages(agent, frames):
  """torso_forward's no-grad forward with each stage in the one-launch form
  deep_stage_bf16_form names for it (bitwise the same features); a stage with
  no form runs conv_pool_fwd + two res_block_fwd.  No autograd."""
  if not supports(agent):
    raise NotImplementedError(
        'bf16 HIP torso: deep ResNet on 3/4-channel uint8 frames only (got %r, %r)' %
        (agent.torso_kind, agent.frame_shape))
  if frames.dtype != torch.uint8:
    raise TypeError('HIP torso expects uint8 frames, got %s' % frames.dtype)
  C = ext()
  params = [p.detach() for p in deep_param_list(agent)]
  forms = deep_stage_bf16_form(frames.shape[1:], frames.shape[0])
  x = frames.contiguous()
  for s in range(3):
    w, b = params[10 * s], params[10 * s + 1]
    blocks = params[10 * s + 2:10 * s + 10]
    pb_h, pb_w = _pool_pads(x.shape[1], x.shape[2])
    last = s == 2
    if forms[s] == 'stage':
      x = C.stage_bf16_fwd(x, w, b, *blocks, pb_h, pb_w, last)
      continue
    if s == 0:
      x = C.conv1_pool_fwd(x, w, b, pb_h, pb_w)[0]
    else:
      x = C.conv_pool_fwd(x, w, b, pb_h, pb_w)[0]
    if forms[s] == 'tail':
      x = C.stage_tail_bf16_fwd(x, *blocks, last)
    else:
      x = C.res_block_fwd(x, *blocks[:4], False)[1]
      x = C.res_block_fwd(x, *blocks[4:], last)[1]
  return x.reshape(x.shape[0], -1)


SHALLOW_BF16_FRAMES = ((72, 96), (84, 84), (72, 128))


def shallow_bf16_form(frame_shape, frames=1):
  """True where shallow_bf16_fwd takes `frames` uint8 frames of this [H, W, C]
  shape: 72x96, 84x84 or 72x128 with C <= 4, 1 <= frames <=
  FUSED_BLOCK_MAX_FRAMES.  Host arithmetic only (the binding's
  shallow_bf16_form says the same)."""
  if len(frame_shape) != 3:
    return False
  h, w, c = (int(d) for d in frame_shape)
  return ((h, w) in SHALLOW_BF16_FRAMES and 1 <= c <= 4 and
          1 <= int(frames) <= FUSED_BLOCK_MAX_FRAMES)


def shallow_bf16_pack(agent, out=None):
  """The shallow agent's three conv weights in the kernel's bf16 B-operand
  layout (shallow_bf16_pack); out: three tensors to refresh in place."""
  from .conv_f32 import shallow_param_list
  p = shallow_param_list(agent)
  packed = ext().shallow_bf16_pack(p[0].detach(), p[2].detach(), p[4].detach())
  if out is None:
    return tuple(packed)
  for dst, src in zip(out, packed):
    dst.copy_(src)
  return out


def torso_forward_shallow_bf16(agent, frames):
  """uint8 frames [N,H,W,C] -> ReLU'd conv features [N, flat] (bf16) of the
  shallow torso in one launch; no autograd.  Uses the agent's
  _inference_cache['wsh16'] (packed once per weight publish) when present,
  else packs per call.  Raises where the kernel declines."""
  if agent.torso_kind != 'shallow':
    raise NotImplementedError('shallow bf16 torso on a %r agent' %
                              (agent.torso_kind,))
  if frames.dtype != torch.uint8:
    raise TypeError('HIP torso expects uint8 frames, got %s' % frames.dtype)
  from .conv_f32 import shallow_param_list
  cache = getattr(agent, '_inference_cache', None)
  wp = None if cache is None else cache.get('wsh16')
  if wp is None:
    wp = shallow_bf16_pack(agent)
  p = shallow_param_list(agent)
  x = ext().shallow_bf16_fwd(frames.contiguous(), wp[0], p[1].detach(),
                             wp[1], p[3].detach(), wp[2], p[5].detach())
  return x.reshape(x.shape[0], -1)


def linear_relu(x, w, b):
  """Torso FC: relu(x W + b) on bf16 operands, fp32 accumulation.  Without
  autograd (actor inference) it is one hand-written bf16 MFMA GEMM
  (gemm_bf16.hip, bias + ReLU in the epilogue, fp32 out); the differentiable
  per-op path (the fused core's test oracle) keeps torch.addmm."""
  x16 = x.to(torch.bfloat16).contiguous()
  w16 = w.to(torch.bfloat16).contiguous()
  if not (torch.is_grad_enabled() and
          (x.requires_grad or w.requires_grad or b.requires_grad)):
    out = torch.empty(x16.shape[0], w16.shape[1], device=x.device,
                      dtype=torch.float32)
    ext().gemm_bf16(x16, w16, False, False, out,
                    bias=b.detach().float().contiguous(), relu=True)
    return out
  y = torch.addmm(b.to(torch.bfloat16), x16, w16)
  return torch.relu(y).to(torch.float32)
