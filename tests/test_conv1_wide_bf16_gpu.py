"""Stage 0 of the bf16 deep torso on uint8 frames of 5 to 16 channels
(conv1w_pool_fwd / conv1w_pool_bwd, csrc/kernels/conv_wide_bf16.hip) against
the float64 oracle of tests/_conv_oracle.py.

C = 5, 8 are both ends of the Cp = 8 instance and 9, 16 of the Cp = 16 one (5
and 9: zero-padded channels, pixels that straddle 16-byte chunks).  21x19 is
odd and runs the runtime-geometry kernels, 72x96 a compiled instance; the
'loop' geometry is 21x19 again with 48 frames and short tiles (px knobs), so
that about 128 persistent workgroups walk two or three tiles each, the last
tile of every image a short one.
"""

import pytest
import torch

from tests import _conv_oracle as O

pytestmark = pytest.mark.gpu

# H, W, frames, px_conv1_fwd / px_conv1_bwd knob (0: default)
GEO = {'21x19': (21, 19, 3, 0), '72x96': (72, 96, 3, 0), 'loop': (21, 19, 48, 100)}
CASES = [(c, g) for c in (5, 8, 9, 16) for g in ('21x19', '72x96')] + [(5, 'loop'), (16, 'loop')]


def knobs(C, px):
  return O.tuned(C, px_conv1_fwd=px, px_conv1_bwd=px) if px else O.tuned(C)


def setup(C_, geo):
  H, W, N, px = GEO[geo]
  g = torch.Generator().manual_seed(1000 * C_ + H)
  w = torch.randn(3, 3, C_, 16, generator=g) * 0.2
  b = torch.randn(16, generator=g) * 0.1
  fr = torch.randint(0, 256, (N, H, W, C_), generator=g, dtype=torch.uint8)
  return H, W, N, px, g, w, b, fr


@pytest.mark.parametrize('C_,geo', CASES)
def test_conv1w_pool_fwd(cuda, C_, geo):
  C = O.ext()
  H, W, N, px, g, w, b, fr = setup(C_, geo)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  with O.small_grid(C), knobs(C, px):
    pooled, arg = C.conv1w_pool_fwd(fr.to(cuda), w.to(cuda), b.to(cuda), pb_h, pb_w)
    rec = O.record(C, 'conv1w_pool_fwd', '%s C=%d' % (geo, C_))
  assert rec['specialized'] == (geo == '72x96'), rec
  if geo == 'loop':
    assert rec['ntiles'] > rec['grid'] and rec['rows'] < (H + 1) // 2, rec
  # the kernel's operands: raw bytes (exact in bf16) and bf16(fp32(w / 255))
  w_k = (w * (1.0 / 255.0)).to(torch.bfloat16)
  x64, w64, b64 = O.d64(fr), O.d64(w_k), O.d64(b)
  y64 = O.conv64(x64, w64, b64)
  A = O.conv64(x64, w64.abs(), b64.abs())
  Cp = 8 if C_ <= 8 else 16
  ref, _ = O.pool64(y64, pb_h, pb_w)
  # the window's largest A: the fp32 max is that close to the float64 max
  Awin = O.pool_taps(A, pb_h, pb_w, fill=0.0).max(dim=-1).values
  O.check_bound(pooled, ref, Awin, Cp, 'conv1w_pool_fwd %s C=%d' % (geo, C_))
  # every code decodes to an in-image tap that rounds to the pooled value: a
  # near-tie may pick either tap, both within the bound of the window's max
  tol = O.REL * ref.abs() + 9 * Cp * O.ACC * Awin
  r, c = O.tap_positions(arg, H, W, pb_h, pb_w)
  n = torch.arange(N).view(N, 1, 1, 1).expand_as(r)
  ch = torch.arange(16).view(1, 1, 1, 16).expand_as(r)
  assert bool((y64[n, r, c, ch] >= ref - 2 * tol).all()), 'argmax is not a maximal tap'


@pytest.mark.parametrize('C_,geo', CASES)
def test_conv1w_pool_bwd(cuda, C_, geo):
  C = O.ext()
  H, W, N, px, g, w, b, fr = setup(C_, geo)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  fd = fr.to(cuda)
  # dP on a 1/8 grid: the gathered dY is exact in bf16 whatever the order
  dP = (torch.randint(-32, 33, (N, Hp, Wo, 16), generator=g).float() / 8).to(torch.bfloat16)
  dPd = dP.to(cuda)
  zeros = lambda: (torch.zeros(3, 3, C_, 16, device=cuda), torch.zeros(16, device=cuda))
  with O.small_grid(C), knobs(C, px):
    _, arg = C.conv1w_pool_fwd(fd, w.to(cuda), b.to(cuda), pb_h, pb_w)
    dw, db = zeros()
    C.conv1w_pool_bwd(dPd, arg, fd, dw, db, pb_h, pb_w)
    rec = O.record(C, 'conv1w_pool_bwd', '%s C=%d' % (geo, C_))
    dw1, db1 = dw.clone(), db.clone()
    C.conv1w_pool_bwd(dPd, arg, fd, dw, db, pb_h, pb_w)  # accumulates
    det = []
    with O.tuned(C, deterministic=1):
      for _ in range(2):
        det.append(zeros())
        C.conv1w_pool_bwd(dPd, arg, fd, det[-1][0], det[-1][1], pb_h, pb_w)
  assert rec['specialized'] == (geo == '72x96'), rec
  if geo == 'loop':
    assert rec['ntiles'] > rec['grid'] and rec['rows'] < H, rec
  dY = O.scatter64(dP, arg, H, W, pb_h, pb_w)
  dw_ref = O.wgrad64(O.d64(fr) / 255.0, dY)
  db_ref = dY.sum(dim=(0, 1, 2))
  tag = 'conv1w_pool_bwd %s C=%d ' % (geo, C_)
  O.check_max(dw1, dw_ref, 5e-3, tag + 'dw')
  O.check_max(db1, db_ref, 1e-3, tag + 'db')
  O.check_max(dw, 2 * O.d64(dw1), 1e-4, tag + 'dw second call')
  O.check_max(db, 2 * O.d64(db1), 1e-4, tag + 'db second call')
  O.bits_equal(det[0][0], det[1][0], tag + 'deterministic dw')
  O.bits_equal(det[0][1], det[1][1], tag + 'deterministic db')
  O.check_max(det[0][0], dw_ref, 5e-3, tag + 'deterministic dw')
  O.check_max(det[0][1], db_ref, 1e-3, tag + 'deterministic db')


def _cos(a, b):
  a, b = a.detach().float().reshape(-1), b.detach().float().reshape(-1)
  return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-12))


def test_wide_agent_runs_bf16_torso(cuda):
  """A bf16 HIP deep agent on 72x96x12 frames: the bf16 torso runs and tracks
  the fp32 torch agent as test_deep_torso_matches_fp32_reference asks at 3 / 4
  channels.

  64 frames, not that test's 6: the rule compares two noisy statistics.  On 6
  frames of uniform noise the reference side of the rule alone, torch's bf16
  gradient against the fp32 one, moves between 0.964 and 0.987 from one frame
  seed to the next at the stage-0 residual convs, and the HIP and torch
  cosines there differ by up to 0.018 in either direction, at 3 channels as
  at 12: more than the rule's margin of 0.01 (with 6 frames and this seed the
  rule was missed at residual_0_1__conv_2d__w, a gradient of res_conv_bwd,
  0.9709 against torch's 0.9837; with the next frame seed the HIP path led
  there by 0.008).  The frame count was set before the 64-frame run, on the
  expectation that per-pixel rounding events average out with the square root
  of their number.  Measured at 64 frames: the rule holds for every
  parameter, but the two paths still differ by up to 0.009 against (0.9785 /
  0.9872 at residual_0_0__conv_2d__b, the narrowest pass) and 0.015 for the
  HIP path, so a part of the difference does not average out over pixels: the
  two paths round the weights differently (the HIP stage 0 rounds w / 255,
  torch rounds w and x / 255), one perturbation shared by all pixels."""
  from scalable_agent_amd.models import Agent
  from scalable_agent_amd.models.agent import torso_precision
  shape = (72, 96, 12)
  torch.manual_seed(6)
  mk = lambda **kw: Agent(9, torso='deep', frame_shape=shape, seed=3, **kw).to(cuda)
  ref = mk()
  tbf = mk(compute_dtype=torch.bfloat16)
  hip = mk(backend='hip', compute_dtype=torch.bfloat16)
  assert torso_precision(hip) == 'bf16'
  frames = torch.randint(0, 256, (64,) + shape, device=cuda, dtype=torch.uint8)
  feats = [m.conv_features(frames) for m in (ref, tbf, hip)]
  assert feats[2].shape == feats[0].shape
  assert _cos(feats[2], feats[0]) > 0.999
  gr = torch.randn_like(feats[0])
  for f in feats:
    (f.float() * gr).sum().backward()
  named = [dict(m.convnet.named_parameters()) for m in (ref, tbf, hip)]
  for n in named[0]:
    c_hip = _cos(named[2][n].grad, named[0][n].grad)
    c_tbf = _cos(named[1][n].grad, named[0][n].grad)
    print('WIDECOS %s hip=%.4f torch_bf16=%.4f' % (n, c_hip, c_tbf))
    assert c_hip > min(0.99, c_tbf - 0.01), (n, c_hip, c_tbf)


def test_wide_agent_fused_stages_bitwise(cuda):
  """No-grad features of a 72x96x12 agent with torso_stages='fused' (stage 0:
  the wide head launch + tail) are bitwise those of 'ops'."""
  from scalable_agent_amd.models import Agent
  mk = lambda **kw: Agent(9, torso='deep', frame_shape=(72, 96, 12), seed=3, backend='hip',
                          compute_dtype=torch.bfloat16, **kw).to(cuda)
  ops, fused = mk(), mk(torso_stages='fused')
  g = torch.Generator().manual_seed(12)
  frames = torch.randint(0, 256, (6, 72, 96, 12), generator=g, dtype=torch.uint8).to(cuda)
  with torch.no_grad():
    assert any(fused.torso_stages_form())
    O.bits_equal(fused.conv_features(frames), ops.conv_features(frames), 'fused vs ops')
