"""Row-keeping stager of the fused fp32 Winograd backward (conv_wino.hip
wino_bwd_fused32_kernel, SA_WINO_KEEP / cf32_wino_keep).

With the stager on, a workgroup keeps the input rows a range shares with the
previous range of its run in LDS and stages only the new ones; with it off
every range stages all its rows.  The LDS values, the MFMA order and the
reductions are the same, so dX, dW and db must be BITWISE equal between the
two, on every instance: compile-time geometry (18x24, 9x12, the 16 -> 32 head
at 36x48 with its wave-pair split, 21x21 / 11x11), the runtime-geometry
fallback (cf32_wino_geo(0)), runs of one range per workgroup (nothing kept:
fewer ranges than workgroups, or exactly as many) and runs of several ranges
(more ranges than the 128 workgroups left by cf32_cu_reserve(16)), ranges
that cross image boundaries, odd maps with a short last tile row.  One
float64 comparison per channel configuration at the tolerance of
tests/test_conv_f32_gpu.py.
"""
import pytest
import torch

from scalable_agent_amd.models import layers

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_conv_f32_gpu.py, test_conv_bwd_fused


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def rel_err(a, ref):
  a = a.detach().double().cpu()
  ref = ref.detach().double().cpu()
  return (a - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _inputs(N, H, W, Cx, Cy):
  g = torch.Generator().manual_seed(N * H + W + Cx + 3 * Cy)
  x = torch.randn(N, H, W, Cx, generator=g)
  w = torch.randn(3, 3, Cx, Cy, generator=g) / (9 * Cx) ** 0.5
  dy = torch.randn(N, H, W, Cy, generator=g)
  add = torch.randn(N, H, W, Cx, generator=g)
  return x, w, dy, add


def _run_both(cuda, x, w, dy, add, mask, relu_x, reserve, geo):
  """[(dx, dw, db) with the stager off, ... on]"""
  C = _C()
  Cx, Cy = w.shape[2], w.shape[3]
  xd, wd, dyd = x.to(cuda), w.to(cuda), dy.to(cuda)
  addd = add.to(cuda) if add is not None else None
  res = []
  prev_keep = C.cf32_wino_keep(1)
  prev_geo = C.cf32_wino_geo(geo)
  prev_res = C.cf32_cu_reserve(reserve)
  try:
    for keep in (0, 1):
      C.cf32_wino_keep(keep)
      dw = torch.zeros(3, 3, Cx, Cy, device=cuda)
      db = torch.zeros(Cy, device=cuda)
      before = C.cf32_wino_keep_launches()
      dx = C.cf32_conv_bwd_fused(dyd, wd, xd, relu_x, dw, db, add=addd, mask=mask)
      # every shape here fits the row slots: the launcher must not have
      # declined it and compared the plain stager with itself
      assert C.cf32_wino_keep_launches() - before == keep
      res.append((dx, dw, db))
    torch.cuda.synchronize()
  finally:
    C.cf32_wino_keep(prev_keep)
    C.cf32_wino_geo(prev_geo)
    C.cf32_cu_reserve(prev_res)
  return res


# (N, H, W, Cx, Cy, CU reserve, geometry switch).  Tiles per image / range:
# 18x24 108 / 32, 9x12 30 / 32, 36x48 432 / 32 (16 -> 32) or 64 (16 -> 16),
# 21x21 121 / 32, 11x11 36 / 32.  Reserve 16 leaves 128 workgroups.
CASES = [
    # fewer ranges than workgroups: one range per workgroup, nothing kept
    (3, 18, 24, 32, 32, 0, 1),    # 11 ranges, they cross image boundaries
    (5, 9, 12, 32, 32, 0, 1),     # 5 ranges, up to 3 images in one
    (2, 36, 48, 16, 32, 0, 1),    # 27 ranges, the wave-pair data gradient
    (3, 21, 21, 32, 32, 0, 0),    # runtime geometry, short last tile row
    (3, 11, 11, 32, 32, 0, 0),
    (3, 21, 21, 32, 32, 0, 1),
    (3, 11, 11, 32, 32, 0, 1),
    # exactly as many ranges as workgroups (128), and one more
    (136, 9, 12, 32, 32, 16, 1),
    (137, 9, 12, 32, 32, 16, 1),
    # more ranges than workgroups: runs of 2 - 5 ranges keep rows
    (160, 18, 24, 32, 32, 16, 1),  # 540 ranges
    (300, 9, 12, 32, 32, 16, 1),   # 282
    (24, 36, 48, 16, 32, 16, 1),   # 324
    (40, 36, 48, 16, 16, 16, 1),   # 270 (64-tile ranges, without mask only)
    (80, 21, 21, 32, 32, 16, 0),   # 303, runtime geometry
    (140, 11, 11, 32, 32, 16, 0),  # 158
    (80, 21, 21, 32, 32, 16, 1),
    (40, 18, 24, 32, 32, 16, 0),   # 135: the flagship map on runtime geometry
    (100, 18, 24, 32, 32, 0, 1),   # 338 ranges over 256 workgroups
]


# (mask, relu_x): a stage head, a residual block's second and first conv.  The
# masked 16 -> 16 backward is wino_bwd_fused_kernel, not fused32.
FLAGS = [(False, False), (True, False), (True, True)]
PARAMS = [c + f for c in CASES for f in FLAGS if not (c[3] == 16 and c[4] == 16 and f[0])]


@pytest.mark.parametrize('N,H,W,Cx,Cy,reserve,geo,mask,relu_x', PARAMS)
def test_keep_is_bitwise_the_plain_stager(cuda, N, H, W, Cx, Cy, reserve, geo, mask, relu_x):
  x, w, dy, add = _inputs(N, H, W, Cx, Cy)
  off, on = _run_both(cuda, x, w, dy, add if mask else None, mask, relu_x, reserve, geo)
  for name, a, b in zip(('dx', 'dw', 'db'), off, on):
    assert torch.equal(a, b), name


@pytest.mark.parametrize('N,H,W,Cx,Cy,mask,relu_x', [
    (160, 18, 24, 32, 32, True, True),
    (24, 36, 48, 16, 32, False, False),
    (40, 36, 48, 16, 16, False, False)])
def test_keep_matches_float64(cuda, N, H, W, Cx, Cy, mask, relu_x):
  """Runs of several ranges per workgroup (128 workgroups) against the
  float64 backward, and bitwise against the plain stager."""
  x, w, dy, add = _inputs(N, H, W, Cx, Cy)
  x64 = x.double().requires_grad_(True)
  xin = x64.clamp(min=0) if relu_x else x64
  w64 = w.double().requires_grad_(True)
  b64 = torch.zeros(Cy, dtype=torch.float64, requires_grad=True)
  _, gw, gb = torch.autograd.grad(layers.conv2d_same_nhwc(xin, w64, b64, 1),
                                  (x64, w64, b64), dy.double())
  x2 = x.double().requires_grad_(True)
  (gx,) = torch.autograd.grad(layers.conv2d_same_nhwc(x2, w.double(), None, 1), x2,
                              dy.double())
  ref = torch.where(x.double() > 0, gx, torch.zeros_like(gx)) + add.double() if mask else gx
  off, on = _run_both(cuda, x, w, dy, add if mask else None, mask, relu_x, 16, 1)
  for a, b in zip(off, on):
    assert torch.equal(a, b)
  assert rel_err(on[0], ref) <= TOL
  assert rel_err(on[1], gw) <= TOL
  assert rel_err(on[2], gb) <= TOL
