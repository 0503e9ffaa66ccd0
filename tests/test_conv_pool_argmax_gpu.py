"""The fused conv + max-pool kernels' argmax, checked against an independent
rule instead of against itself.

The kernels document "first maximal tap of the 3x3 window" in dy*3+dx order
(key32 = ord16 << 16 | (15 - tap), pad keys below -inf).  Here:

  * exact ties: an identity conv on small non-zero integers makes every conv
    output exact and ties frequent; pooled must equal the max-pool bitwise
    and arg the first maximal IN-IMAGE tap computed on the CPU, on even maps
    (pad-before 0), odd maps (pad-before 1) and constant maps (every window
    fully tied: the corner window's code is 4 when pad-before is 1);
  * the backward kernels get a synthetic code map the forward never produced:
    uniformly random in-image codes, with regions where the four windows
    around a 2x2 block's (0, 0) cell all point at that one cell (the 4-way
    collision of gather_pool_grad_blocks), against a float64 scatter whose
    indices are asserted in range.

Random-input argmax checks (decoded without clamping) live with the forward
tests of test_conv_persistent_gpu.py.
"""

import contextlib

import pytest
import torch

from tests import _conv_oracle as O

pytestmark = pytest.mark.gpu


def bf16(t):
  return t.to(torch.bfloat16)


def grid_ctx(C, multi):
  return O.small_grid(C) if multi else contextlib.nullcontext()


def n_for(C, fam, probe, multi):
  """2 images, or (multi) about 2.4 tiles per workgroup of the small grid."""
  if not multi:
    return 2
  probe()
  rec = O.record(C, fam)
  return O.pick_n(rec['ntiles'], rec['grid_max'], 'x2.4')


def assert_multi(C, fam, multi, tag, compiled):
  """More tiles than workgroups iff `multi`, and the compile-time-geometry
  kernel iff the launchers hold one for this map (no silent fall-back to the
  runtime-geometry kernel on the production shapes)."""
  rec = O.record(C, fam, tag)
  assert (rec['ntiles'] > rec['grid']) == multi, rec
  assert rec['specialized'] == compiled, rec


def identity_weights(cin, cout):
  w = torch.zeros(3, 3, cin, cout)
  for co in range(cout):
    w[1, 1, co % cin, co] = 1.0
  return w


def tie_map(g, N, H, W, C, constant):
  if constant:
    return torch.full((N, H, W, C), 3.0)
  v = torch.randint(1, 5, (N, H, W, C), generator=g).float()
  return v * (torch.randint(0, 2, (N, H, W, C), generator=g).float() * 2 - 1)


TIE = [(16, 16, 36, 48), (16, 32, 36, 48), (32, 32, 21, 21), (32, 32, 11, 11),
       (32, 32, 7, 5), (32, 32, 18, 24)]


@pytest.mark.parametrize('multi', [False, True])
@pytest.mark.parametrize('constant', [False, True])
@pytest.mark.parametrize('CIN,COUT,H,W', TIE)
def test_conv_pool_tie_rule(cuda, CIN, COUT, H, W, constant, multi):
  C = O.ext()
  fam = 'conv_pool_fwd'
  g = torch.Generator().manual_seed(1000 + 7 * H + W + CIN + 3 * COUT + constant)
  w = identity_weights(CIN, COUT).to(cuda)
  b = torch.zeros(COUT, device=cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  with grid_ctx(C, multi):
    one = torch.zeros(1, H, W, CIN, device=cuda, dtype=torch.bfloat16)
    N = n_for(C, fam, lambda: C.conv_pool_fwd(one, w, b, pb_h, pb_w), multi)
    x = tie_map(g, N, H, W, CIN, constant)
    pooled, arg = C.conv_pool_fwd(bf16(x).to(cuda), w, b, pb_h, pb_w)
    assert_multi(C, fam, multi, 'tie %dx%d %d->%d' % (H, W, CIN, COUT),
                 O.is_compiled(fam, CIN, H, W))
  y = x[..., [co % CIN for co in range(COUT)]].double()  # the identity conv
  ref, code = O.pool64(y, pb_h, pb_w)
  O.bits_equal(pooled.cpu(), bf16(ref), 'pooled')
  assert torch.equal(arg.cpu().long(), code), \
      '%d codes are not the first maximal in-image tap' % \
      int((arg.cpu().long() != code).sum())
  if constant:
    assert int(code[0, 0, 0, 0]) == 3 * pb_h + pb_w  # 4 when pad-before is 1


@pytest.mark.parametrize('multi', [False, True])
@pytest.mark.parametrize('constant', [False, True])
@pytest.mark.parametrize('H,W,CH', [(72, 96, 3), (84, 84, 4), (21, 19, 4), (20, 26, 3)])
def test_conv1_pool_tie_rule(cuda, H, W, CH, constant, multi):
  """Frames in {0, 255} through a centre-tap weight of 1: the kernel's
  bf16(1 / 255) * 255 = 32895 / 32768 rounds to exactly 1.0 in bf16 (half an
  ulp above 1 is 1 + 2^-8 = 33024 / 32768), so every conv output is 0 or 1."""
  C = O.ext()
  fam = 'conv1_pool_fwd'
  g = torch.Generator().manual_seed(2000 + 7 * H + W + CH + constant)
  w = identity_weights(CH, 16).to(cuda)
  b = torch.zeros(16, device=cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  with grid_ctx(C, multi):
    one = torch.zeros(1, H, W, CH, device=cuda, dtype=torch.uint8)
    N = n_for(C, fam, lambda: C.conv1_pool_fwd(one, w, b, pb_h, pb_w), multi)
    if constant:
      fr = torch.full((N, H, W, CH), 255, dtype=torch.uint8)
    else:
      fr = (torch.randint(0, 2, (N, H, W, CH), generator=g) * 255).to(torch.uint8)
    pooled, arg = C.conv1_pool_fwd(fr.to(cuda), w, b, pb_h, pb_w)
    assert_multi(C, fam, multi, 'tie %dx%dx%d' % (H, W, CH),
                 O.is_compiled(fam, CH, H, W))
  y = (fr[..., [co % CH for co in range(16)]] // 255).double()
  ref, code = O.pool64(y, pb_h, pb_w)
  O.bits_equal(pooled.cpu(), bf16(ref), 'pooled')
  assert torch.equal(arg.cpu().long(), code), \
      '%d codes are not the first maximal in-image tap' % \
      int((arg.cpu().long() != code).sum())
  if constant:
    assert int(code[0, 0, 0, 0]) == 3 * pb_h + pb_w


# ------------------------------------------------ independent argmax, backward

def synthetic_codes(g, N, H, W, C, pb_h, pb_w):
  """Uniformly random in-image codes [N, Hp, Wo, C] (uint8); in a quarter of
  the channels (and, for image 0, everywhere) the windows (i, j), (i-1, j),
  (i, j-1), (i-1, j-1) all name the (0, 0) cell of 2x2 block (i, j), i.e. conv
  position (2i - pb_h, 2j - pb_w), with codes 0, 6, 2 and 8."""
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  i = torch.arange(Hp).view(1, Hp, 1, 1)
  j = torch.arange(Wo).view(1, 1, Wo, 1)
  ok = torch.zeros(N, Hp, Wo, C, 9, dtype=torch.bool)
  for k in range(9):
    r, c = 2 * i - pb_h + k // 3, 2 * j - pb_w + k % 3
    ok[..., k] = ((r >= 0) & (r < H) & (c >= 0) & (c < W)).expand(N, Hp, Wo, C)
  score = torch.rand(N, Hp, Wo, C, 9, generator=g).masked_fill(~ok, -1.0)
  code = score.argmax(dim=-1)
  # collisions: window (i, j) takes the code that points at the (0, 0) cell of
  # the block at (i + (i odd), j + (j odd)), when that cell is in the image
  tgt_r = 2 * (i + i % 2) - pb_h
  tgt_c = 2 * (j + j % 2) - pb_w
  forced = (i % 2) * 6 + (j % 2) * 2
  inside = ((tgt_r >= 0) & (tgt_r < H) & (tgt_c >= 0) & (tgt_c < W)).expand_as(code)
  region = torch.zeros_like(code, dtype=torch.bool)
  region[..., ::4] = True
  region[0] = True
  sel = region & inside
  code = torch.where(sel, forced.expand_as(code), code)
  return code.to(torch.uint8)


def pooled_grad(g, N, Hp, Wo, C):
  """1/8 grid in [-4, 4]: the sum of four is exact in bf16, so the gathered
  dY does not depend on the order or precision of the additions."""
  return bf16(torch.randint(-32, 33, (N, Hp, Wo, C), generator=g).float() / 8)


@pytest.mark.parametrize('multi', [False, True])
@pytest.mark.parametrize('CIN,COUT,H,W', [(16, 32, 36, 48), (32, 32, 21, 21),
                                          (32, 32, 18, 24), (16, 16, 10, 14),
                                          (32, 32, 7, 5)])
def test_pool_conv_bwd_independent_argmax(cuda, CIN, COUT, H, W, multi):
  C = O.ext()
  fam = 'pool_conv_bwd'
  g = torch.Generator().manual_seed(3000 + 7 * H + W + CIN + 3 * COUT)
  w = bf16(torch.randn(3, 3, CIN, COUT, generator=g) * 0.1).float()
  wd = w.to(cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  wshape = (3, 3, CIN, COUT)
  with grid_ctx(C, multi):
    dw, db = torch.zeros(*wshape, device=cuda), torch.zeros(COUT, device=cuda)
    one = torch.zeros(1, H, W, CIN, device=cuda, dtype=torch.bfloat16)
    onep = torch.zeros(1, Hp, Wo, COUT, device=cuda, dtype=torch.bfloat16)
    onea = torch.full((1, Hp, Wo, COUT), 4, device=cuda, dtype=torch.uint8)
    N = n_for(C, fam, lambda: C.pool_conv_bwd(onep, onea, one, wd, dw, db, True,
                                              pb_h, pb_w), multi)
    x = bf16(torch.randn(N, H, W, CIN, generator=g))
    code = synthetic_codes(g, N, H, W, COUT, pb_h, pb_w)
    dP = pooled_grad(g, N, Hp, Wo, COUT)
    dw.zero_()
    db.zero_()
    dx = C.pool_conv_bwd(dP.to(cuda), code.to(cuda), x.to(cuda), wd, dw, db, True,
                         pb_h, pb_w)
    assert_multi(C, fam, multi, 'synthetic %dx%d %d->%d' % (H, W, CIN, COUT),
                 O.is_compiled(fam, CIN, H, W))
  dY = O.scatter64(dP, code, H, W, pb_h, pb_w)
  assert torch.equal(dY, O.d64(bf16(dY)))
  # the forced regions do put four windows on one cell
  hits = O.scatter64(torch.ones_like(dP), code, H, W, pb_h, pb_w)
  assert int(hits.max()) == 4
  w64 = O.d64(w)
  tag = 'synthetic %dx%d %d->%d multi=%d' % (H, W, CIN, COUT, multi)
  O.check_bound(dx, O.dgrad64(dY, w64), O.dgrad64(dY.abs(), w64.abs()), CIN,
                'pool_conv_bwd.dx ' + tag)
  O.check_max(dw, O.wgrad64(O.d64(x), dY), 1e-3, 'pool_conv_bwd.dw ' + tag)
  O.check_max(db, dY.sum(dim=(0, 1, 2)), 1e-3, 'pool_conv_bwd.db ' + tag)


@pytest.mark.parametrize('multi', [False, True])
@pytest.mark.parametrize('H,W,CH', [(72, 96, 3), (84, 84, 4), (21, 19, 4)])
def test_conv1_pool_bwd_independent_argmax(cuda, H, W, CH, multi):
  C = O.ext()
  fam = 'conv1_pool_bwd'
  g = torch.Generator().manual_seed(4000 + 7 * H + W + CH)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  wshape = (3, 3, CH, 16)
  with grid_ctx(C, multi):
    dw, db = torch.zeros(*wshape, device=cuda), torch.zeros(16, device=cuda)
    one = torch.zeros(1, H, W, CH, device=cuda, dtype=torch.uint8)
    onep = torch.zeros(1, Hp, Wo, 16, device=cuda, dtype=torch.bfloat16)
    onea = torch.full((1, Hp, Wo, 16), 4, device=cuda, dtype=torch.uint8)
    N = n_for(C, fam, lambda: C.conv1_pool_bwd(onep, onea, one, dw, db, pb_h, pb_w),
              multi)
    fr = torch.randint(0, 256, (N, H, W, CH), generator=g, dtype=torch.uint8)
    code = synthetic_codes(g, N, H, W, 16, pb_h, pb_w)
    dP = pooled_grad(g, N, Hp, Wo, 16)
    dw.zero_()
    db.zero_()
    C.conv1_pool_bwd(dP.to(cuda), code.to(cuda), fr.to(cuda), dw, db, pb_h, pb_w)
    assert_multi(C, fam, multi, 'synthetic %dx%dx%d' % (H, W, CH),
                 O.is_compiled(fam, CH, H, W))
  dY = O.scatter64(dP, code, H, W, pb_h, pb_w)
  hits = O.scatter64(torch.ones_like(dP), code, H, W, pb_h, pb_w)
  assert int(hits.max()) == 4
  tag = 'synthetic %dx%dx%d multi=%d' % (H, W, CH, multi)
  O.check_max(dw, O.wgrad64(O.d64(fr) / 255.0, dY), 5e-3, 'conv1_pool_bwd.dw ' + tag)
  O.check_max(db, dY.sum(dim=(0, 1, 2)), 1e-3, 'conv1_pool_bwd.db ' + tag)
