"""CPU checks of tests/_conv_f32_oracle.py: each float64 oracle against
float64 torch.autograd on two tiny shapes, and, for every GPU case of
test_conv_f32_direct_gpu.py, what must hold of the INPUTS alone - the exact
regime's precondition (the operation applied to magnitudes stays below 2^24),
the share of pool windows left out of the argmax comparison (< 1 %), the tile
counts of the capped runs and the documented short-tile / ragged-group cases.
"""

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_f32_oracle as O


def _auto_conv(x, w, b, S):
  K = w.shape[0]
  (pt, pb), (pl, pr) = O.same_pads(x.shape[1], K, S), O.same_pads(x.shape[2], K, S)
  xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
  return F.conv2d(xp, w.permute(3, 2, 0, 1), b, stride=S).permute(0, 2, 3, 1)


def _auto_pool(x):
  (pt, pb), (pl, pr) = O.same_pads(x.shape[1], 3, 2), O.same_pads(x.shape[2], 3, 2)
  xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=float('-inf'))
  return F.max_pool2d(xp, 3, 2).permute(0, 2, 3, 1)


# 9x12 -> 5x6 (W pad 0/1, H pad 1/1) and 11x11, every kernel size / stride
@pytest.mark.parametrize('H,W', [(9, 12), (11, 11)])
@pytest.mark.parametrize('K,S', [(3, 2), (3, 1), (4, 2), (8, 4), (4, 1)])
def test_conv_oracles_match_autograd(H, W, K, S):
  g = O.gen(K * 100 + S * 10 + H)
  x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64, requires_grad=True)
  w = torch.randn(K, K, 3, 5, generator=g, dtype=torch.float64, requires_grad=True)
  b = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True)
  y = _auto_conv(x, w, b, S)
  dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
  gx, gw, gb = torch.autograd.grad(y, (x, w, b), dy)
  assert y.shape[1:3] == (O.same_out(H, S), O.same_out(W, S))
  torch.testing.assert_close(O.conv(x.detach(), w.detach(), b.detach(), S), y.detach(),
                             rtol=1e-12, atol=1e-12)
  mask = torch.randn(x.shape, generator=g, dtype=torch.float64)
  add = torch.randn(x.shape, generator=g, dtype=torch.float64)
  torch.testing.assert_close(O.conv_dgrad(dy, w.detach(), S, H, W), gx, rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(O.conv_dgrad(dy, w.detach(), S, H, W, mask, add),
                             torch.where(mask > 0, gx, torch.zeros_like(gx)) + add,
                             rtol=1e-12, atol=1e-12)
  rw, rb = O.conv_wgrad(x.detach(), dy, K, S)
  torch.testing.assert_close(rw, gw, rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(rb, gb, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('H,W', [(9, 12), (11, 11), (10, 7)])
def test_pool_oracles_match_autograd(H, W):
  g = O.gen(H * W)
  x = torch.randn(2, H, W, 4, generator=g, dtype=torch.float64, requires_grad=True)
  y = _auto_pool(x)
  dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
  (gx,) = torch.autograd.grad(y, x, dy)
  val, code = O.maxpool(x.detach())
  assert torch.equal(val, y.detach())
  assert int(code.min()) >= 0 and int(code.max()) <= 8
  torch.testing.assert_close(O.pool_gather(dy, code, H, W), gx, rtol=1e-12, atol=1e-12)


def test_first_tap_wins_ties():
  x = torch.zeros(1, 5, 6, 4, dtype=torch.float64)
  val, code = O.maxpool(x)
  # H = 5: pad-before 1, so the first in-image tap of row 0 is dy = 1; W = 6:
  # pad-before 0, the first tap is dx = 0
  assert torch.equal(code[0, :, :, 0], torch.tensor([[3, 3, 3], [0, 0, 0], [0, 0, 0]]))
  x[0, 2, 3, 0] = 1.0   # window (1, 1) taps rows 1..3, cols 2..4: code 1*3+1
  assert int(O.maxpool(x)[1][0, 1, 1, 0]) == 4
  ones = torch.ones(1, 3, 3, 4, dtype=torch.float64)
  dx = O.pool_gather(ones, O.maxpool(x)[1], 5, 6)
  assert float(dx.sum()) == float(ones.sum())  # every window routed once, inside the map


def _tiles_ok(q):
  p = q['plan']
  for cap in q['caps']:
    assert p['ntiles'] >= 2 * cap + 1, (q, cap)
  assert 2 <= q['N'] <= 9
  assert p['ntiles'] % q['caps'][-1] != 0
  assert q['caps'][0] == O.CAP


@pytest.mark.parametrize('name', sorted(O.ALL_FWD))
def test_forward_cases_are_exact_and_multi_tile(name):
  d = O.fwd_data(name, True)
  _tiles_ok(d)
  for flags in O.FWD_FLAGS:
    ref, A = O.fwd_ref(d, flags)
    assert O.exact_ok(A)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= float(A.max())
  p = d['plan']
  R = p['rows']
  last = d['Ho'] - (p['tiles_per_img'] - 1) * R
  assert (last < R) == (name in O.FWD_SHORT_TILE)
  assert ((R * d['Wo']) % 16 != 0 or (last * d['Wo']) % 16 != 0) == (name in O.FWD_RAGGED_GROUP)


@pytest.mark.parametrize('mode', ['phase', 'stack', 'dilated'])
@pytest.mark.parametrize('name', sorted(O.ALL_DGRAD))
def test_dgrad_cases_are_exact_and_multi_tile(name, mode):
  if mode != 'phase' and O.ALL_DGRAD[name][5] == 1:
    return  # stride 1: one form only
  d = O.dgrad_data(name, True, mode)
  _tiles_ok(d)
  for masked in (False, True):
    ref, A = O.dgrad_ref(d, masked)
    assert O.exact_ok(A)
    assert torch.equal(ref, ref.round())


@pytest.mark.parametrize('name', sorted(O.POOL_CASES))
def test_pool_cases_are_exact_and_mostly_clear(name):
  d = O.pool_data(name, True)
  _tiles_ok(d)
  assert d['plan']['tiles_per_img'] >= 2  # a seam row inside every image
  assert O.exact_ok(d['pre_bound'] / (O.U * (9 * d['Cs'] + 5)))
  assert torch.equal(d['pre'], d['pre'].round())
  # integer maps: real ties, so the first-tap rule decides many windows
  win = O.pool_windows(d['pre'])[0]
  ties = (win == d['val'].unsqueeze(-1)).sum(-1) > 1
  assert int(ties.sum()) >= 100
  r = O.pool_data(name, False)
  assert float((~r['clear']).double().mean()) < 0.01


@pytest.mark.parametrize('scatter', [True, False])
@pytest.mark.parametrize('name', sorted(O.WGRAD_CASES))
def test_wgrad_cases_are_exact_and_multi_tile(name, scatter):
  if not scatter and not name.startswith('stage0'):
    return  # the switch only moves the stage-0 cases
  d = O.wgrad_data(name, True, scatter)
  _tiles_ok(d)
  assert O.exact_ok(d['mw'], d['mb'])
  assert torch.equal(d['rw'], d['rw'].round()) and torch.equal(d['rb'], d['rb'].round())
  assert float(d['dw0'].abs().min()) > 0 and float(d['db0'].abs().min()) > 0
  # the slot tree's depth stays inside the bound's M (module docstring)
  assert d['M'] // 3 + 12 <= d['M']


@pytest.mark.parametrize('shape', O.MAXPOOL_SHAPES)
def test_maxpool_cases_have_ties_and_stay_exact(shape):
  for C in O.MAXPOOL_CHANNELS:
    d = O.maxpool_data(shape, C, True)
    assert O.exact_ok(d['dxmag'])
    win = O.pool_windows(d['x'].double())[0]
    assert float(((win == d['val'].unsqueeze(-1)).sum(-1) > 1).double().mean()) > 0.3
  assert {O.same_pads(n, 3, 2)[0] for s in O.MAXPOOL_SHAPES for n in s[1:]} == {0, 1}


def test_launch_arithmetic_of_the_existing_shapes():
  """run_conv / run_wgrad by hand for the shapes of test_conv_f32_gpu.SHAPES
  that take the direct kernels (grid cap 0); the GPU suite compares
  cf32_launch_info with the same functions."""
  assert O.plan_conv(3, 18, 24, 4, 32, 8, 4) == dict(
      family='conv_fwd', grid_x=15, grid_y=1, ntiles=15, rows=4, tiles_per_img=5)
  assert O.plan_conv(3, 9, 12, 32, 64, 4, 2) == dict(
      family='conv_fwd', grid_x=9, grid_y=4, ntiles=9, rows=3, tiles_per_img=3)
  assert O.plan_conv(3, 5, 6, 64, 128, 3, 2) == dict(
      family='conv_fwd', grid_x=3, grid_y=8, ntiles=3, rows=5, tiles_per_img=1)
  assert O.plan_conv(3, 72, 96, 4, 16, 3, 1) == dict(
      family='conv_fwd', grid_x=108, grid_y=1, ntiles=108, rows=2, tiles_per_img=36)
  assert O.plan_conv(2, 21, 21, 4, 32, 8, 4) == dict(
      family='conv_fwd', grid_x=14, grid_y=1, ntiles=14, rows=3, tiles_per_img=7)
  assert O.plan_wgrad(3, 18, 24, 4, 32, 8, 4) == dict(
      family='conv_wgrad', grid_x=15, grid_y=1, ntiles=15, rows=4, tiles_per_img=5)
  assert O.plan_wgrad(3, 9, 12, 32, 64, 4, 2) == dict(
      family='conv_wgrad', grid_x=9, grid_y=1, ntiles=9, rows=3, tiles_per_img=3)
  assert O.plan_wgrad(3, 5, 6, 64, 128, 3, 2) == dict(
      family='conv_wgrad', grid_x=6, grid_y=2, ntiles=6, rows=3, tiles_per_img=2)
  assert O.plan_wgrad(3, 36, 48, 16, 32, 3, 1) == dict(
      family='conv_wgrad', grid_x=24, grid_y=1, ntiles=24, rows=5, tiles_per_img=8)
  assert O.plan_wgrad(3, 72, 96, 4, 16, 3, 1) == dict(
      family='conv_wgrad', grid_x=45, grid_y=1, ntiles=45, rows=5, tiles_per_img=15)
