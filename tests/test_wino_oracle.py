"""CPU checks of tests/_wino_oracle.py: the magnitude functions against a
brute-force Winograd evaluation of a tiny case, and, for every GPU case of
test_wino_ranges_gpu.py, what must hold of the inputs and the launch
arithmetic alone - the exact regime's precondition (4 * magnitude < 2^24), the
share of pool windows left out of the argmax comparison (< 1 %), the plan
literals, and the shape of the capped runs (every workgroup walks at least two
ranges, a run boundary falls strictly inside an image, a range spans two
images where RT does not divide the tiles per image).
"""

import pytest
import torch

from tests import _conv_f32_oracle as O
from tests import _wino_oracle as Wn


def _brute(x, w, absolute):
  """Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A tile by tile, channel by
  channel, with plain matrix products; `absolute`: on magnitudes."""
  f = (lambda t: t.abs()) if absolute else (lambda t: t)
  N, H, W, Ci = x.shape
  Co = w.shape[3]
  TY, TX = Wn.tiles_of(H, W)
  xp = torch.zeros(N, 2 * TY + 2, 2 * TX + 2, Ci, dtype=torch.float64)
  xp[:, 1:H + 1, 1:W + 1] = f(x)
  out = torch.zeros(N, 2 * TY, 2 * TX, Co, dtype=torch.float64)
  for n in range(N):
    for ty in range(TY):
      for tx in range(TX):
        for co in range(Co):
          M = torch.zeros(4, 4, dtype=torch.float64)
          for ci in range(Ci):
            d = xp[n, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4, ci]
            M += (f(Wn.G_) @ f(w[:, :, ci, co]) @ f(Wn.G_).T) * (f(Wn.BT) @ d @ f(Wn.BT).T)
          out[n, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2, co] = f(Wn.AT) @ M @ f(Wn.AT).T
  return out[:, :H, :W]


def _brute_wgrad(x, dy, absolute):
  f = (lambda t: t.abs()) if absolute else (lambda t: t)
  N, H, W, Ci = x.shape
  Co = dy.shape[3]
  TY, TX = Wn.tiles_of(H, W)
  xp = torch.zeros(N, 2 * TY + 2, 2 * TX + 2, Ci, dtype=torch.float64)
  xp[:, 1:H + 1, 1:W + 1] = f(x)
  yp = torch.zeros(N, 2 * TY, 2 * TX, Co, dtype=torch.float64)
  yp[:, :H, :W] = f(dy)
  dw = torch.zeros(3, 3, Ci, Co, dtype=torch.float64)
  for ci in range(Ci):
    for co in range(Co):
      P = torch.zeros(4, 4, dtype=torch.float64)
      for n in range(N):
        for ty in range(TY):
          for tx in range(TX):
            d = xp[n, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4, ci]
            t = yp[n, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2, co]
            P += (f(Wn.BT) @ d @ f(Wn.BT).T) * (f(Wn.AT).T @ t @ f(Wn.AT))
      dw[:, :, ci, co] = f(Wn.G_).T @ P @ f(Wn.G_)
  return dw


@pytest.mark.parametrize('H,W', [(4, 6), (5, 3)])
def test_magnitudes_match_brute_force(H, W):
  g = O.gen(H * 10 + W)
  x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
  w = torch.randn(3, 3, 3, 2, generator=g, dtype=torch.float64)
  dy = torch.randn(2, H, W, 2, generator=g, dtype=torch.float64)
  # the signed evaluation is the convolution; the magnitude dominates it and
  # the direct magnitude (every Winograd term expands into the direct ones)
  torch.testing.assert_close(Wn.wino_fwd(x, w, False), O.conv(x, w, None, 1),
                             rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(_brute(x, w, False), O.conv(x, w, None, 1), rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(Wn.mag_fwd(x, w), _brute(x, w, True), rtol=1e-13, atol=1e-13)
  assert bool((Wn.mag_fwd(x, w) >= O.conv(x.abs(), w.abs(), None, 1) - 1e-12).all())
  rw, _ = O.conv_wgrad(x, dy, 3, 1)
  torch.testing.assert_close(Wn.wino_wgrad(x, dy, False), rw, rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(Wn.mag_wgrad(x, dy), _brute_wgrad(x, dy, True),
                             rtol=1e-13, atol=1e-13)
  assert bool((Wn.mag_wgrad(x, dy) >= O.conv_wgrad(x.abs(), dy.abs(), 3, 1)[0] - 1e-12).all())
  # the data gradient is the forward over the flipped, transposed weights
  torch.testing.assert_close(Wn.wino_fwd(dy, Wn.flip_t(w), False),
                             O.conv_dgrad(dy, w, 1, H, W), rtol=1e-12, atol=1e-12)


def _runs_ok(nranges, caps, rt, tpi, N, spans=True):
  """The capped walks of a case: >= 2 ranges per run, uneven runs, a run
  boundary strictly inside an image, a range over two images."""
  assert caps[0] == Wn.CAP and 2 <= N <= 16
  assert nranges % caps[-1] != 0
  for cap in caps:
    rs = Wn.runs(nranges, cap)
    assert all(hi - lo >= 2 for lo, hi in rs), (nranges, cap, rs)
    assert nranges >= 2 * cap + 1
  rs = Wn.runs(nranges, caps[-1])
  assert any((lo * rt) % tpi != 0 for lo, _ in rs[1:])
  if spans and tpi % rt != 0:
    assert any((r * rt) // tpi != (min((r + 1) * rt, N * tpi) - 1) // tpi
               for r in range(nranges))


@pytest.mark.parametrize('name', Wn.fwd_cases())
def test_forward_cases(name):
  d = Wn.fwd_data(name, True)
  p = Wn.plan_fwd(d['N'], d['H'], d['W'], d['cin'], d['cout'])
  assert p is not None and p['family'] == 'wino_conv'
  _runs_ok(p['nranges'], d['caps'], 64, p['tiles_per_img'], d['N'])
  for flags in Wn.FWD_FLAGS:
    ref, A = Wn.fwd_ref(d, flags)
    assert Wn.exact_ok4(A)
    assert torch.equal(ref, ref.round()) and bool((ref.abs() <= A).all())
  bias, relu_in, add, relu_out = Wn.FWD_FLAGS['res1']
  assert Wn.FLAG_WORD['res1'] == 1 * relu_in + 2 * relu_out + 8 * add + 16 * bias == 19
  assert Wn.FLAG_WORD['res2'] == 24


@pytest.mark.parametrize('name', Wn.DGRAD_CASES)
def test_dgrad_cases(name):
  d = Wn.dgrad_data(name, True)
  p = Wn.plan_fwd(d['N'], d['H'], d['W'], d['cout'], d['cin'], flip=True)
  assert p is not None and p['fl'] == -1
  _runs_ok(p['nranges'], d['caps'], 64, p['tiles_per_img'], d['N'])
  for masked in (False, True):
    ref, A = Wn.dgrad_ref(d, masked)
    assert Wn.exact_ok4(A) and torch.equal(ref, ref.round())
  assert int((d['mask'] == 0).sum()) > 0  # exact zeros: the mask is x > 0


@pytest.mark.parametrize('name', sorted(Wn.POOL_CASES))
def test_pool_cases(name):
  d = Wn.pool_data(name, True)
  p, rpi = d['plan'], d['rpi']
  assert Wn.exact_ok4(d['mag']) and torch.equal(d['pre'], d['pre'].round())
  nr = p['nranges']
  assert nr == d['N'] * rpi and nr % d['caps'][-1] != 0
  for cap in d['caps']:
    assert nr >= 2 * cap + 1 and all(hi - lo >= 2 for lo, hi in Wn.runs(nr, cap))
  if rpi > 1:
    # some run starts at k > 0 of an image and some run crosses an image
    # boundary (run 0 starts at k = 0)
    starts = [lo for cap in d['caps'] for lo, _ in Wn.runs(nr, cap)]
    assert any(lo % rpi != 0 for lo in starts)
    assert any(lo // rpi != (hi - 1) // rpi for cap in d['caps'] for lo, hi in Wn.runs(nr, cap))
  if p['family'] == 'wino_pool_ot':
    # some capped run walks ranges k = KP - 2, KP - 1 (the single tile row) of
    # an image and on into the next image
    assert any(lo <= n * rpi + rpi - 2 and hi > (n + 1) * rpi for cap in d['caps']
               for lo, hi in Wn.runs(nr, cap) for n in range(d['N'] - 1))
  # integer maps: real ties, many of them partial
  ties = (d['win'] == d['val'].unsqueeze(-1)).sum(-1)
  assert int((ties > 1).sum()) >= 100 and int(((ties > 1) & (ties < 9)).sum()) >= 100
  r = Wn.pool_data(name, False)
  share = float((~r['clear']).double().mean())
  print('WINOREC near_tie_share %s %.4f%%' % (name, 100 * share))
  assert share < 0.01


def test_pool_caps_start_runs_everywhere():
  """Over the pool cases some capped run starts at k = 0 of an image other
  than the first and some at k > 0."""
  k0 = kpos = 0
  for name in Wn.POOL_CASES:
    q = Wn.pool_geom(name)
    for cap in q['caps']:
      for lo, _ in Wn.runs(q['plan']['nranges'], cap)[1:]:
        k0 += lo % q['rpi'] == 0 and q['rpi'] > 1
        kpos += lo % q['rpi'] != 0
  assert k0 >= 3 and kpos >= 3


@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('hw', Wn.WGRAD_MAPS)
def test_wgrad_cases(hw, relu_in):
  d = Wn.wgrad_data(hw, relu_in, True)
  p = Wn.plan_wgrad(d['N'], *hw)
  assert p is not None
  _runs_ok(p['nranges'], d['caps'], 64, p['tiles_per_img'], d['N'])
  assert Wn.exact_ok4(d['mw'], d['mb'])
  assert torch.equal(d['rw'], d['rw'].round()) and torch.equal(d['rb'], d['rb'].round())
  assert float(d['dw0'].abs().min()) > 0 and float(d['db0'].abs().min()) > 0


@pytest.mark.parametrize('name', Wn.bwd_cases())
def test_bwd_cases(name):
  d = Wn.bwd_data(name, True)
  p = Wn.plan_bwd(d['N'], d['H'], d['W'], d['cx'], d['cy'], d['relu'], d['mask'])
  assert p is not None
  _runs_ok(p['nranges'], d['caps'], p['rt'], p['tiles_per_img'], d['N'])
  assert Wn.exact_ok4(d['mdx'], d['mw'], d['mb'])
  assert torch.equal(d['dx'], d['dx'].round()) and torch.equal(d['rw'], d['rw'].round())
  assert int((d['x'] == 0).sum()) > 0
  if p['family'] == 'wino_bwd32':
    keep = Wn.keep_expected(d['N'], d['H'], d['W'], d['cx'], d['cy'])
    assert keep == (name not in Wn.KEEP_DECLINED)
    assert Wn.bwd_family(name) == ('wino_bwd32_keep' if keep else 'wino_bwd32')
    assert Wn.bwd_family(name, keep_on=False) == 'wino_bwd32'
  else:
    assert Wn.bwd_family(name) == 'wino_bwd16' and name not in Wn.KEEP_DECLINED


def _plan(family, cin, cout, grid, nranges, rt, tpi, geo, fl, flip):
  return dict(family=family, cin=cin, cout=cout, grid=grid, nranges=nranges, rt=rt,
              tiles_per_img=tpi, geo=geo, fl=fl, flip=flip)


def test_plan_literals():
  """The launchers' arithmetic by hand, cap 0 (grid = min(nranges, 256 x
  workgroups per CU); 64-tile ranges unless noted)."""
  # forward 16 -> 16 at 36x48: 18 x 24 = 432 tiles per image; 2 images = 864
  # tiles = 13.5 ranges; res conv 1 (fl 19) has a compile-time instance
  assert Wn.plan_fwd(2, 36, 48, 16, 16, fl=19) == _plan('wino_conv', 16, 16, 14, 14, 64, 432,
                                                        1, 19, 0)
  assert Wn.plan_fwd(2, 36, 48, 16, 16, fl=19, geo_on=False) == _plan(
      'wino_conv', 16, 16, 14, 14, 64, 432, 0, -1, 0)
  assert Wn.plan_fwd(4, 18, 24, 32, 32, fl=24) == _plan('wino_conv', 32, 32, 7, 7, 64, 108,
                                                        1, 24, 0)
  assert Wn.plan_fwd(13, 9, 12, 32, 32, fl=19) == _plan('wino_conv', 32, 32, 7, 7, 64, 30,
                                                        1, -1, 0)
  assert Wn.plan_fwd(11, 11, 11, 32, 32, flip=True) == _plan('wino_conv', 32, 32, 7, 7, 64, 36,
                                                             1, -1, 1)
  # production batch: 256 x 432 / 64 = 1728 ranges; 16 -> 16 has 4-wave
  # workgroups, 2 per CU (WPS 2): 512; 16 -> 32 and 32 -> 32 8 waves, 1 per CU
  assert Wn.plan_fwd(256, 36, 48, 16, 16)['grid'] == 512
  assert Wn.plan_fwd(256, 36, 48, 16, 32)['grid'] == 256
  assert Wn.plan_fwd(256, 18, 24, 32, 32)['grid'] == 256
  assert Wn.plan_fwd(256, 18, 24, 32, 32)['nranges'] == 432
  # declines: 7x9 has 20 tiles per image (a range would touch 5 images); the
  # widest maps past the staging slots
  assert Wn.plan_fwd(8, 7, 9, 16, 16) is None
  assert Wn.plan_fwd(2, 4, 128, 32, 32) is None and Wn.plan_fwd(2, 4, 128, 16, 16) is not None
  assert Wn.plan_fwd(2, 8, 144, 16, 16) is None
  # stage heads: one range per tile-row pair; W 48 x 32 channels = 6 waves,
  # 2 workgroups per CU; W 64: 8 waves, 1; W 32: 4 waves, 3
  assert Wn.plan_pool(4, 8, 48, 16, 32) == _plan('wino_pool', 16, 32, 8, 8, 48, 96, 0, -1, 0)
  assert Wn.plan_pool(2, 42, 42, 16, 32) == _plan('wino_pool_ot', 16, 32, 22, 22, 42, 441,
                                                  0, -1, 0)
  assert Wn.plan_pool(256, 36, 48, 16, 32)['grid'] == 512
  assert Wn.plan_pool(256, 36, 64, 16, 32)['grid'] == 256
  assert Wn.plan_pool(256, 36, 32, 16, 32)['grid'] == 768
  assert Wn.plan_pool(256, 72, 96, 4, 16)['grid'] == 512
  assert Wn.plan_pool(256, 72, 128, 4, 16)['grid'] == 256
  assert Wn.plan_pool_img(7, 18, 24, 32, 32) == _plan('wino_pool_img', 32, 32, 7, 7, 108, 108,
                                                      1, -1, 0)
  assert Wn.plan_pool_img(300, 18, 24, 32, 32)['grid'] == 256
  # weight gradient 32 -> 32
  assert Wn.plan_wgrad(4, 18, 24) == _plan('wino_wgrad', 32, 32, 7, 7, 64, 108, 0, -1, 0)
  assert Wn.plan_wgrad(256, 18, 24)['grid'] == 256
  assert Wn.plan_wgrad(8, 7, 9) is None
  # fused backward: 32-tile ranges for the 32-channel-output forms
  assert Wn.plan_bwd(3, 36, 48, 16, 32, False, False) == _plan('wino_bwd32', 16, 32, 41, 41, 32,
                                                               432, 1, 0, 1)
  assert Wn.plan_bwd(2, 18, 24, 32, 32, True, True) == _plan('wino_bwd32', 32, 32, 7, 7, 32,
                                                             108, 1, 5, 1)
  assert Wn.plan_bwd(2, 36, 48, 16, 16, True, True) == _plan('wino_bwd16', 16, 16, 14, 14, 64,
                                                             432, 1, 5, 1)
  assert Wn.plan_bwd(2, 36, 48, 16, 16, False, False) == _plan('wino_bwd32', 16, 16, 14, 14, 64,
                                                               432, 1, 0, 1)
  assert Wn.plan_bwd(256, 36, 48, 16, 16, True, True)['grid'] == 256
  assert Wn.plan_bwd(3, 16, 48, 16, 32, False, False)['geo'] == 0
  assert Wn.wg_slot_cap(16, 16) == Wn.wg_slot_cap(16, 32) == Wn.wg_slot_cap(32, 32) == 512
  # the picker's examples by hand
  assert Wn.pick_tiles(36, 48, 64) == (2, (3,)) and Wn.pick_tiles(18, 24, 64) == (4, (3,))
  assert Wn.pick_tiles(36, 64, 64) == (2, (3, 4))   # 9 ranges per image: % 3 == 0 always
