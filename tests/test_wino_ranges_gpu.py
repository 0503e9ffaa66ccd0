"""The persistent fp32 Winograd kernels of csrc/kernels/conv_wino.hip against
the direct float64 oracles (tests/_wino_oracle.py), with every workgroup
walking a run of several ranges.

Every persistent Winograd kernel walks the contiguous run
[b nranges / G, (b + 1) nranges / G) of ranges, prefetches one range ahead and
carries state between ranges (the pool kernel's register carry, the fused32
kernel's kept LDS rows).  The launchers size G from the CU count, so at the
2..13 images a quick test can afford every workgroup gets ONE range.  Each
case therefore runs
  * with cf32_wino_grid_cap(0): the control, every range a run start, and the
    launch compared with the launchers' arithmetic redone by hand (so the
    hooks change no launch), and
  * with cf32_wino_grid_cap(3) (also 4 where nranges % 3 == 0 for every N,
    and 2 for the 10x48 odd-tile-row head, _wino_oracle.POOL_EXTRA_CAPS):
    runs of 2 or more ranges, uneven, a run boundary inside an image, ranges
    across two images, a ragged last range wherever the map allows one.
Family, geometry, flag instance and grid are asserted from
cf32_wino_launch_info; inputs are read from buf[1:1+N] of NaN-filled storage;
dW / db start from non-zero values; the hooks are restored in `finally`; the
sticky conv error word is read after every case (cf32_wino_fault is never set
here).

Two regimes (derivations in the oracle module): integer inputs, where the
output must EQUAL the direct float64 result (torch.equal; pool argmax codes at
every element, ties included), and normal inputs under the elementwise bound
(M + c) 2^-24 magnitude.  The largest error / bound ratio per family is
printed as a WINOREC line.

Not covered (reachable only in builds with SA_MEASURE_KNOBS): the instances
behind SA_WINO_CFG, SA_WINO_WG_ALL, SA_WINO16_3W, the KD variants of the
16-channel fused backward (SA_FUSED_BWD_KD / SA_FUSED_BWD_WWG=0) and strided
walks under SA_WINO_RUNS=0.
"""

import contextlib

import pytest
import torch

from tests import _conv_f32_oracle as O
from tests import _wino_oracle as Wn

pytestmark = pytest.mark.gpu

REGIMES = [True, False]
REGIME_IDS = ['exact', 'rounding']
_REC = {}


def _rec(family, case, r):
  _REC[family] = max(_REC.get(family, 0.0), r)
  print('WINOREC %s %s ratio=%.3e family_max=%.3e' % (family, case, r, _REC[family]))


@contextlib.contextmanager
def _hooks(C, cap, geo=1, keep=1):
  """Grid cap, geometry and keep switches for one launch; restored after."""
  prev = C.cf32_wino_grid_cap(cap)
  pgeo = C.cf32_wino_geo(geo)
  pkeep = C.cf32_wino_keep(keep)
  try:
    C.cf32_wino_launch_info(True)
    yield
  finally:
    C.cf32_wino_grid_cap(prev)
    C.cf32_wino_geo(pgeo)
    C.cf32_wino_keep(pkeep)
    assert C.cf32_wino_grid_cap(-1) == prev


def _check_launch(C, plan, cap, case):
  """The last Winograd launch is `plan`, its grid cut to the cap; the direct
  launchers saw nothing."""
  info = C.cf32_wino_launch_info(True)
  exp = dict(plan)
  if cap:
    exp['grid'] = min(cap, plan['grid'])
  assert info == exp, (case, info, exp)
  if cap:
    assert info['grid'] == cap and info['nranges'] >= 2 * cap + 1
  assert C.cf32_wino_launch_info()['family'] == 'none'
  print('WINOREC launch %s cap=%d %s' % (case, cap, info))
  return info


def _no_conv_error(C, like):
  assert int(C.lstm_error_word(like)[1]) == 0


def _compare(out, ref, bnd, exact, family, case):
  assert tuple(out.shape) == tuple(ref.shape)
  if exact:
    assert torch.equal(O.d64(out), ref), case
  else:
    r = O.ratio(out, ref, bnd)
    _rec(family, case, r)
    assert r <= 1.0, (case, r)


# ----------------------------------------------------------------- forward

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('flags', sorted(Wn.FWD_FLAGS))
@pytest.mark.parametrize('name', Wn.fwd_cases())
def test_wino_forward(cuda, name, flags, exact):
  """cf32_conv_fwd, 16 -> 16 / 16 -> 32 / 32 -> 32: every instance map with
  compile-time and with runtime geometry, an odd map and the widest map the
  launcher takes, five flag sets (the residual ones with their compile-time
  flag instances)."""
  C = O.ext()
  d = Wn.fwd_data(name, exact)
  ref, A = Wn.fwd_ref(d, flags)
  bias, relu_in, add, relu_out = Wn.FWD_FLAGS[flags]
  x, w = O.embed(d['x'], cuda), d['w'].to(cuda)
  b = d['b'].to(cuda) if bias else None
  addt = O.embed(d['add'], cuda) if add else None
  for geo in (1, 0):
    plan = Wn.plan_fwd(d['N'], d['H'], d['W'], d['cin'], d['cout'], fl=Wn.FLAG_WORD[flags],
                       geo_on=bool(geo))
    assert plan is not None and plan['family'] != 'none'
    for cap in (0,) + d['caps']:
      case = 'fwd/%s/%s/geo%d/cap%d' % (name, flags, geo, cap)
      with _hooks(C, cap, geo=geo):
        C.cf32_launch_info(True)
        y = C.cf32_conv_fwd(x, w, b, 1, 1, 1, d['H'], d['W'], relu_in=relu_in, add=addt,
                            relu_out=relu_out)
        _check_launch(C, plan, cap, case)
        assert C.cf32_launch_info(True)['family'] == 'none'
      _compare(y, ref, Wn.bound_fwd(d['cin'], A), exact, 'wino_conv', case)
  _no_conv_error(C, x)


@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'mask_add'])
@pytest.mark.parametrize('name', Wn.DGRAD_CASES)
def test_wino_dgrad(cuda, name, masked, exact):
  """cf32_conv_dgrad (flipped, transposed weights), plain and with the x > 0
  mask and the residual add."""
  C = O.ext()
  d = Wn.dgrad_data(name, exact)
  ref, A = Wn.dgrad_ref(d, masked)
  dy, w = O.embed(d['dy'], cuda), d['w'].to(cuda)
  mask = O.embed(d['mask'], cuda) if masked else None
  add = O.embed(d['add'], cuda) if masked else None
  for geo in (1, 0):
    plan = Wn.plan_fwd(d['N'], d['H'], d['W'], d['cout'], d['cin'], flip=True, geo_on=bool(geo))
    for cap in (0,) + d['caps']:
      case = 'dgrad/%s/%s/geo%d/cap%d' % (name, 'mask' if masked else 'plain', geo, cap)
      with _hooks(C, cap, geo=geo):
        dx = C.cf32_conv_dgrad(dy, w, 1, 1, 1, d['H'], d['W'], mask=mask, add=add)
        _check_launch(C, plan, cap, case)
      _compare(dx, ref, Wn.bound_fwd(d['cout'], A), exact, 'wino_dgrad', case)
  _no_conv_error(C, dy)


# ------------------------------------------------------------- stage heads

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('name', sorted(Wn.POOL_CASES))
def test_wino_conv_pool(cuda, name, exact):
  """cf32_wino_conv_pool_fwd: pooled values and first-maximal-tap codes
  against float64 conv + pool.  Capped, a run's first range (k > 0) leaves its
  top-row part in `side`, interior ranges carry rows 4k+2, 4k+3 in registers
  and wino_pool_fix_kernel merges the run ends; uncapped every range is a run
  start.  Integer maps tie partially across exactly those merges."""
  C = O.ext()
  d = Wn.pool_data(name, exact)
  x, w, b = O.embed(d['x'], cuda), d['w'].to(cuda), d['b'].to(cuda)
  fam = d['plan']['family']
  for cap in (0,) + d['caps']:
    case = 'pool/%s/cap%d' % (name, cap)
    with _hooks(C, cap):
      out = C.cf32_wino_conv_pool_fwd(x, w, b, d['stages'])
      assert len(out) == 2, case
      _check_launch(C, d['plan'], cap, case)
    p, a = out[0], out[1].cpu().long()
    assert tuple(a.shape) == tuple(d['code'].shape)
    if exact:
      assert torch.equal(O.d64(p), d['val']), case
      assert torch.equal(a, d['code']), case
    else:
      r = O.ratio(p, d['val'], d['val_bound'])
      _rec(fam, case, r)
      assert r <= 1.0, (case, r)
      assert torch.equal(a[d['clear']], d['code'][d['clear']]), case
  _no_conv_error(C, x)


# --------------------------------------------------------- weight gradient

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('relu_in', [False, True], ids=['raw', 'relu_in'])
@pytest.mark.parametrize('hw', Wn.WGRAD_MAPS, ids=lambda s: '%dx%d' % s)
def test_wino_wgrad(cuda, hw, relu_in, exact):
  """cf32_conv_wgrad 32 -> 32: capped, fewer slots than ranges and each slot
  the sum of a run; two calls bitwise equal."""
  C = O.ext()
  d = Wn.wgrad_data(hw, relu_in, exact)
  x, dy = O.embed(d['x'], cuda), O.embed(d['dy'], cuda)
  plan = Wn.plan_wgrad(d['N'], *hw)
  for cap in (0,) + d['caps']:
    case = 'wgrad/%dx%d/relu%d/cap%d' % (hw + (int(relu_in), cap))
    outs = []
    for _ in range(2):
      dw, db = d['dw0'].to(cuda), d['db0'].to(cuda)
      with _hooks(C, cap):
        C.cf32_conv_wgrad(x, dy, 1, 1, 1, relu_in, dw, db)
        _check_launch(C, plan, cap, case)
      outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), case
    _compare(outs[0][0], d['rw'], Wn.bound_wg(d['M'], d['mw']), exact, 'wino_wgrad', case + '/dw')
    _compare(outs[0][1], d['rb'], Wn.bound_wg(d['Mb'], d['mb']), exact, 'wino_wgrad',
             case + '/db')
  _no_conv_error(C, x)


# ---------------------------------------------------------- fused backward

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('name', Wn.bwd_cases())
def test_wino_bwd_fused(cuda, name, exact):
  """cf32_conv_bwd_fused: dX, dW and db of every family, with compile-time and
  runtime geometry and the row-keeping stager on and off - each against the
  oracle, not only against each other.  Capped runs are the regime in which
  rows are kept from one range to the next."""
  C = O.ext()
  d = Wn.bwd_data(name, exact)
  x, dy, w = O.embed(d['x'], cuda), O.embed(d['dy'], cuda), d['w'].to(cuda)
  add = O.embed(d['add'], cuda) if d['add'] is not None else None
  fused32 = Wn.bwd_family(name) != 'wino_bwd16'
  for geo, keep in ((1, 1), (0, 1)) + (((1, 0),) if fused32 else ()):
    plan = dict(Wn.plan_bwd(d['N'], d['H'], d['W'], d['cx'], d['cy'], d['relu'], d['mask'],
                            geo_on=bool(geo)), family=Wn.bwd_family(name, bool(keep)))
    for cap in (0,) + d['caps']:
      case = 'bwd/%s/geo%d/keep%d/cap%d' % (name, geo, keep, cap)
      dw, db = d['dw0'].to(cuda), d['db0'].to(cuda)
      with _hooks(C, cap, geo=geo, keep=keep):
        n0 = C.cf32_wino_keep_launches()
        dx = C.cf32_conv_bwd_fused(dy, w, x, d['relu'], dw, db, add=add, mask=d['mask'])
        _check_launch(C, plan, cap, case)
        assert C.cf32_wino_keep_launches() - n0 == int(plan['family'] == 'wino_bwd32_keep')
      fam = plan['family']
      _compare(dx, d['dx'], Wn.bound_fwd(d['cy'], d['mdx']), exact, fam, case + '/dx')
      _compare(dw, d['rw'], Wn.bound_wg(d['M'], d['mw']), exact, fam, case + '/dw')
      _compare(db, d['rb'], Wn.bound_wg(d['Mb'], d['mb']), exact, fam, case + '/db')
      _no_conv_error(C, x)


# ------------------------------------------------------- uncapped launches

def test_uncapped_wino_launches_match_hand_arithmetic(cuda):
  """The production shapes (a 32-frame chunk of each ladder), cap 0: the hook
  equals run_wino_* redone by hand (literals asserted on the CPU in
  test_wino_oracle.py)."""
  C = O.ext()
  assert C.cf32_wino_grid_cap(-1) == 0
  N = 32
  z = lambda *s: torch.zeros(*s, device=cuda)
  for cin, cout, H, W in [(16, 16, 36, 48), (16, 32, 36, 48), (32, 32, 18, 24), (32, 32, 9, 12),
                          (16, 16, 42, 42), (32, 32, 21, 21), (32, 32, 11, 11),
                          (16, 16, 36, 64), (32, 32, 18, 32), (32, 32, 9, 16)]:
    x, w, b = z(N, H, W, cin), z(3, 3, cin, cout), z(cout)
    C.cf32_wino_launch_info(True)
    C.cf32_conv_fwd(x, w, b, 1, 1, 1, H, W, relu_in=True, relu_out=True)
    _check_launch(C, Wn.plan_fwd(N, H, W, cin, cout, fl=19), 0, 'hand/fwd')
    dy, dw, db = z(N, H, W, cout), z(3, 3, cin, cout), z(cout)
    if cin == cout:
      C.cf32_conv_dgrad(dy, w, 1, 1, 1, H, W)
      _check_launch(C, Wn.plan_fwd(N, H, W, cout, cin, flip=True), 0, 'hand/dgrad')
    if cin == 32:
      C.cf32_conv_wgrad(x, dy, 1, 1, 1, True, dw, db)
      _check_launch(C, Wn.plan_wgrad(N, H, W), 0, 'hand/wgrad')
    for relu, mask in ((True, True), (False, False)):
      C.cf32_conv_bwd_fused(dy, w, x, relu, dw, db, mask=mask)
      info = C.cf32_wino_launch_info(True)
      plan = Wn.plan_bwd(N, H, W, cin, cout, relu, mask)
      keep = plan['family'] == 'wino_bwd32' and Wn.keep_expected(N, H, W, cin, cout)
      assert info == dict(plan, family='wino_bwd32_keep' if keep else plan['family']), info
  for cin, cout, H, W, stages in [(16, 32, 36, 48, 7), (16, 32, 36, 64, 7), (16, 32, 42, 42, 15),
                                  (4, 16, 72, 96, 7), (4, 16, 72, 128, 7), (4, 16, 84, 84, 7)]:
    out = C.cf32_wino_conv_pool_fwd(z(N, H, W, cin), z(3, 3, cin, cout), z(cout), stages)
    assert len(out) == 2
    _check_launch(C, Wn.plan_pool(N, H, W, cin, cout), 0, 'hand/pool')
  out = C.cf32_wino_conv_pool_fwd(z(N, 18, 24, 32), z(3, 3, 32, 32), z(32), 7)
  assert len(out) == 2
  _check_launch(C, Wn.plan_pool_img(N, 18, 24, 32, 32), 0, 'hand/pool_img')
  _no_conv_error(C, out[0])
