"""The direct (non-Winograd) fp32 conv kernels of csrc/kernels/conv_f32.hip
against the float64 oracles of tests/_conv_f32_oracle.py, with every
persistent workgroup walking several tiles.

conv_fwd_kernel, conv_pool_fwd_kernel, conv_wgrad_kernel and
pool_wgrad_kernel are persistent: a workgroup walks tiles blockIdx.x,
blockIdx.x + gridDim.x, ..., prefetching the next tile into registers while
the current one computes.  At the N = 2..9 images a quick test can afford the
launchers give every workgroup ONE tile, so each multi-tile case runs
  * uncapped (one tile per workgroup: the control), and
  * with cf32_grid_cap(3): ntiles >= 7 and ntiles % 3 != 0, so every
    workgroup runs two or three tiles and the last sweep is ragged.
Where the launcher cuts an image into a multiple of 3 tiles, ntiles % 3 != 0
has no solution in N; those cases run on 3 workgroups AND on 4 (or 5), where
N leaves a remainder (_conv_f32_oracle.caps_and_n).

Every case asserts its path and launch shape from cf32_launch_info against
the launch arithmetic redone in the oracle module (so with the cap at 0 the
hooks change no launch), reads its inputs from the slice buf[1:1+N] of a
NaN-filled batch, starts dW / db from non-zero values and restores the hooks
in `finally`.

Regimes (derivations in the oracle module): integer inputs, where the result
must EQUAL the float64 oracle for any tile split, slot count or order
(torch.equal), and random normal inputs under the elementwise bound
(M + 5) 2^-24 A; the largest error / bound ratio of each case is printed as
a CF32REC line.

Short tiles and ragged groups (forward): a last tile of fewer than R rows
comes from the 8x8/4 layer at 72x96 (R = 4, last 2), 4x4/2 at 21x21 (4, 3)
and 32-channel 3x3/1 at 18x24 (8, 2); a last 16-pixel group with fewer than
16 pixels from 8x8/4 at 84x84 (63 pixels per tile), 4x4/2 at 18x24 (36) and
21x21 (44 / 33), 3x3/2 at 9x12 (30) and 11x11 (18) and the 7x9 / 11x11 maps.
The lists are FWD_SHORT_TILE / FWD_RAGGED_GROUP, checked on the CPU.

Switches read once per process run in one child pytest per setting
(test_switch_children); the cases they select assert their path from the
environment, so the same test checks the default path in this process.

Not reachable in a production build, so not covered: conv_fwd instances
<32,32,4,2> and <64,32,3,2> (cout_tile gives 16-wide tiles for these weight
slices; SA_F32_COUT_T is a measure_knob), and the Winograd instances behind
SA_WINO_CFG / SA_WINO_WG_ALL.  The direct 3x3/1 32 -> 32 weight gradient
behind SA_F32_WINO_WG IS covered, at 7x9, which the Winograd launcher
declines (a 64-tile range would touch more than 4 images), as are the
16/32-channel 3x3/1 forward and data-gradient instances there.
"""

import contextlib
import os
import subprocess
import sys

import pytest
import torch

from tests import _conv_f32_oracle as O

pytestmark = pytest.mark.gpu

REGIMES = [True, False]
REGIME_IDS = ['exact', 'rounding']
_REC = {}


def _rec(family, case, r):
  _REC[family] = max(_REC.get(family, 0.0), r)
  print('CF32REC %s %s ratio=%.3e family_max=%.3e' % (family, case, r, _REC[family]))


@contextlib.contextmanager
def _grid_cap(C, cap):
  prev = C.cf32_grid_cap(cap)
  try:
    yield
  finally:
    C.cf32_grid_cap(prev)
    assert C.cf32_grid_cap(-1) == prev


def _check_launch(C, plan, cap, case):
  """The last direct launch is `plan` (grid_x cut to the cap)."""
  info = C.cf32_launch_info(True)
  exp = dict(plan)
  if cap:
    exp['grid_x'] = min(cap, plan['grid_x'])
  assert info == exp, (case, info, exp)
  if cap:
    assert info['ntiles'] > info['grid_x']
    assert info['ntiles'] >= 2 * info['grid_x'] + 1
  print('CF32REC launch %s cap=%d %s' % (case, cap, info))
  assert C.cf32_launch_info()['family'] == 'none'
  return info


def _compare(out, ref, A, M, exact, family, case):
  assert tuple(out.shape) == tuple(ref.shape)
  if exact:
    assert torch.equal(O.d64(out), ref), case
  else:
    r = O.ratio(out, ref, O.bound(M, A))
    _rec(family, case, r)
    assert r <= 1.0, (case, r)


def _wino_off():
  return os.environ.get('SA_F32_WINO', '') == '0'


# ----------------------------------------------------------------- forward

def _forward_case(cuda, table_direct, name, flags, exact):
  C = O.ext()
  d = O.fwd_data(name, exact)
  ref, A = O.fwd_ref(d, flags)
  bias, relu_in, add, relu_out = O.FWD_FLAGS[flags]
  relu_in = relu_in and not d['u8']
  x, w = O.embed(d['x'], cuda), d['w'].to(cuda)
  b = d['b'].to(cuda) if bias else None
  addt = O.embed(d['add'], cuda) if add else None
  for cap in (0,) + d['caps']:
    case = 'fwd/%s/%s/cap%d' % (name, flags, cap)
    with _grid_cap(C, cap):
      C.cf32_launch_info(True)
      y = C.cf32_conv_fwd(x, w, b, d['S'], d['pt'], d['pl'], d['Ho'], d['Wo'],
                          relu_in=relu_in, add=addt, relu_out=relu_out)
      if table_direct:
        _check_launch(C, d['plan'], cap, case)
      else:  # the Winograd kernels took it
        assert C.cf32_launch_info(True)['family'] == 'none'
    _compare(y, ref, A, d['M'], exact, 'conv_fwd', case)


@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('flags', sorted(O.FWD_FLAGS))
@pytest.mark.parametrize('name', sorted(O.FWD_CASES))
def test_conv_fwd_direct(cuda, name, flags, exact):
  _forward_case(cuda, True, name, flags, exact)


@pytest.mark.parametrize('flags', sorted(O.FWD_FLAGS))
@pytest.mark.parametrize('name', sorted(O.WINO_OFF_CASES))
def test_wino_off_fwd(cuda, name, flags):
  """3x3/1 16/32-channel shapes, exact regime: the direct instances under
  SA_F32_WINO=0 (child process), the Winograd kernels otherwise - integer
  data is exact through the Winograd transforms too (quarters of integers)."""
  _forward_case(cuda, _wino_off(), name, flags, True)


# ----------------------------------------------------------- data gradient

def _dgrad_case(cuda, direct, name, masked, exact):
  C = O.ext()
  d = O.dgrad_data(name, exact, O.dgrad_mode())
  ref, A = O.dgrad_ref(d, masked)
  dy, w = O.embed(d['dy'], cuda), d['w'].to(cuda)
  mask = O.embed(d['mask'], cuda) if masked else None
  add = O.embed(d['add'], cuda) if masked else None
  kw = {}
  if d['pooled']:
    kw = dict(pool_arg=O.embed(d['code'].to(torch.uint8), cuda),
              pool_pbh=O.same_pads(d['H'], 3, 2)[0], pool_pbw=O.same_pads(d['W'], 3, 2)[0])
  for cap in (0,) + d['caps']:
    case = 'dgrad/%s/%s/%s/cap%d' % (name, O.dgrad_mode(), 'mask' if masked else 'plain', cap)
    with _grid_cap(C, cap):
      C.cf32_launch_info(True)
      dx = C.cf32_conv_dgrad(dy, w, d['S'], d['pt'], d['pl'], d['H'], d['W'], mask=mask,
                             add=add, **kw)
      if direct:
        _check_launch(C, d['plan'], cap, case)
      else:
        assert C.cf32_launch_info(True)['family'] == 'none'
    _compare(dx, ref, A, d['M'], exact, 'conv_dgrad', case)


@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'mask_add'])
@pytest.mark.parametrize('name', sorted(O.DGRAD_CASES))
def test_conv_dgrad_direct(cuda, name, masked, exact):
  """Stride 2: the phase-decomposed form by default (2x2 sub-kernels,
  strided output placement); the phase-stacked and dilated forms in the
  SA_F32_DGRAD_STACK=1 / SA_F32_DGRAD_PHASE=0 children."""
  _dgrad_case(cuda, True, name, masked, exact)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'mask_add'])
@pytest.mark.parametrize('name', sorted(O.WINO_OFF_DGRAD))
def test_wino_off_dgrad(cuda, name, masked):
  _dgrad_case(cuda, _wino_off(), name, masked, True)


# --------------------------------------------------------- fused conv+pool

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('name', sorted(O.POOL_CASES))
def test_conv_pool_fwd_direct(cuda, name, exact):
  """Pooled values and first-tap argmax codes; two or more tiles per image,
  so with the cap every workgroup recomputes seam rows between its tiles."""
  C = O.ext()
  d = O.pool_data(name, exact)
  x, w, b = O.embed(d['x'], cuda), d['w'].to(cuda), d['b'].to(cuda)
  for cap in (0,) + d['caps']:
    case = 'pool/%s/cap%d' % (name, cap)
    with _grid_cap(C, cap):
      C.cf32_launch_info(True)
      p, a = C.cf32_conv_pool_fwd(x, w, b, d['pbh'], d['pbw'])
      info = _check_launch(C, d['plan'], cap, case)
      assert info['tiles_per_img'] >= 2
    a = a.cpu().long()
    assert tuple(a.shape) == tuple(d['code'].shape)
    if exact:
      assert torch.equal(O.d64(p), d['val']), case
      assert torch.equal(a, d['code']), case
    else:
      r = O.ratio(p, d['val'], d['val_bound'])
      _rec('conv_pool_fwd', case, r)
      assert r <= 1.0, (case, r)
      assert torch.equal(a[d['clear']], d['code'][d['clear']]), case


# --------------------------------------------------------- weight gradient

def _wgrad_call(C, d, dev, dw, db):
  kw = {}
  if d['pooled']:
    kw = dict(pool_arg=d['_code'], pool_pbh=O.same_pads(d['H'], 3, 2)[0],
              pool_pbw=O.same_pads(d['W'], 3, 2)[0])
  C.cf32_conv_wgrad(d['_x'], d['_dy'], d['S'], d['pt'], d['pl'], d['relu_in'], dw, db, **kw)


def _wgrad_inputs(name, exact, dev):
  d = dict(O.wgrad_data(name, exact, O.scatter_on()))
  d['_x'], d['_dy'] = O.embed(d['x'], dev), O.embed(d['dy'], dev)
  d['_code'] = O.embed(d['code'].to(torch.uint8), dev) if d['pooled'] else None
  return d


@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('name', sorted(O.WGRAD_CASES))
def test_conv_wgrad_direct(cuda, name, exact):
  """Every reachable SA_WG_CASE, relu_in, dw_cin = 3 into the 4-channel
  image, the pool_arg GATHER forms and the stage-0 scatter kernel (stage0_*:
  pool_wgrad by default, conv_wgrad's GATHER instance with
  SA_F32_POOL_SCATTER=0).  Capped: fewer slots than tiles, each slot sums
  several tiles; two runs bitwise equal."""
  C = O.ext()
  d = _wgrad_inputs(name, exact, cuda)
  if name.startswith('stage0'):
    assert d['plan']['family'] == ('pool_wgrad' if O.scatter_on() else 'conv_wgrad')
  for cap in (0,) + d['caps']:
    case = 'wgrad/%s/cap%d' % (name, cap)
    outs = []
    with _grid_cap(C, cap):
      for _ in range(2):
        dw, db = d['dw0'].to(cuda), d['db0'].to(cuda)
        C.cf32_launch_info(True)
        _wgrad_call(C, d, cuda, dw, db)
        info = _check_launch(C, d['plan'], cap, case)
        if cap:
          assert info['grid_x'] == cap < info['ntiles']  # the slot count
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    _compare(outs[0][0], d['rw'], d['mw'], d['M'], exact, d['plan']['family'], case + '/dw')
    _compare(outs[0][1], d['rb'], d['mb'], d['M'], exact, d['plan']['family'], case + '/db')


DEFER_JOBS = ['s3_9x12', 's2_21x21', 'r16_36x48', 'stage0_f32_72x96', 'pool_h32_18x24',
              'd1_u8c3_72x96']


@pytest.mark.parametrize('njobs', [len(DEFER_JOBS), 18], ids=['one_launch', 'past_kMaxJobs'])
@pytest.mark.parametrize('cap', [0, 3])
def test_deferred_wgrad_reductions(cuda, njobs, cap):
  """Several different weight gradients queued under cf32_wgrad_defer and
  summed by one cf32_wgrad_flush (wgrad_reduce_multi_kernel; 18 jobs: two
  launches, kMaxJobs = 16 each) are bitwise the immediate reductions, and
  within the bound of the float64 oracle."""
  C = O.ext()
  jobs = [_wgrad_inputs(DEFER_JOBS[i % len(DEFER_JOBS)], False, cuda) for i in range(njobs)]
  def run():
    outs = []
    for d in jobs:
      dw, db = d['dw0'].to(cuda), d['db0'].to(cuda)
      _wgrad_call(C, d, cuda, dw, db)
      outs.append((dw, db))
    return outs
  with _grid_cap(C, cap):
    now = run()
    try:
      C.cf32_wgrad_defer(True)
      later = run()
      # nothing summed yet: the outputs still hold their starting values
      assert all(torch.equal(dw, d['dw0'].to(cuda)) for (dw, _), d in zip(later, jobs))
      assert C.cf32_wgrad_flush() == njobs
    finally:
      C.cf32_wgrad_defer(False)
    assert C.cf32_wgrad_flush() == 0
  for i, ((dw, db), (dw2, db2), d) in enumerate(zip(now, later, jobs)):
    assert torch.equal(dw, dw2) and torch.equal(db, db2), i
    _compare(dw2, d['rw'], d['mw'], d['M'], False, 'wgrad_flush', 'defer/%d/cap%d/dw' % (i, cap))
    _compare(db2, d['rb'], d['mb'], d['M'], False, 'wgrad_flush', 'defer/%d/cap%d/db' % (i, cap))


# ---------------------------------------------------------------- max-pool

@pytest.mark.parametrize('exact', REGIMES, ids=REGIME_IDS)
@pytest.mark.parametrize('C_', O.MAXPOOL_CHANNELS)
@pytest.mark.parametrize('shape', O.MAXPOOL_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_maxpool_direct(cuda, shape, C_, exact):
  """Values (exact in both regimes), first-tap codes (integer data: tied
  windows) and the gradient.  Even maps take maxpool_bwd_blk_kernel, or
  maxpool_bwd_kernel with SA_F32_POOL_BWD_BLK=0: both equal the oracle on
  integer data, hence each other bitwise."""
  C = O.ext()
  d = O.maxpool_data(shape, C_, exact)
  y, arg = C.cf32_maxpool_fwd(O.embed(d['x'], cuda), d['pbh'], d['pbw'])
  assert torch.equal(O.d64(y), d['val'])
  assert torch.equal(arg.cpu().long(), d['code'])
  C.cf32_launch_info(True)
  dx = C.cf32_maxpool_bwd(O.embed(d['dy'], cuda), O.embed(d['code'].to(torch.uint8), cuda),
                          d['H'], d['W'], d['pbh'], d['pbw'])
  blk = (d['H'] % 2 == 0 and d['W'] % 2 == 0 and
         os.environ.get('SA_F32_POOL_BWD_BLK', '') != '0')
  fam = C.cf32_launch_info(True)['family']
  assert fam == ('maxpool_bwd_blk' if blk else 'maxpool_bwd')
  # at most four windows per position
  _compare(dx, d['dx'], d['dxmag'], 4, exact, fam, 'maxpool/%dx%dx%d/C%d' % (shape + (C_,)))


# ---------------------------------------------------------------- the rest

@pytest.mark.parametrize('n', [4, 4096 * 256 * 4 + 4], ids=['n4', 'past_one_sweep'])
def test_relu_mask(cuda, n):
  """dy *= (ref > 0): -0.0 and NaN in ref are not > 0; n past one sweep of
  the 4096-block grid."""
  C = O.ext()
  g = O.gen(n)
  dy = torch.randn(n, generator=g)
  ref = torch.randn(n, generator=g)
  ref[0], ref[1], ref[-1], ref[-2] = -0.0, float('nan'), float('nan'), -0.0
  ref[2] = 0.0
  want = torch.where(ref > 0, dy, torch.zeros_like(dy))
  out = dy.to(cuda)
  C.cf32_relu_mask_(out, ref.to(cuda))
  assert torch.equal(out.cpu(), want)
  assert float(out[0]) == 0 and float(out[1]) == 0 and float(out[-1]) == 0


def test_frames_family(cuda):
  """frames_f32_tile_kernel by default, frames_f32_kernel under
  SA_FRAMES_TILE=0; both exact table look-ups."""
  C = O.ext()
  fr = O.frames(O.gen(5), (3, 5, 7, 3), False).to(cuda)
  C.cf32_launch_info(True)
  y = C.cf32_frames_f32(fr).cpu()
  tiled = os.environ.get('SA_FRAMES_TILE', '') != '0'
  assert C.cf32_launch_info(True)['family'] == ('frames_tile' if tiled else 'frames')
  table = (torch.arange(256, dtype=torch.float64) / 255.0).float()
  assert torch.equal(y[..., :3], table[fr.cpu().long()]) and float(y[..., 3].abs().max()) == 0


@pytest.mark.parametrize('C_', [16, 32])
def test_bwd_fused_switch(cuda, C_):
  """cf32_conv_bwd_fused on integer data: the fused Winograd backward by
  default; with SA_F32_FUSED_BWD=0 and SA_F32_WINO=0 the direct weight and
  data gradient kernels.  Either way equal to the oracle."""
  C = O.ext()
  g = O.gen(C_)
  N, H, W = 4, 18, 24
  x, dy = O.acts(g, (N, H, W, C_), True), O.acts(g, (N, H, W, C_), True)
  w = O.weights(g, (3, 3, C_, C_), True)
  dw, db = torch.ones(3, 3, C_, C_, device=cuda), torch.ones(C_, device=cuda)
  C.cf32_launch_info(True)
  dx = C.cf32_conv_bwd_fused(O.embed(dy, cuda), w.to(cuda), O.embed(x, cuda), True, dw, db,
                             mask=True)
  direct = _wino_off() and os.environ.get('SA_F32_FUSED_BWD', '') == '0'
  fam = C.cf32_launch_info(True)['family']
  # default: the fused kernel (or, where it declines a map, its Winograd /
  # direct-wgrad fallback); switched off: the direct data gradient runs last
  assert (fam == 'conv_fwd') == direct
  gx = O.conv_dgrad(dy.double(), w.double(), 1, H, W, mask=x.double())
  rw, rb = O.conv_wgrad(x.double().clamp(min=0), dy.double(), 3, 1)
  assert torch.equal(O.d64(dx), gx)
  assert torch.equal(O.d64(dw), rw + 1) and torch.equal(O.d64(db), rb + 1)


def test_uncapped_launches_match_hand_arithmetic(cuda):
  """The launch shapes of the direct kernels for the shapes of
  test_conv_f32_gpu.SHAPES, cap 0, equal run_conv / run_wgrad redone by hand
  (the literals are asserted on the CPU in test_conv_f32_oracle.py)."""
  C = O.ext()
  assert C.cf32_grid_cap(-1) == 0
  # (N, H, W, Cin, Cout, K, S, uint8)
  for N, H, W, Cin, Cout, K, S, u8 in [(3, 72, 96, 3, 32, 8, 4, True),
                                      (3, 18, 24, 32, 64, 4, 2, False),
                                      (3, 9, 12, 64, 128, 3, 2, False),
                                      (3, 72, 96, 3, 16, 3, 1, True),
                                      (2, 84, 84, 4, 32, 8, 4, True),
                                      (2, 21, 21, 32, 64, 4, 2, False),
                                      (2, 11, 11, 64, 128, 3, 2, False),
                                      (2, 72, 128, 3, 16, 3, 1, True),
                                      (3, 36, 48, 16, 32, 3, 1, False),
                                      (3, 36, 48, 16, 16, 3, 1, False)]:
    g = O.gen(H)
    x, _ = O.source(g, N, H, W, Cin, u8, True)
    w = O.weights(g, (K, K, Cin, Cout), True).to(cuda)
    Ho, Wo = O.same_out(H, S), O.same_out(W, S)
    pt, pl = O.same_pads(H, K, S)[0], O.same_pads(W, K, S)[0]
    cinp = 4 if u8 else Cin
    if Cin not in (16, 32) or K != 3:
      C.cf32_launch_info(True)
      C.cf32_conv_fwd(x.to(cuda), w, None, S, pt, pl, Ho, Wo)
      _check_launch(C, O.plan_conv(N, Ho, Wo, cinp, Cout, K, S), 0, 'hand/fwd')
    dw = torch.zeros_like(w)
    C.cf32_launch_info(True)
    C.cf32_conv_wgrad(x.to(cuda), torch.zeros(N, Ho, Wo, Cout, device=cuda), S, pt, pl, False,
                      dw, None)
    _check_launch(C, O.plan_wgrad(N, Ho, Wo, cinp, Cout, K, S), 0, 'hand/wgrad')


# ---------------------------------------------- switches read once per process

CHILDREN = {
    'wino_off': ({'SA_F32_WINO': '0', 'SA_F32_FUSED_BWD': '0'}, [],
                 'test_wino_off or test_bwd_fused_switch'),
    'pool_scatter_off': ({'SA_F32_POOL_SCATTER': '0'}, [],
                         'test_conv_wgrad_direct and stage0'),
    'pool_bwd_blk_off': ({'SA_F32_POOL_BWD_BLK': '0'}, [], 'test_maxpool_direct'),
    'frames_tile_off': ({'SA_FRAMES_TILE': '0'}, ['test_conv_f32_gpu.py'],
                        'test_frames_f32_is_exact_division or test_frames_family'),
    'dgrad_stack': ({'SA_F32_DGRAD_STACK': '1'}, [],
                    'test_conv_dgrad_direct and (s2_ or s3_)'),
    'dgrad_dilated': ({'SA_F32_DGRAD_PHASE': '0'}, [],
                      'test_conv_dgrad_direct and (s2_ or s3_)'),
}


@pytest.mark.parametrize('child', sorted(CHILDREN))
def test_switch_children(cuda, child):
  """One child pytest per setting (the extension reads each switch once per
  process); the selected cases assert their path from the environment."""
  env, extra, expr = CHILDREN[child]
  here = os.path.dirname(os.path.abspath(__file__))
  root = os.path.dirname(here)
  files = [os.path.join(here, f) for f in extra] + [os.path.abspath(__file__)]
  r = subprocess.run(
      [sys.executable, '-m', 'pytest', '-q', '-s', '-p', 'no:cacheprovider'] + files +
      ['-k', expr],
      capture_output=True, text=True, timeout=600, cwd=root,
      env=dict(os.environ, PYTHONPATH=root, **env))
  print('\n'.join(l for l in r.stdout.splitlines() if l.startswith('CF32REC') and
                  'launch' not in l))
  assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
  assert ' passed' in r.stdout and ' failed' not in r.stdout and ' skipped' not in r.stdout
