"""The bf16 conv torso's persistent tile loop against a float64 oracle.

Every kernel of csrc/kernels/conv_torso.hip is persistent: a workgroup walks
several tiles (TileIter, XCD-contiguous ranges), prefetching tile k+1 while
tile k computes and carrying its weight-gradient accumulators across tiles.
test_conv_gpu.py launches at most 27 tiles, one per workgroup.  Here the grid
is shrunk to about 128 workgroups (small_grid) and the batch is chosen from
the launch record so that workgroups run a second and a third tile, with
ranges that cross image boundaries and fractional XCD range bounds:

  * float64 CPU oracle with the derived elementwise bound of _conv_oracle.py
    (conv1 converts fp32 weights in the kernel: the suite's max-norm bounds);
  * schedule independence: the big launch is BITWISE equal to the same
    images run in slices small enough for one tile per workgroup;
  * weight gradients against float64 (1e-3 max) and the slices' sum (1e-4),
    accumulated into non-zero dW / db, atomic and deterministic flush.

Each launch under test asserts from conv_launch_info() that ntiles > grid
(== for the control) and that the expected kind of kernel ran.
"""

import pytest
import torch

from tests import _conv_oracle as O

pytestmark = pytest.mark.gpu

MODES = ['one', 'plus', 'x2.4']


def bf16(t):
  return t.to(torch.bfloat16)


def rnd(g, *shape, scale=1.0):
  return torch.randn(*shape, generator=g) * scale


def seed_of(*key):
  return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def plan(C, family, probe, mode):
  """(N, slice size) for `mode`, from a one-image probe launch's record."""
  probe()
  rec = O.record(C, family)
  tpi, gmax = rec['ntiles'], rec['grid_max']
  assert rec['grid'] == tpi and gmax >= 8
  return O.pick_n(tpi, gmax, mode), max(gmax // tpi, 1)


def check_launch(C, family, tag, mode, compiled):
  rec = O.record(C, family, tag + ' ' + mode)
  if mode == 'one':
    assert rec['ntiles'] == rec['grid'], rec
  else:
    assert rec['ntiles'] > rec['grid'], rec
  assert rec['specialized'] == compiled, rec
  return rec


def check_slice(C, family):
  rec = O.record(C, family)
  assert rec['ntiles'] == rec['grid'], rec


# ----------------------------------------------------------------- forward

# C, H, W, resid, post, relu_in (the forms the torso uses), specialize knob
RES_FWD = [
    (16, 36, 48, False, True, True, 1), (16, 36, 48, True, False, False, 1),
    (32, 18, 24, True, True, False, 1), (32, 18, 24, False, True, True, 0),
    (32, 9, 12, True, False, False, 1), (32, 21, 21, False, True, True, 1),
    (32, 11, 11, True, True, False, 1), (16, 10, 14, True, False, False, 1),
    (32, 7, 5, False, True, True, 1)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('Cc,H,W,resid,post,relu_in,spec', RES_FWD)
def test_res_conv_fwd(cuda, Cc, H, W, resid, post, relu_in, spec, mode):
  C = O.ext()
  fam = 'res_conv_fwd'
  g = torch.Generator().manual_seed(seed_of(1, Cc, H, W, resid, post, spec))
  w = bf16(rnd(g, 3, 3, Cc, Cc, scale=0.1)).float()
  b = rnd(g, Cc, scale=0.1)
  wd, bd = w.to(cuda), b.to(cuda)
  compiled = bool(spec) and O.is_compiled(fam, Cc, H, W)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, Cc, device=cuda, dtype=torch.bfloat16)
    N, ns = plan(C, fam, lambda: C.res_conv_fwd(one, wd, bd, None, post, relu_in),
                 mode)
    x = bf16(rnd(g, N, H, W, Cc))
    r = bf16(rnd(g, N, H, W, Cc)) if resid else None
    xd = x.to(cuda)
    rd = r.to(cuda) if resid else None
    y = C.res_conv_fwd(xd, wd, bd, rd, post, relu_in)
    check_launch(C, fam, '%dx%d C%d' % (H, W, Cc), mode, compiled)
    parts = []
    for s in range(0, N, ns):
      parts.append(C.res_conv_fwd(xd[s:s + ns], wd, bd,
                                  rd[s:s + ns] if resid else None, post, relu_in))
      check_slice(C, fam)
    O.bits_equal(y, torch.cat(parts), 'y vs one-tile-per-workgroup slices')
  xin = O.d64(x).relu() if relu_in else O.d64(x)
  ref = O.conv64(xin, O.d64(w), O.d64(b))
  A = O.conv64(xin.abs(), O.d64(w).abs(), O.d64(b).abs())
  if resid:
    ref, A = ref + O.d64(r), A + O.d64(r).abs()
  if post:
    ref = ref.relu()
  O.check_bound(y, ref, A, Cc, 'res_conv_fwd %dx%d C%d %s' % (H, W, Cc, mode))


RES_BLOCK = [(16, 36, 48, False, 1), (32, 18, 24, False, 1), (32, 9, 12, True, 1),
             (32, 21, 21, False, 1), (32, 11, 11, True, 1), (16, 10, 14, False, 1),
             (32, 7, 5, True, 1), (16, 36, 48, True, 0)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('Cc,H,W,last,spec', RES_BLOCK)
def test_res_block_fwd(cuda, Cc, H, W, last, spec, mode):
  C = O.ext()
  fam = 'res_block_fwd'
  g = torch.Generator().manual_seed(seed_of(2, Cc, H, W, last, spec))
  w1 = bf16(rnd(g, 3, 3, Cc, Cc, scale=0.1)).float()
  w2 = bf16(rnd(g, 3, 3, Cc, Cc, scale=0.1)).float()
  b1, b2 = rnd(g, Cc, scale=0.1), rnd(g, Cc, scale=0.1)
  dev = [t.to(cuda) for t in (w1, b1, w2, b2)]
  compiled = bool(spec) and O.is_compiled(fam, Cc, H, W)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, Cc, device=cuda, dtype=torch.bfloat16)
    N, ns = plan(C, fam, lambda: C.res_block_fwd(one, *dev, last), mode)
    x = bf16(rnd(g, N, H, W, Cc))
    xd = x.to(cuda)
    t, y = C.res_block_fwd(xd, *dev, last)
    check_launch(C, fam, '%dx%d C%d' % (H, W, Cc), mode, compiled)
    tp, yp = [], []
    for s in range(0, N, ns):
      ti, yi = C.res_block_fwd(xd[s:s + ns], *dev, last)
      check_slice(C, fam)
      tp.append(ti)
      yp.append(yi)
    O.bits_equal(t, torch.cat(tp), 't vs slices')
    O.bits_equal(y, torch.cat(yp), 'y vs slices')
  x64 = O.d64(x)
  tref = O.conv64(x64.relu(), O.d64(w1), O.d64(b1)).relu()
  tA = O.conv64(x64.relu(), O.d64(w1).abs(), O.d64(b1).abs())
  tag = '%dx%d C%d %s' % (H, W, Cc, mode)
  O.check_bound(t, tref, tA, Cc, 'res_block_fwd.t ' + tag)
  # conv2 reads the bf16 t the kernel stored: its oracle starts from that t
  t64 = O.d64(t)
  yref = O.conv64(t64, O.d64(w2), O.d64(b2)) + x64
  yA = O.conv64(t64.abs(), O.d64(w2).abs(), O.d64(b2).abs()) + x64.abs()
  if last:
    yref = yref.relu()
  O.check_bound(y, yref, yA, Cc, 'res_block_fwd.y ' + tag)


def pooled_bound_check(pooled, arg, y64, A, K, pb_h, pb_w, what, conv1_tol=None):
  """pooled against the float64 max-pool, |err| <= 2^-8 |ref| + 9 K 2^-23 Awin:
  the rounding to bf16 is monotone, so pooled = bf16(max of the fp32 taps);
  every fp32 tap is within 9 K 2^-23 A of its float64 value, so the fp32 max
  is within Awin-scaled accumulation error (Awin = the window's largest A) of
  the float64 max; the one rounding adds at most 2^-8 of the pooled value
  itself.  Only the accumulation term takes the window's maximum.  arg,
  decoded without clamping, must lie inside the image and name a tap within
  twice that tolerance of its window's float64 max."""
  N, H, W, _ = y64.shape
  ref, _ = O.pool64(y64, pb_h, pb_w)
  if conv1_tol is None:
    Awin = O.pool_taps(A, pb_h, pb_w, fill=0.0).max(dim=-1).values
    O.check_bound(pooled, ref, Awin, K, what)
    tol = O.REL * ref.abs() + 9 * K * O.ACC * Awin
  else:
    O.check_max(pooled, ref, conv1_tol, what)
    tol = torch.full_like(ref, conv1_tol * float(ref.abs().max()))
  r, c = O.tap_positions(arg, H, W, pb_h, pb_w)
  n = torch.arange(N).view(N, 1, 1, 1).expand_as(r)
  ch = torch.arange(y64.shape[3]).view(1, 1, 1, -1).expand_as(r)
  picked = y64[n, r, c, ch]
  assert bool((picked >= ref - 2 * tol).all()), what + ': argmax is not a maximal tap'


# CIN, COUT, H, W, specialize knob
POOL = [(16, 32, 36, 48, 1), (32, 32, 18, 24, 1), (32, 32, 21, 21, 1),
        (16, 16, 10, 14, 1), (32, 32, 7, 5, 1), (16, 32, 36, 48, 0)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('CIN,COUT,H,W,spec', POOL)
def test_conv_pool_fwd(cuda, CIN, COUT, H, W, spec, mode):
  C = O.ext()
  fam = 'conv_pool_fwd'
  g = torch.Generator().manual_seed(seed_of(3, CIN, COUT, H, W, spec))
  w = bf16(rnd(g, 3, 3, CIN, COUT, scale=0.1)).float()
  b = rnd(g, COUT, scale=0.1)
  wd, bd = w.to(cuda), b.to(cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  compiled = bool(spec) and O.is_compiled(fam, CIN, H, W)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, CIN, device=cuda, dtype=torch.bfloat16)
    N, ns = plan(C, fam, lambda: C.conv_pool_fwd(one, wd, bd, pb_h, pb_w), mode)
    x = bf16(rnd(g, N, H, W, CIN))
    xd = x.to(cuda)
    pooled, arg = C.conv_pool_fwd(xd, wd, bd, pb_h, pb_w)
    check_launch(C, fam, '%dx%d %d->%d' % (H, W, CIN, COUT), mode, compiled)
    pp, ap = [], []
    for s in range(0, N, ns):
      pi, ai = C.conv_pool_fwd(xd[s:s + ns], wd, bd, pb_h, pb_w)
      check_slice(C, fam)
      pp.append(pi)
      ap.append(ai)
    O.bits_equal(pooled, torch.cat(pp), 'pooled vs slices')
    O.bits_equal(arg, torch.cat(ap), 'arg vs slices')
  y64 = O.conv64(O.d64(x), O.d64(w), O.d64(b))
  A = O.conv64(O.d64(x).abs(), O.d64(w).abs(), O.d64(b).abs())
  pooled_bound_check(pooled, arg, y64, A, CIN, pb_h, pb_w,
                     'conv_pool_fwd %dx%d %d->%d %s' % (H, W, CIN, COUT, mode))


CONV1 = [(72, 96, 3, 1), (84, 84, 4, 1), (84, 84, 4, 0), (21, 19, 4, 1)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H,W,CH,spec', CONV1)
def test_conv1_pool_fwd(cuda, H, W, CH, spec, mode):
  C = O.ext()
  fam = 'conv1_pool_fwd'
  g = torch.Generator().manual_seed(seed_of(4, H, W, CH, spec))
  w = rnd(g, 3, 3, CH, 16, scale=0.2)
  b = rnd(g, 16, scale=0.1)
  wd, bd = w.to(cuda), b.to(cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  compiled = bool(spec) and O.is_compiled(fam, CH, H, W)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, CH, device=cuda, dtype=torch.uint8)
    N, ns = plan(C, fam, lambda: C.conv1_pool_fwd(one, wd, bd, pb_h, pb_w), mode)
    fr = torch.randint(0, 256, (N, H, W, CH), generator=g, dtype=torch.uint8)
    fd = fr.to(cuda)
    pooled, arg = C.conv1_pool_fwd(fd, wd, bd, pb_h, pb_w)
    check_launch(C, fam, '%dx%dx%d' % (H, W, CH), mode, compiled)
    pp, ap = [], []
    for s in range(0, N, ns):
      pi, ai = C.conv1_pool_fwd(fd[s:s + ns], wd, bd, pb_h, pb_w)
      check_slice(C, fam)
      pp.append(pi)
      ap.append(ai)
    O.bits_equal(pooled, torch.cat(pp), 'pooled vs slices')
    O.bits_equal(arg, torch.cat(ap), 'arg vs slices')
  y64 = O.conv64(O.d64(fr) / 255.0, O.d64(w), O.d64(b))
  pooled_bound_check(pooled, arg, y64, None, CH, pb_h, pb_w,
                     'conv1_pool_fwd %dx%dx%d %s' % (H, W, CH, mode),
                     conv1_tol=2e-2)


# ---------------------------------------------------------------- backward

def grad_checks(C, fam, tag, mode, compiled, launch, N, ns, wshape, cuda, g,
                dw_ref, db_ref, dw_tol, dx_check):
  """Everything the issue asks of a backward family.  launch(sl, dw, db) runs
  images `sl` and returns dx (or None)."""
  nout = wshape[3]
  zeros = lambda: (torch.zeros(*wshape, device=cuda), torch.zeros(nout, device=cuda))
  full = slice(0, N)
  # atomic flush, dW / db from zero
  dw, db = zeros()
  dx = launch(full, dw, db)
  check_launch(C, fam, tag, mode, compiled)
  dxp, dws, dbs = [], torch.zeros(*wshape, dtype=torch.float64), \
      torch.zeros(nout, dtype=torch.float64)
  for s in range(0, N, ns):
    dwi, dbi = zeros()
    dxp.append(launch(slice(s, min(s + ns, N)), dwi, dbi))
    check_slice(C, fam)
    dws += O.d64(dwi)
    dbs += O.d64(dbi)
  if dx is not None:
    O.bits_equal(dx, torch.cat(dxp), 'dx vs slices')
    dx_check(dx)
  O.check_max(dw, dw_ref, dw_tol, '%s.dw %s %s' % (fam, tag, mode))
  O.check_max(db, db_ref, 1e-3, '%s.db %s %s' % (fam, tag, mode))
  O.check_max(dw, dws, 1e-4, '%s.dw-vs-slices %s %s' % (fam, tag, mode))
  O.check_max(db, dbs, 1e-4, '%s.db-vs-slices %s %s' % (fam, tag, mode))
  # accumulation into non-zero dW / db: start + grad.  The start has the
  # gradient's own scale, so the fp32 add rounds far below the 1e-3 bound.
  sw = rnd(g, *wshape) * float(dw_ref.abs().max())
  sb = rnd(g, nout) * float(db_ref.abs().max())
  for det in (0, 1):
    with O.tuned(C, deterministic=det):
      dwa, dba = sw.to(cuda), sb.to(cuda)
      dxa = launch(full, dwa, dba)
      check_launch(C, fam, tag, mode, compiled)
      name = '%s.%s-accumulate %s %s' % (fam, 'det' if det else 'atomic', tag, mode)
      O.check_max(O.d64(dwa) - O.d64(sw.float()), dw_ref, dw_tol, name + ' dw')
      O.check_max(O.d64(dba) - O.d64(sb.float()), db_ref, 1e-3, name + ' db')
      if dx is not None:
        O.bits_equal(dxa, dx, 'dx, flush mode %d' % det)
  # deterministic flush: repeatable bitwise, and the atomic result
  with O.tuned(C, deterministic=1):
    dw1, db1 = zeros()
    dx1 = launch(full, dw1, db1)
    check_launch(C, fam, tag, mode, compiled)
    dw2, db2 = zeros()
    launch(full, dw2, db2)
  O.bits_equal(dw1, dw2, 'deterministic dw, two launches')
  O.bits_equal(db1, db2, 'deterministic db, two launches')
  O.check_max(dw1, dw, 1e-4, '%s.dw det-vs-atomic %s %s' % (fam, tag, mode))
  O.check_max(db1, db, 1e-4, '%s.db det-vs-atomic %s %s' % (fam, tag, mode))
  if dx is not None:
    O.bits_equal(dx1, dx, 'dx deterministic vs atomic')
  return dw, db, dw1, db1


# C, H, W, skip, relu_act, specialize knob
RES_BWD = [
    (16, 36, 48, True, True, 1), (16, 36, 48, False, False, 1),
    (32, 18, 24, True, False, 1), (32, 18, 24, False, True, 0),
    (32, 9, 12, False, True, 1), (32, 21, 21, True, True, 1),
    (32, 11, 11, False, False, 1), (16, 10, 14, True, False, 1),
    (32, 7, 5, False, True, 1)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('Cc,H,W,skip,relu_act,spec', RES_BWD)
def test_res_conv_bwd(cuda, Cc, H, W, skip, relu_act, spec, mode):
  C = O.ext()
  fam = 'res_conv_bwd'
  g = torch.Generator().manual_seed(seed_of(5, Cc, H, W, skip, relu_act, spec))
  w = bf16(rnd(g, 3, 3, Cc, Cc, scale=0.1)).float()
  wd = w.to(cuda)
  compiled = bool(spec) and O.is_compiled(fam, Cc, H, W)
  tag = '%dx%d C%d' % (H, W, Cc)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, Cc, device=cuda, dtype=torch.bfloat16)
    zw, zb = torch.zeros(3, 3, Cc, Cc, device=cuda), torch.zeros(Cc, device=cuda)
    N, ns = plan(C, fam, lambda: C.res_conv_bwd(one, one, None, wd, zw, zb, relu_act),
                 mode)
    act = bf16(rnd(g, N, H, W, Cc))
    if not relu_act:
      act = bf16(act.float().relu())  # stored post-ReLU
    dy = bf16(rnd(g, N, H, W, Cc))
    sk = bf16(rnd(g, N, H, W, Cc)) if skip else None
    actd, dyd = act.to(cuda), dy.to(cuda)
    skd = sk.to(cuda) if skip else None
    a64, dy64, w64 = O.d64(act), O.d64(dy), O.d64(w)
    mask = (a64 > 0).to(torch.float64)
    dx_ref = mask * O.dgrad64(dy64, w64)
    A = mask * O.dgrad64(dy64.abs(), w64.abs())
    if skip:
      dx_ref, A = dx_ref + O.d64(sk), A + O.d64(sk).abs()
    dw_ref, db_ref = O.wgrad64(a64.relu(), dy64), dy64.sum(dim=(0, 1, 2))

    def launch(sl, dw, db):
      return C.res_conv_bwd(dyd[sl], actd[sl], skd[sl] if skip else None, wd,
                            dw, db, relu_act)

    grad_checks(C, fam, tag, mode, compiled, launch, N, ns, (3, 3, Cc, Cc), cuda,
                g, dw_ref, db_ref, 1e-3,
                lambda dx: O.check_bound(dx, dx_ref, A, Cc,
                                         'res_conv_bwd.dx %s %s' % (tag, mode)))


def pooled_grad(g, N, Hp, Wo, C):
  """dP on a 1/8 grid in [-4, 4]: the sum of the up to four windows that land
  on one conv cell is then exact in bf16 (8 significant bits), so the gathered
  dY has one value whatever the order and precision of the additions."""
  return bf16(torch.randint(-32, 33, (N, Hp, Wo, C), generator=g).float() / 8)


POOL_BWD = [(16, 32, 36, 48, 1), (32, 32, 18, 24, 1), (32, 32, 21, 21, 1),
            (16, 16, 10, 14, 1), (32, 32, 7, 5, 1), (32, 32, 18, 24, 0)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('CIN,COUT,H,W,spec', POOL_BWD)
def test_pool_conv_bwd(cuda, CIN, COUT, H, W, spec, mode):
  C = O.ext()
  fam = 'pool_conv_bwd'
  g = torch.Generator().manual_seed(seed_of(6, CIN, COUT, H, W, spec))
  w = bf16(rnd(g, 3, 3, CIN, COUT, scale=0.1)).float()
  b = rnd(g, COUT, scale=0.1)
  wd, bd = w.to(cuda), b.to(cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  compiled = bool(spec) and O.is_compiled(fam, CIN, H, W)
  tag = '%dx%d %d->%d' % (H, W, CIN, COUT)
  wshape = (3, 3, CIN, COUT)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, CIN, device=cuda, dtype=torch.bfloat16)
    onep = torch.zeros(1, Hp, Wo, COUT, device=cuda, dtype=torch.bfloat16)
    onea = torch.full((1, Hp, Wo, COUT), 4, device=cuda, dtype=torch.uint8)
    zw, zb = torch.zeros(*wshape, device=cuda), torch.zeros(COUT, device=cuda)
    N, ns = plan(C, fam, lambda: C.pool_conv_bwd(onep, onea, one, wd, zw, zb, True,
                                                 pb_h, pb_w), mode)
    x = bf16(rnd(g, N, H, W, CIN))
    xd = x.to(cuda)
    _, argd = C.conv_pool_fwd(xd, wd, bd, pb_h, pb_w)
    dP = pooled_grad(g, N, Hp, Wo, COUT)
    dPd = dP.to(cuda)
    dY = O.scatter64(dP, argd, H, W, pb_h, pb_w)
    assert torch.equal(dY, O.d64(bf16(dY)))  # exact in bf16 (pooled_grad)
    w64 = O.d64(w)
    dx_ref, A = O.dgrad64(dY, w64), O.dgrad64(dY.abs(), w64.abs())
    dw_ref, db_ref = O.wgrad64(O.d64(x), dY), dY.sum(dim=(0, 1, 2))

    def launch(sl, dw, db, need_dx=True):
      return C.pool_conv_bwd(dPd[sl], argd[sl], xd[sl], wd, dw, db, need_dx,
                             pb_h, pb_w)

    dw, db, dw1, db1 = grad_checks(
        C, fam, tag, mode, compiled, launch, N, ns, wshape, cuda, g, dw_ref,
        db_ref, 1e-3,
        lambda dx: O.check_bound(dx, dx_ref, A, CIN,
                                 'pool_conv_bwd.dx %s %s' % (tag, mode)))
    # need_dx=False: no dx, the same weight gradients
    dwn, dbn = torch.zeros(*wshape, device=cuda), torch.zeros(COUT, device=cuda)
    assert launch(slice(0, N), dwn, dbn, False) is None
    check_launch(C, fam, tag, mode, compiled)
    O.check_max(dwn, dw, 1e-4, 'pool_conv_bwd.dw need_dx=False ' + tag)
    O.check_max(dbn, db, 1e-4, 'pool_conv_bwd.db need_dx=False ' + tag)
    with O.tuned(C, deterministic=1):
      dwn, dbn = torch.zeros(*wshape, device=cuda), torch.zeros(COUT, device=cuda)
      assert launch(slice(0, N), dwn, dbn, False) is None
    O.bits_equal(dwn, dw1, 'deterministic dw, need_dx=False')
    O.bits_equal(dbn, db1, 'deterministic db, need_dx=False')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('H,W,CH,spec', CONV1)
def test_conv1_pool_bwd(cuda, H, W, CH, spec, mode):
  C = O.ext()
  fam = 'conv1_pool_bwd'
  g = torch.Generator().manual_seed(seed_of(7, H, W, CH, spec))
  w = rnd(g, 3, 3, CH, 16, scale=0.2)
  b = rnd(g, 16, scale=0.1)
  wd, bd = w.to(cuda), b.to(cuda)
  pb_h, pb_w = O.pool_pb(H), O.pool_pb(W)
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  compiled = bool(spec) and O.is_compiled(fam, CH, H, W)
  tag = '%dx%dx%d' % (H, W, CH)
  wshape = (3, 3, CH, 16)
  with O.small_grid(C), O.tuned(C, specialize=spec):
    one = torch.zeros(1, H, W, CH, device=cuda, dtype=torch.uint8)
    onep = torch.zeros(1, Hp, Wo, 16, device=cuda, dtype=torch.bfloat16)
    onea = torch.full((1, Hp, Wo, 16), 4, device=cuda, dtype=torch.uint8)
    zw, zb = torch.zeros(*wshape, device=cuda), torch.zeros(16, device=cuda)
    N, ns = plan(C, fam, lambda: C.conv1_pool_bwd(onep, onea, one, zw, zb, pb_h, pb_w),
                 mode)
    fr = torch.randint(0, 256, (N, H, W, CH), generator=g, dtype=torch.uint8)
    fd = fr.to(cuda)
    _, argd = C.conv1_pool_fwd(fd, wd, bd, pb_h, pb_w)
    dP = pooled_grad(g, N, Hp, Wo, 16)
    dPd = dP.to(cuda)
    dY = O.scatter64(dP, argd, H, W, pb_h, pb_w)
    dw_ref = O.wgrad64(O.d64(fr) / 255.0, dY)
    db_ref = dY.sum(dim=(0, 1, 2))

    def launch(sl, dw, db):
      C.conv1_pool_bwd(dPd[sl], argd[sl], fd[sl], dw, db, pb_h, pb_w)
      return None

    grad_checks(C, fam, tag, mode, compiled, launch, N, ns, wshape, cuda, g,
                dw_ref, db_ref, 5e-3, None)
