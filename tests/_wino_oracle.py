"""Float64 oracles, magnitude functions, launch arithmetic and case tables for
the persistent fp32 Winograd kernels of csrc/kernels/conv_wino.hip
(test_wino_oracle.py on the CPU, test_wino_ranges_gpu.py on the GPU).

Reference values are the DIRECT float64 convolutions of _conv_f32_oracle.py
(conv, conv_dgrad, conv_wgrad, maxpool), never a Winograd evaluation.  The
Winograd algebra appears here only in the magnitude functions below.

F(2x2, 3x3):  Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A per 2x2 output tile,
dW = G^T [ sum_tiles (B^T x B) .* (A dY A^T) ] G for the weight gradient.
B and A hold 0 / +-1, G holds 0, 1, +-1/2.

Magnitudes.  `mag_fwd` / `mag_wgrad` are the same operations applied to
magnitudes, i.e. with every entry of G, B, A, the weights and the activations
replaced by its absolute value:
  forward / data gradient   |A^T| [ sum_ci |G||g||G^T| .* |B^T||d||B| ] |A|
                            + |bias| + |add|
  weight gradient           |G^T| [ sum_tiles |B^T||x||B| .* |A||dY||A^T| ] |G|
                            + |dW at the start|
  bias gradient             sum |dY| + |db at the start|
They bound every partial sum the kernels can form, in any order, and every
intermediate of the transforms.

Exact regime.  Activations and dY are integers in [-3, 3], weights and biases
in [-2, 2] (_conv_f32_oracle.acts / weights).  B^T d B, A^T M A and A dY A^T
only add and subtract; G g G^T and G^T P G add multiples of 1/2 and 1/4.  So
every intermediate is a multiple of 1/4 of magnitude at most the magnitude
function, and a multiple of 1/4 below 2^22 is a float32: where
4 * magnitude < 2^24 (`exact_ok4`, asserted on the CPU for every exact case)
no operation rounds, whatever the split into ranges, runs and slots, and the
kernel output must EQUAL the direct float64 result, which is the same integer.
Integer maps have many exactly tied pool windows and many exact zeros: the
ReLU mask is x > 0 and the argmax code is the FIRST maximal tap, both compared
at every element.

Rounding regime (random normal inputs).  Elementwise
  |out - ref| <= (M + c) 2^-24 magnitude
counting, to first order, the rounded operations above any one term:
  forward / data gradient, M = Cin (the data gradient: the channels of dY)
    4   G g G^T: two passes, each (a +- b) + c (the halvings are exact)
    2   B^T d B: two passes of one add / subtract (wino_input_transform)
    Cin the MFMA chain over the input channels (products are fused)
    4   A^T M A: two passes of two adds (wino_output_transform)
    2   bias, residual add (mask, ReLU and max are exact)
    1   the fused32 16-channel data gradient adds two half-chains' output
        transforms; also covers the second-order part of (1 + 2^-24)^(M+12)
    => c = 13
  weight gradient, M = N TY TX (tiles), bias gradient M = N H W (pixels)
    2   B^T x B,  2  A dY A^T (one add per pass)
    M   the tile sum in ANY order and grouping (MFMA k-steps, waves, ranges,
        per-workgroup slots, the slot tree): a sum of M terms leaves each term
        under at most M - 1 additions
    4   G^T P G: two passes of two adds, once per slot (linear, so the slot
        sum of transformed partials has the magnitude of the whole)
    1   the read-modify-write of dW / db
    1   second order (M <= 7000 here: (M 2^-24)^2 is far below one unit)
    => c = 10
The constants come from these chains, not from measured errors; the GPU test
prints the largest error / bound ratio per family (WINOREC lines).

Pool.  The max is 1-Lipschitz, so a pooled value is off by at most the largest
bound in its window; in the rounding regime a code is compared where the
float64 window's two largest values differ by more than twice that
(_conv_f32_oracle.argmax_clear); the share of windows left out stays below
1 % (checked on the CPU from float64 alone).

Launch arithmetic.  plan_* redo run_wino_g, run_wino_pool, run_wino_pool_img,
run_wino_wgrad, run_wino_bwd32_g and run_wino_bwd_g by hand for a grid cap of
0: TY, TX, tiles per image, RT, nranges, the grid and the decline conditions
(more than 4 images per range, staging slots, LDS).  The GPU test compares
cf32_wino_launch_info with them, so with the cap at 0 the hooks change no
launch.  Which fused32 cases run the row-keeping instance is tabled by hand
(KEEP_DECLINED) and asserted from the hook.

Case picker (`pick`): per (kernel, map) the smallest N >= 2 with
nranges >= 2 cap + 1, nranges % cap != 0 (uneven runs) and a ragged last range
(NT % RT != 0) wherever some N gives one; cap = 3, and where nranges % 3 != 0
has no solution in N the case also runs on 4 or 5 workgroups.
"""

import functools
import math

import torch

from tests import _conv_f32_oracle as O

U = O.U
CAP = 3
C_FWD = 13
C_WG = 10
CUS = 256
LDS_MAX = 160 * 1024
K_MAX_PARTS = 4

G_ = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
                  dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


# --------------------------------------------------------------- magnitudes

def tiles_of(H, W):
  return (H + 1) // 2, (W + 1) // 2


def patches(x):
  """[N,TY,TX,4,4,C]: the 4x4 input patch of every 2x2 tile of the 1-padded
  map (zeros outside)."""
  N, H, W, C = x.shape
  TY, TX = tiles_of(H, W)
  xp = torch.zeros(N, 2 * TY + 2, 2 * TX + 2, C, dtype=torch.float64)
  xp[:, 1:H + 1, 1:W + 1] = x
  return torch.stack([torch.stack([xp[:, i:i + 2 * TY:2, j:j + 2 * TX:2] for j in range(4)], 3)
                      for i in range(4)], 3)


def out_tiles(y):
  """[N,TY,TX,2,2,C]: the 2x2 tiles of a map (zeros past an odd edge)."""
  N, H, W, C = y.shape
  TY, TX = tiles_of(H, W)
  yp = torch.zeros(N, 2 * TY, 2 * TX, C, dtype=torch.float64)
  yp[:, :H, :W] = y
  return yp.reshape(N, TY, 2, TX, 2, C).permute(0, 1, 3, 2, 4, 5)


def wino_fwd(x, w, absolute):
  """The F(2x2,3x3) evaluation of conv(x, w) (HWIO), or, with `absolute`, the
  same on magnitudes: |A^T| [ sum |G||g||G^T| .* |B^T||d||B| ] |A|."""
  f = (lambda t: t.abs()) if absolute else (lambda t: t)
  N, H, W, _ = x.shape
  TY, TX = tiles_of(H, W)
  Uw = torch.einsum('ak,klio,bl->abio', f(G_), f(w), f(G_))
  V = torch.einsum('ai,ntxijc,bj->ntxabc', f(BT), patches(f(x)), f(BT))
  M = torch.einsum('ntxabc,abco->ntxabo', V, Uw)
  Y = torch.einsum('pa,ntxabo,qb->ntxpqo', f(AT), M, f(AT))
  return Y.permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * TY, 2 * TX, -1)[:, :H, :W].contiguous()


def mag_fwd(x, w):
  return wino_fwd(x.double(), w.double(), True)


def flip_t(w):
  """The data gradient's weights: flipped in (ky, kx), transposed in (ci, co)."""
  return w.flip(0, 1).transpose(2, 3).contiguous()


def wino_wgrad(x, dy, absolute):
  """G^T [ sum_tiles (B^T x B) .* (A dY A^T) ] G (HWIO), or on magnitudes."""
  f = (lambda t: t.abs()) if absolute else (lambda t: t)
  V = torch.einsum('ai,ntxijc,bj->ntxabc', f(BT), patches(f(x)), f(BT))
  Z = torch.einsum('pa,ntxpqo,qb->ntxabo', f(AT), out_tiles(f(dy)), f(AT))
  P = torch.einsum('ntxabc,ntxabo->abco', V, Z)
  return torch.einsum('ak,abco,bl->klco', f(G_), P, f(G_))


def mag_wgrad(x, dy):
  return wino_wgrad(x.double(), dy.double(), True)


def bound_fwd(cin, mag):
  return (cin + C_FWD) * U * mag


def bound_wg(M, mag):
  return (M + C_WG) * U * mag


def exact_ok4(*mags):
  """Every intermediate is a multiple of 1/4: 4 * magnitude < 2^24."""
  return all(4 * float(m.max()) < O.EXACT_LIMIT for m in mags)


# -------------------------------------------------- launch arithmetic (host)

def wino_parts(RT, per_img):
  return (RT - 1 + per_img - 1) // per_img + 1


def wino_maxrows(RT, TX, TY):
  rows = RT // TX if RT % TX == 0 else (RT - 1 + TX - 1) // TX + 1
  return 2 * rows + 2 * (1 if (TY * TX) % RT == 0 else wino_parts(RT, TY * TX))


def wino_lpad(TX):
  return (8 - (TX + 2) % 8) % 8


GEO16 = ((36, 48), (42, 42), (36, 64))
GEO32 = ((18, 24), (9, 12), (21, 21), (11, 11), (18, 32), (9, 16))
# (cin, cout): (NW, MAXC, WPS) of wino_conv_launch's default instances
FWD_CFG = {(16, 16): (4, 10, 2), (16, 32): (8, 5, 2), (32, 32): (8, 8, 2)}


def geo_maps(cin, cout):
  if cin == 16:
    return GEO16
  return GEO32 if (cin, cout) == (32, 32) else ()


def fwd_fl(cin, cout, H, W, fl, flip, geo_on):
  """The compile-time flag instance run_wino_fl picks, or -1."""
  if flip or not geo_on:
    return -1
  if (cin, cout) == (16, 16) and fl in (19, 24) and (H, W) in GEO16:
    return fl
  if (cin, cout) == (32, 32):
    if fl == 19 and (H, W) in ((18, 24), (18, 32)):
      return 19
    if fl == 24 and (H, W) in GEO32:
      return 24
  return -1


def _base(N, H, W, RT):
  TY, TX = tiles_of(H, W)
  NT = N * TY * TX
  return TY, TX, NT, -(-NT // RT)


def plan_fwd(N, H, W, cin, cout, fl=0, flip=False, geo_on=True):
  """run_wino_g behind wino_conv_launch; None where it declines."""
  NW, MAXC, WPS = FWD_CFG[(cin, cout)]
  RT = 64
  TY, TX, NT, nranges = _base(N, H, W, RT)
  if NT >= 1 << 22 or wino_parts(RT, TY * TX) > K_MAX_PARTS:
    return None
  geo = geo_on and (H, W) in geo_maps(cin, cout)
  Wl = 2 * TX + 2
  WlP = Wl + (wino_lpad(TX) if geo else 0)
  maxrows = wino_maxrows(RT, TX, TY)
  if maxrows * Wl * (cin // 4) > MAXC * 64 * NW or maxrows > 64 * NW:
    return None
  nbytes = 4 * (16 * cin * cout + maxrows * WlP * (cin + 4) + maxrows)
  if nbytes > LDS_MAX:
    return None
  per_cu = max(1, min(WPS * 4 // NW, LDS_MAX // (nbytes + 256)))
  return dict(family='wino_conv', cin=cin, cout=cout, grid=max(1, min(nranges, CUS * per_cu)),
              nranges=nranges, rt=RT, tiles_per_img=TY * TX, geo=int(geo),
              fl=fwd_fl(cin, cout, H, W, fl, flip, geo_on), flip=int(flip))


def plan_pool(N, H, W, cin, cout):
  """run_wino_pool: ranges are tile-row pairs (RT = W tiles), an odd number of
  tile rows ends each image with a single row (the OT instance)."""
  TY, TX = H // 2, W // 2
  NW = -(-W // 16) * (cout // 16)
  PP, IPP = (4 if cin == 4 else cin + 4), cout + 4
  xreg = max(6 * (W + 2) * PP, 4 * W * IPP)
  nbytes = 4 * (16 * cin * cout + xreg + 6)
  per_cu = max(1, min(3 * 4 // NW, LDS_MAX // (nbytes + 256)))
  nranges = N * ((TY + 1) // 2)
  return dict(family='wino_pool_ot' if TY % 2 else 'wino_pool', cin=cin, cout=cout,
              grid=max(1, min(nranges, CUS * per_cu)), nranges=nranges, rt=W,
              tiles_per_img=TY * TX, geo=0, fl=-1, flip=0)


def plan_pool_img(N, H, W, cin, cout):
  nti = (H // 2) * (W // 2)
  return dict(family='wino_pool_img', cin=cin, cout=cout, grid=max(1, min(N, CUS)), nranges=N,
              rt=nti, tiles_per_img=nti, geo=1, fl=-1, flip=0)


def wg_slot_cap(cin, cout):
  rows16 = ((9 * cin + 16) // 16) * 16
  return O.wgrad_slots(3, cin, cout) * rows16 * cout // (rows16 * cout)


def plan_wgrad(N, H, W):
  """run_wino_wgrad<32, 32, 1, 64, 15, 14>."""
  cin = cout = 32
  RT, MAXCX, MAXCD = 64, 15, 14
  TY, TX, NT, nranges = _base(N, H, W, RT)
  parts = wino_parts(RT, TY * TX)
  if NT >= 1 << 22 or parts > K_MAX_PARTS:
    return None
  Wl, Wd = 2 * TX + 2, 2 * TX
  maxrows = 2 * ((RT - 1 + TX - 1) // TX + 1) + 2 * parts
  if (maxrows * Wl * (cin // 4) > MAXCX * 256 or maxrows * Wd * (cout // 4) > MAXCD * 256 or
      maxrows > 256):
    return None
  stage = 4 * maxrows * (Wl * (cin + 8) + Wd * (cout + 8)) + 4 * (maxrows + 2 * RT)
  if max(stage, 4 * (16 * cin * cout + cout)) > LDS_MAX:
    return None
  return dict(family='wino_wgrad', cin=cin, cout=cout,
              grid=min(nranges, CUS, wg_slot_cap(cin, cout)), nranges=nranges, rt=RT,
              tiles_per_img=TY * TX, geo=0, fl=-1, flip=0)


# (CX, CY): (RT, MAXCX, MAXCY) of wino_bwd_fused_launch's fused32 instances
BWD32_CFG = {(16, 16): (64, 5, 5), (32, 32): (32, 5, 5), (16, 32): (32, 4, 8)}


def fused32_lds(CX, CY, RT, maxrows, Wl):
  return (4 * (16 * CX * CY + maxrows * Wl * (CX + CY + 8)) +
          (4 * 2 * 4 * 64 * 4 if (RT // 16) * (CX // 16) == 2 else 0) + 4 * (2 + maxrows + RT))


def keep_fits(RT, H, TX, TY, NT, nranges, maxrows, krows):
  """fused32_keep_fits, line by line."""
  nslots = maxrows - 1
  if krows < 1 or nslots < 2:
    return False
  per_img = TX * TY
  period = per_img // math.gcd(per_img, RT)
  prevB = -1
  for r in range(min(nranges, period + 1)):
    t0 = r * RT
    t1 = min(t0 + RT, NT)
    R0, R1 = t0 // TX, (t1 - 1) // TX
    n0, n1 = R0 // TY, R1 // TY
    A = n0 * H + max(2 * (R0 - n0 * TY) - 1, 0)
    B = n1 * H + min(2 * (R1 - n1 * TY) + 2, H - 1)
    if B - A + 1 > nslots:
      return False
    if r > 0 and A <= prevB and B - prevB > krows:
      return False
    prevB = B
  return True


def plan_bwd(N, H, W, cx, cy, relu, mask, geo_on=True, keep_on=True):
  """wino_bwd_fused_launch: the masked 16 -> 16 convs run wino_bwd_fused_kernel
  (wino_bwd16), everything else the fused32 kernel.  `family` is wino_bwd32
  here; KEEP_DECLINED says which cases run the row-keeping instance."""
  if (cx, cy) == (16, 16) and mask:
    RT, MAXC, NW = 64, 5, 8
    TY, TX, NT, nranges = _base(N, H, W, RT)
    if NT >= 1 << 22 or wino_parts(RT, TY * TX) > K_MAX_PARTS:
      return None
    Wl = 2 * TX + 2
    maxrows = wino_maxrows(RT, TX, TY)
    if maxrows * Wl * 4 > MAXC * 64 * NW or maxrows > 64 * NW:
      return None
    if 4 * (16 * 256 + 2 * maxrows * Wl * 20) + 4 * (maxrows + RT) > LDS_MAX:
      return None
    return dict(family='wino_bwd16', cin=16, cout=16,
                grid=min(nranges, CUS, wg_slot_cap(16, 16)), nranges=nranges, rt=RT,
                tiles_per_img=TY * TX, geo=int(geo_on and (H, W) in GEO16),
                fl=(1 if relu else 0) | 4, flip=1)
  RT, MAXCX, MAXCY = BWD32_CFG[(cx, cy)]
  TY, TX, NT, nranges = _base(N, H, W, RT)
  if NT >= 1 << 22 or wino_parts(RT, TY * TX) > K_MAX_PARTS:
    return None
  Wl = 2 * TX + 2
  maxrows = wino_maxrows(RT, TX, TY)
  if (maxrows * Wl * (cy // 4) > MAXCY * 512 or maxrows * Wl * (cx // 4) > MAXCX * 512 or
      maxrows > 512):
    return None
  if fused32_lds(cx, cy, RT, maxrows, Wl) > LDS_MAX:
    return None
  # compile-time geometry: every 32-channel-input form, and the unmasked 16s;
  # the relu-without-mask form has none
  geo = (geo_on and (mask or not relu) and (cx == 32 or not mask) and
         (H, W) in geo_maps(cx, cy))
  return dict(family='wino_bwd32', cin=cx, cout=cy,
              grid=min(nranges, CUS, wg_slot_cap(cx, cy)), nranges=nranges, rt=RT,
              tiles_per_img=TY * TX, geo=int(geo), fl=(1 if relu else 0) | (4 if mask else 0),
              flip=1)


def keep_expected(N, H, W, cx, cy):
  """run_wino_bwd32_g's choice of the row-keeping instance, recomputed (the
  CPU test holds KEEP_DECLINED against it)."""
  RT = BWD32_CFG[(cx, cy)][0]
  TY, TX, NT, nranges = _base(N, H, W, RT)
  Wl = 2 * TX + 2
  maxrows = wino_maxrows(RT, TX, TY)
  kcx, kcy = ((2, 4) if (cx, cy) == (16, 32) else (3, 3))
  krows = min(kcy * 512 // (Wl * (cy // 4)), kcx * 512 // (Wl * (cx // 4)), maxrows - 1)
  kbytes = fused32_lds(cx, cy, RT, maxrows, Wl) + 4 * (4 + 3 * RT + 2 * maxrows)
  return kbytes <= LDS_MAX and keep_fits(RT, H, TX, TY, NT, nranges, maxrows, krows)


def runs(nranges, G):
  """The contiguous run [lo, hi) of every workgroup (range_walk)."""
  return [(b * nranges // G, (b + 1) * nranges // G) for b in range(G)]


def pick(nr, ragged, lo=2, hi=16):
  """(N, caps) of the case picker (module docstring); nr(N) = nranges,
  ragged(N) = the last range is short."""
  def first(cap, want_ragged):
    for n in range(lo, hi + 1):
      if nr(n) >= 2 * cap + 1 and nr(n) % cap != 0 and (ragged(n) or not want_ragged):
        return n
    return None
  for caps in ((CAP,), (CAP, 4), (CAP, 5)):
    for want in (True, False):
      n = first(caps[-1], want)
      if n is not None and nr(n) >= 2 * CAP + 1:
        return n, caps
  raise AssertionError('no N')


def pick_tiles(H, W, RT):
  TY, TX = tiles_of(H, W)
  return pick(lambda n: -(-n * TY * TX // RT), lambda n: (n * TY * TX) % RT != 0)


def _seed(*key):
  return O._seed('wino', *key)


# ------------------------------------------------------------ forward cases
# (bias, relu_in, add, relu_out) and the launcher's flag word
FWD_FLAGS = {'none': (False, False, False, False), 'bias': (True, False, False, False),
             'res1': (True, True, False, True), 'res2': (True, False, True, False),
             'add_relu': (False, False, True, True)}
FLAG_WORD = {'none': 0, 'bias': 16, 'res1': 19, 'res2': 24, 'add_relu': 10}
# maps without an instance: odd H and W (partial tiles on both edges), and one
# wider than every instance map of the configuration that run_wino_g still
# takes (16-channel inputs: 128 columns = one tile row per 64-tile range,
# 4 staged rows of 130 pixels; 32 -> 32: 8x64, 6 rows of 66 pixels)
RUNTIME_MAPS = {(16, 16): ((13, 15), (4, 128)), (16, 32): ((13, 15), (4, 128)),
                (32, 32): ((13, 15), (8, 64))}


def fwd_cases():
  out = []
  for (cin, cout) in sorted(FWD_CFG):
    for (H, W) in geo_maps(cin, cout) + RUNTIME_MAPS[(cin, cout)]:
      out.append('%dto%d_%dx%d' % (cin, cout, H, W))
  return out


def parse(name):
  ch, hw = name.split('_')[-2:]
  cin, cout = (int(v) for v in ch.split('to'))
  H, W = (int(v) for v in hw.split('x'))
  return cin, cout, H, W


@functools.lru_cache(maxsize=None)
def fwd_data(name, exact):
  cin, cout, H, W = parse(name)
  N, caps = pick_tiles(H, W, 64)
  g = O.gen(_seed('fwd', name, exact))
  x = O.acts(g, (N, H, W, cin), exact)
  w = O.weights(g, (3, 3, cin, cout), exact)
  b = O.weights(g, (cout,), exact)
  add = O.acts(g, (N, H, W, cout), exact)
  x64, w64 = x.double(), w.double()
  return dict(N=N, caps=caps, H=H, W=W, cin=cin, cout=cout, x=x, w=w, b=b, add=add,
              lin=O.conv(x64, w64, None, 1), lin_relu=O.conv(x64.clamp(min=0), w64, None, 1),
              mag=mag_fwd(x64, w64), mag_relu=mag_fwd(x64.clamp(min=0), w64))


def fwd_ref(d, flags):
  bias, relu_in, add, relu_out = FWD_FLAGS[flags]
  ref = (d['lin_relu'] if relu_in else d['lin']).clone()
  A = (d['mag_relu'] if relu_in else d['mag']).clone()
  if bias:
    ref += d['b'].double()
    A += d['b'].double().abs()
  if add:
    ref += d['add'].double()
    A += d['add'].double().abs()
  if relu_out:
    ref = ref.clamp(min=0)
  return ref, A


DGRAD_CASES = ('16to16_36x48', '16to16_13x15', '32to32_18x24', '32to32_11x11')


@functools.lru_cache(maxsize=None)
def dgrad_data(name, exact):
  cin, cout, H, W = parse(name)
  N, caps = pick_tiles(H, W, 64)
  g = O.gen(_seed('dgrad', name, exact))
  dy = O.acts(g, (N, H, W, cout), exact)
  w = O.weights(g, (3, 3, cin, cout), exact)
  mask = O.acts(g, (N, H, W, cin), exact)
  add = O.acts(g, (N, H, W, cin), exact)
  return dict(N=N, caps=caps, H=H, W=W, cin=cin, cout=cout, dy=dy, w=w, mask=mask, add=add,
              lin=O.conv_dgrad(dy.double(), w.double(), 1, H, W),
              mag=mag_fwd(dy.double(), flip_t(w.double())))


def dgrad_ref(d, masked):
  if not masked:
    return d['lin'], d['mag']
  ref = torch.where(d['mask'].double() > 0, d['lin'], torch.zeros_like(d['lin']))
  return ref + d['add'].double(), d['mag'] + d['add'].double().abs()


# --------------------------------------------------------- stage-head cases
# name: (H, W, cin, cout, stages).  H = 8: two ranges per image; H = 12: three
# (nranges % 3 == 0 for every N: also capped at 4); H = 4: one range per image,
# every range a whole image; 42x42 and 10x48: an odd number of tile rows (the
# OT instance; stages 15 turns the 42-wide one on)
POOL_CASES = {
    'h16to32_8x48': (8, 48, 16, 32, 15), 'h16to32_12x48': (12, 48, 16, 32, 15),
    'h16to32_8x32': (8, 32, 16, 32, 15), 'h16to32_4x32': (4, 32, 16, 32, 15),
    'h16to32_8x64': (8, 64, 16, 32, 15),
    'h16to32_42x42': (42, 42, 16, 32, 15), 'h16to32_10x48': (10, 48, 16, 32, 15),
    'h4to16_8x96': (8, 96, 4, 16, 3), 'h4to16_8x64': (8, 64, 4, 16, 3),
    'h4to16_8x128': (8, 128, 4, 16, 3), 'h4to16_8x84': (8, 84, 4, 16, 3),
    'h32to32_18x24': (18, 24, 32, 32, 7),
}


# Extra grid caps.  An odd-TY image ends with a single tile row that stores no
# pooled row of its own; a run that carries rows into it and walks on into the
# next image must drop that carry.  10x48 on 3 or 4 workgroups has no such run
# (its runs there start on the single-row range or end in it), on 2 it has.
POOL_EXTRA_CAPS = {'h16to32_10x48': (2,)}


def pool_plan(name, N):
  H, W, cin, cout, _ = POOL_CASES[name]
  if cin == 32:
    return plan_pool_img(N, H, W, cin, cout)
  return plan_pool(N, H, W, cin, cout)


def pool_geom(name):
  H, W, cin, cout, stages = POOL_CASES[name]
  N, caps = pick(lambda n: pool_plan(name, n)['nranges'], lambda n: True)
  return dict(H=H, W=W, cin=cin, cout=cout, stages=stages, N=N,
              caps=caps + POOL_EXTRA_CAPS.get(name, ()),
              plan=pool_plan(name, N), rpi=pool_plan(name, 1)['nranges'])


@functools.lru_cache(maxsize=None)
def pool_data(name, exact):
  q = pool_geom(name)
  g = O.gen(_seed('pool', name, exact))
  x = O.acts(g, (q['N'], q['H'], q['W'], q['cin']), exact)
  if q['cin'] == 4:
    x[..., 3] = 0  # the image's pad channel
  w = O.weights(g, (3, 3, q['cin'], q['cout']), exact)
  b = O.weights(g, (q['cout'],), exact)
  pre = O.conv(x.double(), w.double(), b.double(), 1)
  mag = mag_fwd(x, w) + b.double().abs()
  bnd = bound_fwd(q['cin'], mag)
  win = O.pool_windows(pre)[0]
  wb = O.pool_windows(bnd)[0].clamp(min=0)
  val, code = O.first_max(win)
  return dict(q, x=x, w=w, b=b, pre=pre, mag=mag, val=val, code=code, win=win,
              val_bound=wb.max(-1).values, clear=O.argmax_clear(win, wb))


# ------------------------------------------------------ weight-grad cases
WGRAD_MAPS = ((18, 24), (9, 12), (21, 21), (13, 15))


@functools.lru_cache(maxsize=None)
def wgrad_data(hw, relu_in, exact):
  H, W = hw
  N, caps = pick_tiles(H, W, 64)
  g = O.gen(_seed('wgrad', hw, relu_in, exact))
  x = O.acts(g, (N, H, W, 32), exact)
  dy = O.acts(g, (N, H, W, 32), exact)
  dw0 = O.weights(g, (3, 3, 32, 32), True)
  db0 = O.weights(g, (32,), True) + 3.0
  dw0[dw0 == 0] = 1.0
  xin = x.double().clamp(min=0) if relu_in else x.double()
  rw, rb = O.conv_wgrad(xin, dy.double(), 3, 1)
  TY, TX = tiles_of(H, W)
  return dict(N=N, caps=caps, H=H, W=W, x=x, dy=dy, dw0=dw0, db0=db0,
              rw=rw + dw0.double(), rb=rb + db0.double(),
              mw=mag_wgrad(xin, dy) + dw0.double().abs(),
              mb=dy.double().abs().sum((0, 1, 2)) + db0.double().abs(),
              M=N * TY * TX, Mb=N * H * W)


# ------------------------------------------------------ fused backward cases
# form: (cx, cy, relu_x, mask, add)
BWD_FORMS = {
    'res16_relu_add': (16, 16, True, True, True),    # wino_bwd16, conv 1 of a block
    'res16_plain': (16, 16, False, True, False),     # wino_bwd16, conv 2
    'u16': (16, 16, False, False, False),            # unmasked 16 -> 16: fused32 over 64 tiles
    'head16to32': (16, 32, False, False, False),
    'res32_relu_add': (32, 32, True, True, True),
    'res32_plain': (32, 32, False, True, False),
    'head32': (32, 32, False, False, False),
}
# 36x64 and 16x48: whole-tile-row ranges of one image leave no slot for the
# zero row, the keep stager declines (run_wino_bwd32_g)
BWD_MAPS = {16: GEO16 + ((16, 48),), 32: GEO32 + ((13, 15),)}


def bwd_cases():
  out = []
  for form, (cx, cy, _, _, _) in sorted(BWD_FORMS.items()):
    for (H, W) in BWD_MAPS[cx]:
      # the relu + add forms on two maps each (an even and an odd one)
      if form.endswith('relu_add') and (H, W) not in ((36, 48), (42, 42), (18, 24), (11, 11)):
        continue
      out.append('%s_%dto%d_%dx%d' % (form, cx, cy, H, W))
  return out


def bwd_form(name):
  form = name.rsplit('_', 2)[0]
  return form, BWD_FORMS[form]


def bwd_rt(cx, cy, mask):
  return 64 if (cx, cy) == (16, 16) else 32


# The fused32 cases that must run the plain stager (wino_bwd32) although the
# keep switch is on; every other fused32 case must run wino_bwd32_keep.  By
# hand from fused32_keep_fits, which needs every range's image rows in
# maxrows - 1 row slots.  36x64 (TX 32; RT 32 and RT 64): every range is whole
# tile rows of one image, maxrows = 2 RT / TX + 2 is exactly the rows an
# interior range reads.  16x48 at RT 64 (TY TX = 192 = 3 RT: one image per
# range, maxrows = 2 * 4 + 2 = 10): range 1 is tiles 64..127 = tile rows 2..5
# = image rows 3..12, 10 rows for 9 slots.  (16x48 at RT 32 fits: every range
# there touches 2 tile rows = 6 image rows, maxrows = 2 * 3 + 2 = 8: 7 slots.)
# The recomputation (keep_expected) is held against this table on the CPU,
# the launch hook on the GPU.
KEEP_DECLINED = frozenset(('head16to32_16to32_36x64', 'u16_16to16_36x64', 'u16_16to16_16x48'))


def bwd_family(name, keep_on=True):
  """The family a fused-backward case must report."""
  _, (cx, cy, _, mask, _) = bwd_form(name)
  if (cx, cy) == (16, 16) and mask:
    return 'wino_bwd16'
  return 'wino_bwd32_keep' if keep_on and name not in KEEP_DECLINED else 'wino_bwd32'


@functools.lru_cache(maxsize=None)
def bwd_data(name, exact):
  form, (cx, cy, relu, mask, add) = bwd_form(name)
  _, _, H, W = parse(name)
  N, caps = pick_tiles(H, W, bwd_rt(cx, cy, mask))
  g = O.gen(_seed('bwd', name, exact))
  x = O.acts(g, (N, H, W, cx), exact)
  dy = O.acts(g, (N, H, W, cy), exact)
  w = O.weights(g, (3, 3, cx, cy), exact)
  addt = O.acts(g, (N, H, W, cx), exact)
  dw0 = O.weights(g, (3, 3, cx, cy), True)
  db0 = O.weights(g, (cy,), True) + 3.0
  dw0[dw0 == 0] = 1.0
  x64, dy64 = x.double(), dy.double()
  xin = x64.clamp(min=0) if relu else x64
  dx = O.conv_dgrad(dy64, w.double(), 1, H, W, mask=x64 if mask else None,
                    add=addt.double() if add else None)
  mdx = mag_fwd(dy64, flip_t(w.double())) + (addt.double().abs() if add else 0)
  rw, rb = O.conv_wgrad(xin, dy64, 3, 1)
  TY, TX = tiles_of(H, W)
  return dict(N=N, caps=caps, H=H, W=W, cx=cx, cy=cy, relu=relu, mask=mask, x=x, dy=dy, w=w,
              add=addt if add else None, dw0=dw0, db0=db0, dx=dx, mdx=mdx,
              rw=rw + dw0.double(), rb=rb + db0.double(),
              mw=mag_wgrad(xin, dy64) + dw0.double().abs(),
              mb=dy64.abs().sum((0, 1, 2)) + db0.double().abs(), M=N * TY * TX, Mb=N * H * W)
