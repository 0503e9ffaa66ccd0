"""Float64 CPU oracles for the direct fp32 conv kernels (conv_f32.hip), their
case tables and the launch arithmetic of the direct launchers
(test_conv_f32_oracle.py on the CPU, test_conv_f32_direct_gpu.py on the GPU).

Everything is NHWC and float64 on the CPU with explicit TF-SAME pads, written
as plain loops over the K x K taps; nothing goes through
scalable_agent_amd.models.layers, torch.nn.functional's convolutions or the
GPU.  test_conv_f32_oracle.py checks each oracle against float64
torch.autograd.

Two input regimes.

Exact.  Activations and dY are integers in [-3, 3], weights and biases in
[-2, 2], uint8 frames take values in {0, 255} (x / 255 is exactly 0 or 1).
Every product and every partial sum of any subset of the terms is then an
integer whose magnitude is at most A, the same operation applied to
magnitudes.  Where A < 2^24 every such integer is a float32, so a float32
fused-multiply-add chain makes no rounding at all, whatever the order of the
terms, the number of weight-gradient slots or the split into tiles: the kernel
output must EQUAL the float64 oracle.  `exact_ok` is that precondition; the
CPU test asserts it for every GPU case.  Integer maps also have many exactly
tied pool windows, so the first-maximal-tap rule is tested on real ties.

Rounding.  Random normal inputs (uint8 frames uniform in 0..255).  The
elementwise bound is

  |out - ref| <= (M + 5) 2^-24 A

A as above (including |bias|, |add| and, for the accumulated weight
gradients, the starting value), M the number of accumulated terms: K K C for
a correlation over C source channels (forward: C = Cin; data gradient:
C = the channel count of dY), N Ho Wo for the weight and bias gradients.
Derivation: every product is rounded once (fma) and a sum of M terms in ANY
order and grouping - MFMA k-steps, per-wave pixel groups, per-workgroup slots,
the two-level slot tree - leaves each term under at most M - 1 additions, so to
first order the error is at most (M - 1) 2^-24 times the sum of magnitudes,
plus one unit for the product.  (The weight-gradient slot tree adds at most
12 levels to a chain of at most M / 3 terms: below M for every case here.)
The + 5 covers what is not a term of that sum: the x / 255 conversion of a
frame, the bias, the residual add, the read-modify-write of dW, and the up
to three additions of the pool-gradient gather that produce one source value.
The second-order part of (1 + 2^-24)^M is below 0.4 % of the bound at the
largest M here (62208) and the measured ratios sit far below 1.  ReLU and the
mask select are exact.  The max-pool is 1-Lipschitz in the maximum norm, so a
pooled value is off by at most the largest bound in its window; an argmax
code is compared only where the float64 window's two largest values differ by
more than twice that (both taps may move), which `argmax_clear` computes.
"""

import torch

U = 2.0 ** -24
EXACT_LIMIT = 2 ** 24


def ext():
  from scalable_agent_amd import ops
  return ops.ext()


def d64(t):
  return t.detach().to('cpu').to(torch.float64)


# ---------------------------------------------------------------- geometry

def same_out(n, s):
  return -(-n // s)


def same_pads(n, k, s):
  """TF-SAME (before, after) pads of a size-k, stride-s window over n."""
  total = max((same_out(n, s) - 1) * s + k - n, 0)
  return total // 2, total - total // 2


# ------------------------------------------------------------------ oracle

def _pad(x, pt, pb, pl, pr, value=0.0):
  N, H, W, C = x.shape
  xp = torch.full((N, H + pt + pb, W + pl + pr, C), value, dtype=x.dtype)
  xp[:, pt:pt + H, pl:pl + W] = x
  return xp


def _taps(xp, ky, kx, Ho, Wo, S):
  return xp[:, ky:ky + (Ho - 1) * S + 1:S, kx:kx + (Wo - 1) * S + 1:S]


def conv(x, w, b, S):
  """TF-SAME conv, x [N,H,W,Ci] float64, w HWIO [K,K,Ci,Co], b [Co] or None."""
  N, H, W, _ = x.shape
  K = w.shape[0]
  (pt, pb), (pl, pr) = same_pads(H, K, S), same_pads(W, K, S)
  Ho, Wo = same_out(H, S), same_out(W, S)
  xp = _pad(x, pt, pb, pl, pr)
  out = torch.zeros(N, Ho, Wo, w.shape[3], dtype=torch.float64)
  for ky in range(K):
    for kx in range(K):
      out += torch.einsum('nhwi,io->nhwo', _taps(xp, ky, kx, Ho, Wo, S), w[ky, kx])
  return out if b is None else out + b


def conv_dgrad(dy, w, S, H, W, mask=None, add=None):
  """dX [N,H,W,Ci] of conv(x, w, S) [* (mask > 0)] [+ add]."""
  N, Ho, Wo, _ = dy.shape
  K = w.shape[0]
  (pt, pb), (pl, pr) = same_pads(H, K, S), same_pads(W, K, S)
  # rows the last window reaches past the padded map are never read
  Hp = max(H + pt + pb, (Ho - 1) * S + K)
  Wp = max(W + pl + pr, (Wo - 1) * S + K)
  dxp = torch.zeros(N, Hp, Wp, w.shape[2], dtype=torch.float64)
  for ky in range(K):
    for kx in range(K):
      _taps(dxp, ky, kx, Ho, Wo, S).add_(torch.einsum('nhwo,io->nhwi', dy, w[ky, kx]))
  dx = dxp[:, pt:pt + H, pl:pl + W].clone()
  if mask is not None:
    dx = torch.where(mask > 0, dx, torch.zeros_like(dx))
  return dx if add is None else dx + add


def conv_wgrad(x, dy, K, S):
  """(dW HWIO, db) of conv(x, w, S) for the output gradient dy."""
  N, H, W, Ci = x.shape
  _, Ho, Wo, Co = dy.shape
  (pt, pb), (pl, pr) = same_pads(H, K, S), same_pads(W, K, S)
  xp = _pad(x, pt, pb, pl, pr)
  dw = torch.zeros(K, K, Ci, Co, dtype=torch.float64)
  for ky in range(K):
    for kx in range(K):
      dw[ky, kx] = torch.einsum('nhwi,nhwo->io', _taps(xp, ky, kx, Ho, Wo, S), dy)
  return dw, dy.sum((0, 1, 2))


def pool_windows(x):
  """The 3x3/2 TF-SAME windows of x: [N,Hp,Wp,C,9] (tap dy*3+dx, -inf pads)
  and the pads before."""
  N, H, W, C = x.shape
  (pbh, pah), (pbw, paw) = same_pads(H, 3, 2), same_pads(W, 3, 2)
  Hp, Wp = same_out(H, 2), same_out(W, 2)
  xp = _pad(x, pbh, pah, pbw, paw, value=float('-inf'))
  win = torch.stack([_taps(xp, dy, dx, Hp, Wp, 2) for dy in range(3) for dx in range(3)], -1)
  return win, pbh, pbw


def first_max(win):
  """(max, index of the FIRST maximal entry) along the last axis."""
  best = win.max(-1).values
  n = win.shape[-1]
  rank = (win == best.unsqueeze(-1)).long() * (n - torch.arange(n))
  return best, n - rank.max(-1).values


def maxpool(x):
  """3x3/2 TF-SAME max-pool: (pooled, first maximal tap code dy*3+dx)."""
  win, _, _ = pool_windows(x)
  return first_max(win)


def pool_gather(dP, code, H, W):
  """Gradient of the pool's input: dP routed to each window's argmax tap.  A
  position collects at most four windows; the kernels add them in ascending
  (py, px) order, which float64 (and the exact regime) does not depend on."""
  N, Hp, Wp, C = dP.shape
  pbh, pbw = same_pads(H, 3, 2)[0], same_pads(W, 3, 2)[0]
  dxp = torch.zeros(N, 2 * Hp + 1, 2 * Wp + 1, C, dtype=torch.float64)
  for dy in range(3):
    for dx in range(3):
      _taps(dxp, dy, dx, Hp, Wp, 2).add_(torch.where(code == dy * 3 + dx, dP,
                                                     torch.zeros_like(dP)))
  return dxp[:, pbh:pbh + H, pbw:pbw + W].clone()


# ------------------------------------------------------- bounds, exactness

def bound(M, A):
  return (M + 5) * U * A


def exact_ok(*mags):
  """The exact regime's precondition: every magnitude sum stays below 2^24."""
  return all(float(m.max()) < EXACT_LIMIT for m in mags)


def argmax_clear(win, win_bound):
  """Windows whose float64 maximum beats the runner-up by more than twice the
  largest bound in the window (pads carry bound 0)."""
  top2 = win.topk(2, dim=-1).values
  return (top2[..., 0] - top2[..., 1]) > 2 * win_bound.max(-1).values


def ratio(out, ref, bnd):
  """Largest |out - ref| / bound; NaN or inf in `out` gives inf."""
  out = d64(out)
  if not torch.isfinite(out).all():
    return float('inf')
  return float(((out - ref).abs() / bnd.clamp(min=1e-300)).max())


# ------------------------------------------------------------------ inputs

def gen(seed):
  return torch.Generator().manual_seed(seed)


def ints(g, shape, lim):
  return torch.randint(-lim, lim + 1, shape, generator=g).float()


def acts(g, shape, exact):
  return ints(g, shape, 3) if exact else torch.randn(shape, generator=g)


def weights(g, shape, exact):
  if exact:
    return ints(g, shape, 2)
  fan = 1
  for d in shape[:-1]:
    fan *= d
  return torch.randn(shape, generator=g) / fan ** 0.5 if len(shape) > 1 else \
      torch.randn(shape, generator=g) * 0.1


def frames(g, shape, exact):
  if exact:
    return (torch.randint(0, 2, shape, generator=g) * 255).to(torch.uint8)
  return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def source(g, N, H, W, C, u8, exact):
  """(tensor the kernel reads, its float64 value)."""
  if u8:
    x = frames(g, (N, H, W, C), exact)
    return x, x.double() / 255.0
  x = acts(g, (N, H, W, C), exact)
  return x, x.double()


def embed(t, dev):
  """t as the contiguous slice buf[1:1+N] of a NaN-filled (uint8: 0x7f-filled)
  GPU batch of N + 2 images: a read across the batch's ends poisons the
  output (or, for frames, changes it)."""
  N = t.shape[0]
  if t.dtype == torch.uint8:
    buf = torch.full((N + 2,) + tuple(t.shape[1:]), 127, dtype=torch.uint8, device=dev)
  else:
    buf = torch.full((N + 2,) + tuple(t.shape[1:]), float('nan'), dtype=t.dtype, device=dev)
  buf[1:1 + N] = t.to(dev)
  view = buf[1:1 + N]
  assert view.is_contiguous()
  return view


# ----------------------------------------------- launch arithmetic (host)
# What run_conv / run_conv_pool / run_wgrad / run_pool_wgrad compute for a
# shape with the grid cap at 0, redone here from their formulas: the GPU tests
# compare cf32_launch_info with it, so the hooks change no launch.

K_THREADS = 256
LDS_SOFT, LDS_HARD = 80 * 1024, 156 * 1024
CUS = 256


def _fwd_pitch(c):
  return c + 8 if c >= 16 else c


def _wg_pitch(c):
  return c + (48 - c % 32) % 32 if c >= 16 else c


def _fwd_maxc(c):
  return 16 if c >= 64 else (9 if c == 32 else 8)


def _occupancy(lds, cap):
  return max(1, min(cap, (160 * 1024) // (lds + 512)))


def cout_tile(cinp, cout, K):
  return 32 if cout % 32 == 0 and 4 * K * K * 32 * cinp <= 48 * 1024 else 16


def plan_conv(N, Ho, Wo, cinp, cout, K, S):
  """run_conv: Ho x Wo output rows of a K x K stride-S correlation over cinp
  staged channels, cout output channels."""
  ct = cout_tile(cinp, cout, K)
  PP, Wl = _fwd_pitch(cinp), (Wo - 1) * S + K
  nbytes = lambda R: 4 * K * K * ct * cinp + 4 * ((R - 1) * S + K) * Wl * PP
  budget = LDS_SOFT if nbytes(1) <= LDS_SOFT else LDS_HARD
  best, best_cost = 0, 1e30
  for R in range(1, Ho + 1):
    rows = (R - 1) * S + K
    if (nbytes(R) > budget or rows * Wl * (cinp // 4) > _fwd_maxc(cinp) * K_THREADS or
        (R * Wo + 15) // 16 > 16):
      break
    nt = -(-Ho // R)
    cost = sum(((min(R, Ho - t * R) * Wo + 15) // 16 + 3) // 4 + 0.4 for t in range(nt))
    if cost < best_cost - 1e-9:
      best, best_cost = R, cost
  assert best > 0
  R, nt, gy = best, -(-Ho // best), cout // ct
  per_cu = _occupancy(nbytes(R), 3 if cinp <= 16 and ct <= 16 else 2)
  return dict(family='conv_fwd', grid_x=max(1, min(N * nt, CUS * per_cu // gy)), grid_y=gy,
              ntiles=N * nt, rows=R, tiles_per_img=nt)


def plan_conv_pool(N, H, W, cinp, cout):
  PP, Wl = _fwd_pitch(cinp), W + 2
  Hp = (H + 1) // 2
  nbytes = lambda R: 4 * (9 * cinp * cout + (2 * R + 3) * Wl * PP +
                          (2 * R + 1) * (W + 2) * (cout + 4))
  budget = LDS_SOFT if nbytes(2) <= LDS_SOFT else LDS_HARD
  R = 0
  for r in range(1, min(Hp, 2 if cinp == 4 else 1 << 20) + 1):
    if nbytes(r) > budget or (2 * r + 3) * Wl * (cinp // 4) > 8 * K_THREADS:
      break
    R = r
  assert R > 0
  nt = -(-Hp // R)
  R = -(-Hp // nt)
  per_cu = _occupancy(nbytes(R), 3)
  return dict(family='conv_pool_fwd', grid_x=max(1, min(N * nt, CUS * per_cu)), grid_y=1,
              ntiles=N * nt, rows=R, tiles_per_img=nt)


# (cinp, K, S, Cout) -> (NTT, WSM) of conv_launch's SA_WG_CASE table
WG_CASES = {(4, 3, 1, 16): (1, 1), (4, 8, 4, 32): (2, 2), (4, 3, 1, 32): (2, 1),
            (16, 3, 1, 16): (1, 1), (16, 3, 1, 32): (2, 1), (32, 3, 1, 32): (2, 2),
            (32, 4, 2, 64): (4, 4), (64, 3, 2, 128): (4, 4)}


def wgrad_slots(K, cinp, cout):
  rows = ((K * K * cinp + 16) // 16) * 16
  return max(128, min(512, (8 << 20) // (rows * cout)))


def plan_wgrad(N, Ho, Wo, cinp, cout, K, S):
  NTT, WSM = WG_CASES[(cinp, K, S, cout)]
  MT = (K * K * cinp + 16) // 16
  XP, CG = _wg_pitch(cinp), NTT * 16
  DP = CG + 16 if CG % 32 == 0 else CG
  Wl = (Wo - 1) * S + K
  red = 4 * MT * 16 * CG if 4 // WSM > 1 else 0
  nbytes = lambda R: max(red, 4 * (((R - 1) * S + K) * Wl * XP + R * Wo * DP))
  budget = LDS_SOFT if nbytes(1) <= LDS_SOFT else LDS_HARD
  Rmax = 0
  for R in range(1, Ho + 1):
    if (nbytes(R) > budget or ((R - 1) * S + K) * Wl * (cinp // 4) > 8 * K_THREADS or
        R * Wo * (CG // 4) > 8 * K_THREADS):
      break
    Rmax = R
  assert Rmax > 0
  nt = -(-Ho // Rmax)
  R = -(-Ho // nt)
  return dict(family='conv_wgrad', grid_x=min(N * nt, wgrad_slots(K, cinp, cout)),
              grid_y=cout // CG, ntiles=N * nt, rows=R, tiles_per_img=nt)


def plan_pool_wgrad(N, H, W):
  tpi = -(-((H + 1) // 2) // 2)
  return dict(family='pool_wgrad', grid_x=min(N * tpi, 1280), grid_y=1, ntiles=N * tpi,
              rows=2, tiles_per_img=tpi)


def pick_n(tpi, cap=3, lo=2, hi=9):
  """Fewest images in [lo, hi] whose tile count gives `cap` workgroups at
  least two full sweeps plus a ragged third (ntiles >= 2 cap + 1, ntiles not
  a multiple of cap); None where tpi is a multiple of cap."""
  for n in range(lo, hi + 1):
    if n * tpi >= 2 * cap + 1 and (n * tpi) % cap != 0:
      return n
  return None


# ------------------------------------------------------------------- cases
# Every GPU case of test_conv_f32_direct_gpu.py, with its inputs and float64
# references built here (once per process, shared, never modified), so the CPU
# test can check the exact regime's precondition and the argmax shares for
# exactly what the GPU runs.

import functools
import os
import zlib

CAP = 3


def _seed(*key):
  return zlib.crc32(repr(key).encode()) & 0x7fffffff


def caps_and_n(tpi):
  """(N, caps) of a multi-tile case of `tpi` tiles per image.  The capped run
  uses 3 workgroups with ntiles >= 7 and ntiles % 3 != 0.  Where the launcher
  cuts an image into a multiple of 3 tiles no N gives a ragged last sweep on
  3 workgroups: such cases also run on 4, 5 or 7 workgroups (the first for
  which some N in 2..9 leaves a remainder), with N taken from that."""
  n = pick_n(tpi, CAP)
  if n is not None:
    return n, (CAP,)
  for cap in (4, 5, 7):
    n = pick_n(tpi, cap)
    if n is not None and n * tpi >= 2 * CAP + 1:
      return n, (CAP, cap)
  raise AssertionError(tpi)


def dgrad_mode():
  """Which strided data-gradient form this process runs (the switches are
  read once per process by the extension)."""
  if os.environ.get('SA_F32_DGRAD_PHASE', '') == '0':
    return 'dilated'
  if os.environ.get('SA_F32_DGRAD_STACK', '') == '1':
    return 'stack'
  return 'phase'


# name: (H, W, Cs, Cout, K, S, uint8 source).  All reach conv_fwd_kernel in a
# default process: uint8 and 4-channel sources, strides > 1 and 32 -> 16 have
# no Winograd instance, and the 7x9 maps are declined by the Winograd
# launcher (a 64-tile range would touch more than 4 images).
FWD_CASES = {
    's1_u8c3_72x96': (72, 96, 3, 32, 8, 4, True),
    's1_u8c4_72x96': (72, 96, 4, 32, 8, 4, True),
    's1_f32_72x96': (72, 96, 4, 32, 8, 4, False),
    's1_u8c3_84x84': (84, 84, 3, 32, 8, 4, True),
    's1_u8c4_84x84': (84, 84, 4, 32, 8, 4, True),
    's1_f32_84x84': (84, 84, 4, 32, 8, 4, False),
    's2_18x24': (18, 24, 32, 64, 4, 2, False),
    's2_21x21': (21, 21, 32, 64, 4, 2, False),
    's2_c16_21x21': (21, 21, 32, 16, 4, 2, False),   # the 16-wide 4x4/2 tile
    's3_9x12': (9, 12, 64, 128, 3, 2, False),        # W pad 0/1
    's3_11x11': (11, 11, 64, 128, 3, 2, False),
    'd1_u8c3_72x96': (72, 96, 3, 16, 3, 1, True),
    'd1_u8c3_72x128': (72, 128, 3, 16, 3, 1, True),
    'd1_f32_20x24': (20, 24, 4, 16, 3, 1, False),
    'r32to16_18x24': (18, 24, 32, 16, 3, 1, False),
    'r16_7x9': (7, 9, 16, 16, 3, 1, False),
    'h16to32_7x9': (7, 9, 16, 32, 3, 1, False),
    'r32_7x9': (7, 9, 32, 32, 3, 1, False),
}
# SA_F32_WINO=0 only (the Winograd kernels take these in a default process)
WINO_OFF_CASES = {
    'r16_36x48': (36, 48, 16, 16, 3, 1, False),
    'h16to32_36x48': (36, 48, 16, 32, 3, 1, False),
    'r32_18x24': (18, 24, 32, 32, 3, 1, False),
    'r16_11x11': (11, 11, 16, 16, 3, 1, False),
    'r32_11x11': (11, 11, 32, 32, 3, 1, False),
    'r16_18x24': (18, 24, 16, 16, 3, 1, False),
}
ALL_FWD = dict(FWD_CASES, **WINO_OFF_CASES)
# (bias, relu_in, add, relu_out)
FWD_FLAGS = {'none': (False, False, False, False), 'bias': (True, False, False, False),
             'relu': (True, True, False, True), 'add': (True, False, True, True)}
# Which forward cases have a last tile of fewer than R rows / a last 16-pixel
# group with fewer than 16 pixels (from plan_conv; the CPU test checks both
# lists against it).  R and the width are the launcher's, so not every shape
# can have both; between them the shapes cover both in every kernel family.
FWD_SHORT_TILE = ('s1_u8c3_72x96', 's1_u8c4_72x96', 's1_f32_72x96', 's2_21x21', 's2_c16_21x21',
                  'r32to16_18x24', 'r32_18x24', 'r16_18x24')
FWD_RAGGED_GROUP = ('s1_u8c3_84x84', 's1_u8c4_84x84', 's1_f32_84x84', 's2_18x24', 's2_21x21',
                    's2_c16_21x21', 's3_9x12', 's3_11x11', 'r16_7x9', 'h16to32_7x9', 'r32_7x9',
                    'r16_11x11', 'r32_11x11')


def fwd_geom(name):
  H, W, Cs, Cout, K, S, u8 = ALL_FWD[name]
  Ho, Wo = same_out(H, S), same_out(W, S)
  plan1 = plan_conv(1, Ho, Wo, 4 if u8 else Cs, Cout, K, S)
  N, caps = caps_and_n(plan1['tiles_per_img'])
  return dict(H=H, W=W, Cs=Cs, Cout=Cout, K=K, S=S, u8=u8, Ho=Ho, Wo=Wo, N=N, caps=caps,
              pt=same_pads(H, K, S)[0], pl=same_pads(W, K, S)[0],
              plan=plan_conv(N, Ho, Wo, 4 if u8 else Cs, Cout, K, S))


@functools.lru_cache(maxsize=None)
def fwd_data(name, exact):
  q = fwd_geom(name)
  g = gen(_seed('fwd', name, exact))
  x, x64 = source(g, q['N'], q['H'], q['W'], q['Cs'], q['u8'], exact)
  w = weights(g, (q['K'], q['K'], q['Cs'], q['Cout']), exact)
  b = weights(g, (q['Cout'],), exact)
  add = acts(g, (q['N'], q['Ho'], q['Wo'], q['Cout']), exact)
  lin = conv(x64, w.double(), None, q['S'])
  lin_relu = conv(x64.clamp(min=0), w.double(), None, q['S'])
  mag = conv(x64.abs(), w.double().abs(), None, q['S'])
  return dict(q, x=x, w=w, b=b, add=add, lin=lin, lin_relu=lin_relu, mag=mag,
              M=q['K'] * q['K'] * q['Cs'])


def fwd_ref(d, flags):
  """(float64 reference, magnitude A) of a forward case under a flag set."""
  bias, relu_in, add, relu_out = FWD_FLAGS[flags]
  relu_in = relu_in and not d['u8']  # frames are never ReLU'd
  ref = (d['lin_relu'] if relu_in else d['lin']).clone()
  A = d['mag'].clone()
  if bias:
    ref += d['b'].double()
    A += d['b'].double().abs()
  if add:
    ref += d['add'].double()
    A += d['add'].double().abs()
  if relu_out:
    ref = ref.clamp(min=0)
  return ref, A


# name: (H, W, Cin, Cout, K, S, pooled) - the data gradient of conv Cin -> Cout;
# pooled: dY is the gradient of the conv output's 3x3/2 max-pool (pool_arg).
DGRAD_CASES = {
    's2_18x24': (18, 24, 32, 64, 4, 2, False),     # 2x2 phase sub-kernels, 64 -> 32
    's2_21x21': (21, 21, 32, 64, 4, 2, False),
    's3_9x12': (9, 12, 64, 128, 3, 2, False),      # 2x2 phase sub-kernels, 128 -> 64
    's3_11x11': (11, 11, 64, 128, 3, 2, False),
    'k4s1_9x12': (9, 12, 32, 64, 4, 1, False),     # the 4x4 form (64 -> 16-wide tiles)
    'k3s1_c128_9x12': (9, 12, 64, 128, 3, 1, False),  # the 3x3 form over 128 channels
    'h16to32_36x48': (36, 48, 16, 32, 3, 1, False),   # 32 -> 16: no Winograd instance
    'r16_7x9': (7, 9, 16, 16, 3, 1, False),        # declined by the Winograd launcher
    'r32_7x9': (7, 9, 32, 32, 3, 1, False),
    'pool_h16to32_36x48': (36, 48, 16, 32, 3, 1, True),
    'pool_h16to32_42x42': (42, 42, 16, 32, 3, 1, True),
    'pool_h32_18x24': (18, 24, 32, 32, 3, 1, True),
    'pool_h32_21x21': (21, 21, 32, 32, 3, 1, True),
}
WINO_OFF_DGRAD = {
    'r16_36x48': (36, 48, 16, 16, 3, 1, False),
    'r32_18x24': (18, 24, 32, 32, 3, 1, False),
    'r16_11x11': (11, 11, 16, 16, 3, 1, False),
    'r32_11x11': (11, 11, 32, 32, 3, 1, False),
}
ALL_DGRAD = dict(DGRAD_CASES, **WINO_OFF_DGRAD)


def dgrad_last_launch(H, W, Cin, Cout, K, S, mode):
  """(Ho, Wo, staged channels, output channels, K) of the LAST conv_fwd
  launch of cf32_conv_dgrad (bindings: conv_dgrad)."""
  if S == 1 or mode == 'dilated':
    return H, W, Cout, Cin, K
  pt, pl = same_pads(H, K, S)[0], same_pads(W, K, S)[0]
  Kq = -(-K // S)
  lo = lambda p, r: max(p - r + S - 1, 0) // S
  hi = lambda n, p, r: (n - 1 + p - r) // S
  if mode == 'stack':
    ho = max(hi(H, pt, r) for r in range(S)) - min(lo(pt, r) for r in range(S)) + 1
    wo = max(hi(W, pl, r) for r in range(S)) - min(lo(pl, r) for r in range(S)) + 1
    return ho, wo, Cout, S * S * Cin, Kq
  r = S - 1
  return hi(H, pt, r) - lo(pt, r) + 1, hi(W, pl, r) - lo(pl, r) + 1, Cout, Cin, Kq


def dgrad_geom(name, mode='phase'):
  H, W, Cin, Cout, K, S, pooled = ALL_DGRAD[name]
  ll = dgrad_last_launch(H, W, Cin, Cout, K, S, mode)
  plan1 = plan_conv(1, ll[0], ll[1], ll[2], ll[3], ll[4], 1)
  N, caps = caps_and_n(plan1['tiles_per_img'])
  return dict(H=H, W=W, Cin=Cin, Cout=Cout, K=K, S=S, pooled=pooled, N=N, caps=caps,
              Ho=same_out(H, S), Wo=same_out(W, S),
              pt=same_pads(H, K, S)[0], pl=same_pads(W, K, S)[0],
              plan=plan_conv(N, ll[0], ll[1], ll[2], ll[3], ll[4], 1))


def pool_codes(g, N, H, W, C, exact):
  """Argmax codes of a real pre-pool map (ties included in the exact regime)."""
  pre = acts(g, (N, H, W, C), exact).double()
  return maxpool(pre)[1]


@functools.lru_cache(maxsize=None)
def dgrad_data(name, exact, mode='phase'):
  q = dgrad_geom(name, mode)
  g = gen(_seed('dgrad', name, exact))
  N, H, W = q['N'], q['H'], q['W']
  w = weights(g, (q['K'], q['K'], q['Cin'], q['Cout']), exact)
  mask = acts(g, (N, H, W, q['Cin']), exact)
  add = acts(g, (N, H, W, q['Cin']), exact)
  code = None
  if q['pooled']:
    code = pool_codes(g, N, H, W, q['Cout'], exact)
    dy = acts(g, tuple(code.shape), exact)
    dy64 = pool_gather(dy.double(), code, H, W)
    dymag = pool_gather(dy.double().abs(), code, H, W)
  else:
    dy = acts(g, (N, q['Ho'], q['Wo'], q['Cout']), exact)
    dy64, dymag = dy.double(), dy.double().abs()
  lin = conv_dgrad(dy64, w.double(), q['S'], H, W)
  mag = conv_dgrad(dymag, w.double().abs(), q['S'], H, W)
  return dict(q, w=w, dy=dy, mask=mask, add=add, code=code, lin=lin, mag=mag,
              M=q['K'] * q['K'] * q['Cout'])


def dgrad_ref(d, masked):
  if not masked:
    return d['lin'], d['mag']
  ref = torch.where(d['mask'].double() > 0, d['lin'], torch.zeros_like(d['lin']))
  return ref + d['add'].double(), d['mag'] + d['add'].double().abs()


# name: (H, W, Cs, Cout, uint8 source): conv3x3/1 + bias + 3x3/2 max-pool
POOL_CASES = {
    'u8c3_72x96': (72, 96, 3, 16, True),
    'f32_72x96': (72, 96, 4, 16, False),
    'u8c4_84x84': (84, 84, 4, 16, True),
    'f32_84x84': (84, 84, 4, 16, False),
    'h16to32_42x42': (42, 42, 16, 32, False),
    'h16to32_36x48': (36, 48, 16, 32, False),
    'h32_21x21': (21, 21, 32, 32, False),
    'h32_18x24': (18, 24, 32, 32, False),
}


def pool_geom(name):
  H, W, Cs, Cout, u8 = POOL_CASES[name]
  cinp = 4 if u8 else Cs
  N, caps = caps_and_n(plan_conv_pool(1, H, W, cinp, Cout)['tiles_per_img'])
  return dict(H=H, W=W, Cs=Cs, Cout=Cout, u8=u8, N=N, caps=caps,
              pbh=same_pads(H, 3, 2)[0], pbw=same_pads(W, 3, 2)[0],
              plan=plan_conv_pool(N, H, W, cinp, Cout))


@functools.lru_cache(maxsize=None)
def pool_data(name, exact):
  q = pool_geom(name)
  g = gen(_seed('pool', name, exact))
  x, x64 = source(g, q['N'], q['H'], q['W'], q['Cs'], q['u8'], exact)
  w = weights(g, (3, 3, q['Cs'], q['Cout']), exact)
  b = weights(g, (q['Cout'],), exact)
  pre = conv(x64, w.double(), b.double(), 1)
  bnd = bound(9 * q['Cs'], conv(x64.abs(), w.double().abs(), b.double().abs(), 1))
  win, _, _ = pool_windows(pre)
  # bounds of the window's taps; the -inf pads carry none
  wb = pool_windows(bnd)[0].clamp(min=0)
  val, code = first_max(win)
  return dict(q, x=x, w=w, b=b, pre=pre, pre_bound=bnd, val=val, code=code,
              val_bound=wb.max(-1).values, clear=argmax_clear(win, wb))


# name: (H, W, Cs, Cout, K, S, uint8 source, relu_in, dw_cin, pooled)
WGRAD_CASES = {
    'd1_u8c3_72x96': (72, 96, 3, 16, 3, 1, True, False, 3, False),    # (4,3,1,u8,16)
    'd1_f32_cin3_72x96': (72, 96, 4, 16, 3, 1, False, False, 3, False),  # (4,3,1,f32,16), dw_cin 3
    'd1_f32_84x84': (84, 84, 4, 16, 3, 1, False, False, 4, False),
    's1_f32_72x96': (72, 96, 4, 32, 8, 4, False, False, 4, False),    # (4,8,4,f32,32)
    's1_u8c3_72x96': (72, 96, 3, 32, 8, 4, True, False, 3, False),    # (4,8,4,u8,32)
    's1_u8c4_84x84': (84, 84, 4, 32, 8, 4, True, False, 4, False),
    'u8c3to32_72x96': (72, 96, 3, 32, 3, 1, True, False, 3, False),   # (4,3,1,u8,32)
    'r16_36x48': (36, 48, 16, 16, 3, 1, False, True, 16, False),      # (16,3,1,f32,16)
    'h16to32_36x48': (36, 48, 16, 32, 3, 1, False, False, 16, False),  # (16,3,1,f32,32)
    'h16to32_42x42_relu': (42, 42, 16, 32, 3, 1, False, True, 16, False),
    'r32_7x9': (7, 9, 32, 32, 3, 1, False, True, 32, False),          # (32,3,1,f32,32), Winograd declines
    's2_18x24': (18, 24, 32, 64, 4, 2, False, True, 32, False),       # (32,4,2,f32,64)
    's2_21x21': (21, 21, 32, 64, 4, 2, False, False, 32, False),
    's3_9x12': (9, 12, 64, 128, 3, 2, False, True, 64, False),        # (64,3,2,f32,128)
    's3_11x11': (11, 11, 64, 128, 3, 2, False, False, 64, False),
    # dY gathered from (dP, argmax): the GATHER instances
    'pool_h16to32_36x48': (36, 48, 16, 32, 3, 1, False, False, 16, True),
    'pool_h16to32_42x42': (42, 42, 16, 32, 3, 1, False, False, 16, True),
    'pool_h32_18x24': (18, 24, 32, 32, 3, 1, False, False, 32, True),
    'pool_h32_21x21': (21, 21, 32, 32, 3, 1, False, False, 32, True),
    # stage 0 from (dP, argmax): pool_wgrad_kernel (scatter), or with
    # SA_F32_POOL_SCATTER=0 the GATHER instance of conv_wgrad_kernel
    'stage0_u8c3_72x96': (72, 96, 3, 16, 3, 1, True, False, 3, True),
    'stage0_u8c4_84x84': (84, 84, 4, 16, 3, 1, True, False, 4, True),
    'stage0_f32_72x96': (72, 96, 4, 16, 3, 1, False, False, 4, True),
    'stage0_f32_cin3_84x84': (84, 84, 4, 16, 3, 1, False, False, 3, True),
}


def scatter_on():
  return os.environ.get('SA_F32_POOL_SCATTER', '') != '0'


def wgrad_geom(name, scatter=True):
  H, W, Cs, Cout, K, S, u8, relu_in, dw_cin, pooled = WGRAD_CASES[name]
  cinp = 4 if u8 else Cs
  Ho, Wo = same_out(H, S), same_out(W, S)
  if name.startswith('stage0') and scatter:
    planf = lambda n: plan_pool_wgrad(n, H, W)
  else:
    planf = lambda n: plan_wgrad(n, Ho, Wo, cinp, Cout, K, S)
  N, caps = caps_and_n(planf(1)['tiles_per_img'])
  return dict(H=H, W=W, Cs=Cs, Cout=Cout, K=K, S=S, u8=u8, relu_in=relu_in, dw_cin=dw_cin,
              pooled=pooled, Ho=Ho, Wo=Wo, N=N, caps=caps, plan=planf(N),
              pt=same_pads(H, K, S)[0], pl=same_pads(W, K, S)[0])


@functools.lru_cache(maxsize=None)
def wgrad_data(name, exact, scatter=True):
  q = wgrad_geom(name, scatter)
  g = gen(_seed('wgrad', name, exact))
  N, H, W, K = q['N'], q['H'], q['W'], q['K']
  x, x64 = source(g, N, H, W, q['Cs'], q['u8'], exact)
  if q['dw_cin'] < q['Cs']:
    x[..., q['dw_cin']:] = 0   # the image's pad channel
    x64[..., q['dw_cin']:] = 0
  code = None
  if q['pooled']:
    code = pool_codes(g, N, H, W, q['Cout'], exact)
    dy = acts(g, tuple(code.shape), exact)
    dy64 = pool_gather(dy.double(), code, H, W)
    dymag = pool_gather(dy.double().abs(), code, H, W)
  else:
    dy = acts(g, (N, q['Ho'], q['Wo'], q['Cout']), exact)
    dy64, dymag = dy.double(), dy.double().abs()
  dw0 = weights(g, (K, K, q['dw_cin'], q['Cout']), True)  # known non-zero start
  db0 = weights(g, (q['Cout'],), True) + 3.0
  dw0[dw0 == 0] = 1.0
  xin = x64.clamp(min=0) if q['relu_in'] else x64
  rw, rb = conv_wgrad(xin, dy64, K, q['S'])
  mw, mb = conv_wgrad(xin.abs(), dymag, K, q['S'])
  c = q['dw_cin']
  return dict(q, x=x, dy=dy, code=code, dw0=dw0, db0=db0,
              rw=rw[:, :, :c] + dw0.double(), rb=rb + db0.double(),
              mw=mw[:, :, :c] + dw0.double().abs(), mb=mb + db0.double().abs(),
              M=N * q['Ho'] * q['Wo'])


# (N, H, W): even and odd maps, pad-before 0 and 1 on each axis
MAXPOOL_SHAPES = ((2, 10, 12), (2, 9, 11), (3, 9, 12), (2, 12, 7))
MAXPOOL_CHANNELS = (16, 32, 64, 128)


@functools.lru_cache(maxsize=None)
def maxpool_data(shape, C, exact):
  N, H, W = shape
  g = gen(_seed('maxpool', shape, C, exact))
  x = acts(g, (N, H, W, C), exact)
  val, code = maxpool(x.double())
  dy = acts(g, tuple(val.shape), exact)
  return dict(x=x, val=val, code=code, dy=dy, H=H, W=W,
              pbh=same_pads(H, 3, 2)[0], pbw=same_pads(W, 3, 2)[0],
              dx=pool_gather(dy.double(), code, H, W),
              dxmag=pool_gather(dy.double().abs(), code, H, W))
