"""Float64 CPU oracle and launch helpers for the bf16 conv-torso op tests
(test_conv_persistent_gpu.py, test_conv_pool_argmax_gpu.py).

Everything here is NHWC and float64 on the CPU, written with explicit TF-SAME
pads; nothing goes through scalable_agent_amd.models.layers or the GPU.

Output bound (bf16 outputs y, t, pooled, dx), elementwise:

  |out - ref| <= 2^-8 |ref| + 9 K 2^-23 A

A is the same convolution applied to magnitudes (plus |b|, |resid| or
|skip|), K the input channel count of the layer.  Derivation: the inputs are
bf16, so every product is exact in fp32; the fp32 accumulation of the 9 K
products (any order, MFMA included) is off by at most 9 K 2^-24 A, doubled
for the bias / residual additions and slack; the rounding to bf16 (8
significant bits, unit roundoff 2^-8) costs at most 2^-8 |ref|.  Round-to-
nearest reaches that worst case just above a power of two (half an ulp of
2^-7 against a value of 1 + epsilon), so over a million outputs the largest
error / bound ratio sits near 0.98-0.99 by construction; a kernel that
truncated instead (up to 2^-7 |ref|) would exceed the bound.
"""

import contextlib

import torch
import torch.nn.functional as F

REL = 2.0 ** -8
ACC = 2.0 ** -23


def ext():
  from scalable_agent_amd import ops
  return ops.ext()


def pool_pb(n):
  """TF-SAME pad-before of a 3x3 / stride-2 pool over n positions."""
  out = (n + 1) // 2
  return max((out - 1) * 2 + 3 - n, 0) // 2


def d64(t):
  return t.detach().to('cpu').to(torch.float64)


# ------------------------------------------------------------------- knobs

@contextlib.contextmanager
def tuned(C, **knobs):
  """conv_tune knobs set for the block and restored after it."""
  prev = {}
  try:
    for k, v in knobs.items():
      prev[k] = C.conv_tune(k, v)
      assert prev[k] >= 0, k
    yield
  finally:
    for k, v in prev.items():
      C.conv_tune(k, v)


@contextlib.contextmanager
def small_grid(C):
  """About 128 persistent workgroups: 16 of 32 CUs per XCD reserved and one
  resident workgroup per CU, so a few hundred tiles give every workgroup a
  second and third tile."""
  prev_res = C.cf32_cu_reserve(16)
  try:
    with tuned(C, cap_fwd=1, cap_bwd=1):
      yield
  finally:
    C.cf32_cu_reserve(prev_res)


def record(C, family, out=None):
  """The launch record of `family`, printed (pytest -s / -rA collects the
  grid, ntiles and rows that actually ran)."""
  rec = C.conv_launch_info(family)
  assert rec['family'] == family, rec
  if out is not None:
    print('CONVREC %s %s grid=%d ntiles=%d rows=%d specialized=%d' %
          (family, out, rec['grid'], rec['ntiles'], rec['rows'],
           rec['specialized']))
  return rec


def pick_n(tpi, gmax, mode):
  """Images for a launch of `tpi` tiles per image on at most `gmax`
  workgroups.  'one': every workgroup runs one tile (control).  'plus': the
  fewest images with more tiles than workgroups; ntiles - gmax workgroups
  then run a second tile.  That is exactly one workgroup (gmax + 1 tiles)
  only where tpi divides gmax + 1, i.e. at the shapes of 1 or 3 tiles per
  image; whole images of 5, 6 or 9 tiles overshoot 128 workgroups by 2 to 7
  tiles, and no CU reserve makes 256 - 8 r one less than a multiple of 6.
  'x2.4': about 2.4 tiles per workgroup with an odd tile count (tpi even:
  not a multiple of 8), so XCD ranges have fractional bounds."""
  if mode == 'one':
    return max(gmax // tpi, 1)
  if mode == 'plus':
    return gmax // tpi + 1
  assert mode == 'x2.4', mode
  n = max(int(round(2.4 * gmax / tpi)), gmax // tpi + 1)
  bad = (lambda t: t % 2 == 0) if tpi % 2 else (lambda t: t % 8 == 0)
  while bad(n * tpi):
    n += 1
  return n


# ------------------------------------------------------------------ oracle

def conv64(x, w, b=None):
  """3x3 stride-1 conv, TF SAME (one zero pixel each side)."""
  xc = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1))
  y = F.conv2d(xc, w.permute(3, 2, 0, 1).contiguous(), b)
  return y.permute(0, 2, 3, 1).contiguous()


def dgrad64(dy, w):
  """dX[q, ci] = sum_tap W[tap][ci][co] dY[q - (tap - centre)][co]."""
  return conv64(dy, w.flip(0, 1).transpose(2, 3).contiguous())


def wgrad64(x, dy):
  """dW[ky, kx, ci, co] = sum_q x[q + (ky - 1, kx - 1)][ci] dY[q][co]."""
  N, H, W, _ = x.shape
  xp = F.pad(x, (0, 0, 1, 1, 1, 1))
  dw = torch.empty(3, 3, x.shape[3], dy.shape[3], dtype=torch.float64)
  dyf = dy.reshape(-1, dy.shape[3])
  for ky in range(3):
    for kx in range(3):
      xs = xp[:, ky:ky + H, kx:kx + W].reshape(-1, x.shape[3])
      dw[ky, kx] = xs.t() @ dyf
  return dw


def pool_taps(y, pb_h, pb_w, fill=float('-inf')):
  """[N, Hp, Wo, C, 9] taps (dy*3+dx order) of the 3x3/2 windows; window
  (i, j) starts at conv position (2i - pb_h, 2j - pb_w); taps outside the
  image hold `fill`."""
  N, H, W, C = y.shape
  Hp, Wo = (H + 1) // 2, (W + 1) // 2
  rows, cols = 2 * (Hp - 1) + 3, 2 * (Wo - 1) + 3
  assert rows >= pb_h + H and cols >= pb_w + W
  yp = torch.full((N, rows, cols, C), fill, dtype=y.dtype)
  yp[:, pb_h:pb_h + H, pb_w:pb_w + W] = y
  taps = [yp[:, dy:dy + 2 * Hp - 1:2, dx:dx + 2 * Wo - 1:2]
          for dy in range(3) for dx in range(3)]
  return torch.stack(taps, dim=-1)


def pool64(y, pb_h, pb_w):
  """(pooled, code): max and the FIRST maximal in-image tap (dy*3+dx)."""
  taps = pool_taps(y, pb_h, pb_w)
  best = torch.full(taps.shape[:-1], float('-inf'), dtype=y.dtype)
  code = torch.full(taps.shape[:-1], -1, dtype=torch.long)
  for k in range(9):
    v = taps[..., k]
    better = v > best  # strict: an equal later tap never replaces the first
    best = torch.where(better, v, best)
    code = torch.where(better, torch.full_like(code, k), code)
  assert int(code.min()) >= 0
  return best, code


def tap_positions(code, H, W, pb_h, pb_w):
  """Conv row / column every window's code points at, decoded WITHOUT
  clamping; asserts that all of them lie inside the image."""
  code = code.to('cpu').long()
  N, Hp, Wo, C = code.shape
  assert int(code.min()) >= 0 and int(code.max()) <= 8, \
      'argmax code outside 0..8: [%d, %d]' % (int(code.min()), int(code.max()))
  i = torch.arange(Hp).view(1, Hp, 1, 1)
  j = torch.arange(Wo).view(1, 1, Wo, 1)
  r = 2 * i - pb_h + code // 3
  c = 2 * j - pb_w + code % 3
  bad = (r < 0) | (r >= H) | (c < 0) | (c >= W)
  assert not bool(bad.any()), \
      '%d argmax codes point outside the %dx%d image' % (int(bad.sum()), H, W)
  return r, c


def scatter64(dP, code, H, W, pb_h, pb_w):
  """dY[N, H, W, C] in float64: every pooled gradient added at the conv
  position its code names (indices asserted in range: no wrap-around)."""
  r, c = tap_positions(code, H, W, pb_h, pb_w)
  N, Hp, Wo, C = dP.shape
  n = torch.arange(N).view(N, 1, 1, 1).expand_as(r)
  ch = torch.arange(C).view(1, 1, 1, C).expand_as(r)
  dY = torch.zeros(N, H, W, C, dtype=torch.float64)
  dY.index_put_((n.reshape(-1), r.reshape(-1), c.reshape(-1), ch.reshape(-1)),
                d64(dP).reshape(-1), accumulate=True)
  return dY


# ------------------------------------------------------------------ checks

def check_bound(out, ref, A, K, what, extra=None):
  """|out - ref| <= 2^-8 |ref| + 9 K 2^-23 A elementwise; prints the largest
  error / bound ratio.  `extra` (a tensor like ref) is added to the bound
  where the caller derives a further term."""
  out = d64(out)
  assert out.shape == ref.shape, (out.shape, ref.shape)
  assert bool(torch.isfinite(out).all()), what
  err = (out - ref).abs()
  bound = REL * ref.abs() + 9 * K * ACC * A
  if extra is not None:
    bound = bound + extra
  ratio = float((err / bound.clamp_min(1e-300)).max())
  print('CONVERR %s ratio=%.4f' % (what, ratio))
  over = err > bound
  assert not bool(over.any()), \
      '%s: %d elements over the bound, worst ratio %.3f' % (what, int(over.sum()), ratio)
  return ratio


def check_max(a, ref, tol, what):
  """max |a - ref| <= tol * max |ref| (the suite's bound for fp32 grads)."""
  a, ref = d64(a), d64(ref)
  err = float((a - ref).abs().max())
  scale = max(float(ref.abs().max()), 1e-30)
  print('CONVERR %s maxerr/scale=%.3g tol=%.0e' % (what, err / scale, tol))
  assert err <= tol * scale, '%s: max err %.4g vs scale %.4g' % (what, err, scale)


def bits_equal(a, b, what):
  assert a.dtype == b.dtype and a.shape == b.shape, what
  if a.dtype == torch.bfloat16:
    a, b = a.view(torch.int16), b.view(torch.int16)
  elif a.dtype == torch.float32:
    a, b = a.view(torch.int32), b.view(torch.int32)
  n = int((a != b).sum())
  assert n == 0, '%s: %d elements differ bitwise' % (what, n)


# ----------------------------------------------------------------- geometry

def is_compiled(family, C, H, W):
  """Whether the launchers hold a compile-time geometry for this map."""
  if family.startswith('conv1'):
    return (H, W) in ((72, 96), (72, 128), (84, 84))
  if C == 16:
    return (H, W) in ((36, 48), (36, 64), (42, 42))
  pool = family in ('conv_pool_fwd', 'pool_conv_bwd')
  if pool or H * 2 > 18 + 9:
    return (H, W) in ((18, 24), (18, 32), (21, 21))
  return (H, W) in ((9, 12), (9, 16), (11, 11))
