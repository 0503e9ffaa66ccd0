"""Float64 one-step (teacher-forced) oracle of the LSTM recurrence (test helper).

Kernels under test: lstm.hip (mode 0, per-step fp32), lstm_persistent.hip
(mode 1, whole-unroll fp32) and lstm_gang.hip (mode 2, whole-unroll with a
bf16 recurrent product).  A free-running comparison accumulates the bf16
error of T steps and can never be tight, so every step is checked on its own:
step t of the oracle is fed the KERNEL's previous outputs (hs[t-1], cs[t-1]
forward; dG[t+1] backward) and computes that one step in float64.

R is the identity for modes 0 and 1 and bf16 round-to-nearest-even for mode 2
(the gang rounds h_{t-1} / dG_{t+1} and W_h for the product, and every
backward partial for the exchange; everything else stays fp32).

Bounds are derived, with u = 2^-24:
  * a K-term fp32 MFMA chain: K u sum|a||b| per element, from the oracle's own
    operands (forward K = H; backward K = 4H, or 128 per partial in mode 2,
    whose 8 rounded partials are then added in fp32: 8 u sum|R(P_src)|);
  * n fp32 roundings of a product / sum: gamma_n = n u / (1 - n u);
  * sigmoid is 1/4-Lipschitz, tanh 1-Lipschitz; products propagate by the
    float64 magnitudes;
  * the backward carry chain runs in float64 from dc_last with the oracle's
    own dc_t; its error bound is the running sum
    e_carry[t] = e_dc[t] f_t keep_t + gamma_2 |carry[t]|,
    e_dc[t] = e_carry[t+1] + e_local[t] + u |dc_t|  (f keep <= 1);
  * one term cannot be derived: the intrinsic error of the __expf-based
    sigmoid and of tanhf.  It was measured on an MI355X as the largest
    |kernel - float64| / u over the gate outputs of the step-mode T = 1 case
    (test_activation_constant, H = 256, B = 32): ACT_MEASURED below.  The
    bounds allow ACT_ULPS = 2 x that, the maximum being over a finite sample.

Near-tie partials (mode 2 backward): R(P_src) in the kernel rounds an fp32-
accumulated partial.  Where the float64 partial lies within
delta = 128 u sum|a||b| of a bf16 rounding midpoint the kernel may round the
other way; such an element is allowed the bf16 ulps of its near-tie partials
on top of the tight bound, elements without one are held to the tight bound.
The share of (step, row, unit) elements with a near-tie partial is returned
and must stay <= MAX_TIE_SHARE.
"""

import torch

U = 2.0 ** -24
# |kernel - float64| / u by gate: i 1.609, g 3.085, f 1.826, o 1.494
ACT_MEASURED = 3.085
ACT_ULPS = 2.0 * ACT_MEASURED
MAX_TIE_SHARE = 0.60


def gamma(n):
  return n * U / (1.0 - n * U)


def bf16_rne(x):
  """x rounded to the nearest bf16 (ties to even), as float64.  x may be
  fp32 or float64 (rounded once, directly); normal range only."""
  x = x.double()
  m, e = torch.frexp(x)  # |m| in [0.5, 1): 8 significant bits = m * 256
  return torch.round(m * 256.0) * torch.exp2((e - 8).double())


def bf16_near_tie(x, delta):
  """(near, ulp): x within delta of a bf16 rounding midpoint; x's bf16 ulp."""
  m, e = torch.frexp(x.double())
  y = m.abs() * 256.0
  ulp = torch.exp2((e - 8).double())
  near = ((y - torch.floor(y) - 0.5).abs() * ulp <= delta) & (delta > 0)
  return near, ulp


def _ident(x):
  return x.double()


def _prev(first, seq):
  return torch.cat([first.reshape((1,) + seq.shape[1:]).to(seq.dtype), seq[:-1]])


def forward(xw, done, c0, h0, w_h, hs, cs, mode):
  """One-step forward oracle of every step t, fed hs[t-1] / cs[t-1] (h0, c0
  at t = 0).  Returns {name: (float64 reference, bound)} for acts, cs, hs and
  'hpm': the fp32 keep * h_prev the kernels must reproduce bitwise."""
  T, B, H4 = xw.shape
  H = H4 // 4
  rnd = bf16_rne if mode == 2 else _ident
  keep = (done.reshape(T, B) == 0).double().unsqueeze(-1)
  hp = _prev(h0, hs)
  cp = _prev(c0, cs).double()
  a, w = rnd(hp), rnd(w_h)
  prod = keep * (a @ w)
  mag = keep * (a.abs() @ w.abs())
  x = xw.double()
  bias = torch.zeros(H4, dtype=torch.float64)
  bias[2 * H:3 * H] = 1.0
  pre = x + prod + bias
  e_pre = H * U * mag + gamma(2) * (prod.abs() + x.abs() + bias)
  pi, pg, pf, po = pre.split(H, -1)
  ei, eg, ef, eo = e_pre.split(H, -1)
  act = ACT_ULPS * U
  i, g, f, o = torch.sigmoid(pi), torch.tanh(pg), torch.sigmoid(pf), torch.sigmoid(po)
  ei, eg, ef, eo = ei / 4 + act, eg + act, ef / 4 + act, eo / 4 + act
  kcp = keep * cp
  c = f * kcp + i * g
  e_c = (ef * kcp.abs() + ei * g.abs() + eg * i.abs() + ei * eg +
         gamma(3) * ((f * kcp).abs() + (i * g).abs()))
  tc = torch.tanh(c)
  e_tc = e_c + act
  h = o * tc
  e_h = eo * tc.abs() + o * e_tc + eo * e_tc + U * h.abs()
  return {
      'acts': (torch.cat([i, g, f, o], -1), torch.cat([ei, eg, ef, eo], -1)),
      'cs': (c, e_c),
      'hs': (h, e_h),
      'hpm': (keep.to(hp.dtype) * hp, None),
  }


def recurrent_gang(dg_next, w_h):
  """Mode 2 recurrent term sum_src R(P_src) of the steps whose dG_{t+1} is
  dg_next [N, B, 4H]: (rec, bound of the 8 fp32 additions, near-tie ulp
  allowance, near-tie mask), each [N, B, H]."""
  N, B, H4 = dg_next.shape
  H = H4 // 4
  S = H // 32  # source workgroups, 32 units x 4 gates = 128 columns each
  d = bf16_rne(dg_next).reshape(N, B, 4, S, 32)
  w = bf16_rne(w_h).reshape(H, 4, S, 32)
  p = torch.einsum('nbgsu,kgsu->nbsk', d, w)
  mag = torch.einsum('nbgsu,kgsu->nbsk', d.abs(), w.abs())
  near, ulp = bf16_near_tie(p, 128 * U * mag)
  rp = bf16_rne(p)
  allow = (near.double() * ulp).sum(2)
  e_sum = 8 * U * (rp.abs().sum(2) + allow)
  return rp.sum(2), e_sum, allow, near.any(2)


def backward(dh_out, done, w_h, acts, cs, c0, dc_last, dg, mode, cuts=()):
  """One-step backward oracle of every step t: the recurrent term comes from
  the kernel's own dG[t+1] (`dg`), the carry chain runs in float64 from
  dc_last.  acts / cs / c0 are the saved tensors the kernel was given.
  cuts: steps t that receive no recurrent term (the last step of a time
  chunk, whose dh_out already holds it).  Returns {'dg': (ref, bound),
  'dc0': (ref, bound), 'tie_share': float}."""
  T, B, H4 = acts.shape
  H = H4 // 4
  kf = (done.reshape(T, B) == 0).double().unsqueeze(-1)
  knext = torch.cat([kf[1:], torch.ones(1, B, 1, dtype=torch.float64)])
  for t in cuts:
    knext[t] = 0.0
  i, g, f, o = acts.double().split(H, -1)
  cp = _prev(c0, cs).double()
  zero = torch.zeros(1, B, H, dtype=torch.float64)
  tie_share = 0.0
  if T == 1:
    rec = e_rec = zero
  elif mode == 2:
    r, e_sum, allow, mask = recurrent_gang(dg[1:], w_h)
    rec = torch.cat([r, zero])
    e_rec = torch.cat([e_sum + allow, zero])
    tie_share = float((mask & (knext[:-1] != 0)).double().mean())
  else:
    d, w = dg[1:].double(), w_h.double()
    rec = torch.cat([d @ w.t(), zero])
    e_rec = torch.cat([H4 * U * (d.abs() @ w.abs().t()), zero])
  dh = dh_out.double().reshape(T, B, H) + knext * rec
  e_dh = knext * e_rec + U * dh.abs()
  tc = torch.tanh(cs.double())
  e_tc = ACT_ULPS * U
  s = 1.0 - tc * tc
  loc = dh * o * s
  e_s = 2.0 * tc.abs() * e_tc + gamma(2)
  e_loc = e_dh * (o * s).abs() + (dh * o).abs() * e_s + gamma(2) * loc.abs()
  fk = f * kf
  dc, e_dc = torch.empty_like(loc), torch.empty_like(loc)
  carry = torch.zeros(B, H, dtype=torch.float64) if dc_last is None else dc_last.double()
  e_carry = torch.zeros(B, H, dtype=torch.float64)
  for t in range(T - 1, -1, -1):
    dc[t] = carry + loc[t]
    e_dc[t] = e_carry + e_loc[t] + U * dc[t].abs()
    carry = dc[t] * fk[t]
    e_carry = e_dc[t] * fk[t] + gamma(2) * carry.abs()
  gi = dc * g * i * (1.0 - i)
  gg = dc * i * (1.0 - g * g)
  gf = dc * kf * cp * f * (1.0 - f)
  go = dh * tc * o * (1.0 - o)
  e_gi = e_dc * (g * i * (1.0 - i)).abs() + gamma(4) * gi.abs()
  e_gg = (e_dc * (i * (1.0 - g * g)).abs() + gamma(2) * (dc * i).abs() +
          gamma(2) * gg.abs())
  e_gf = e_dc * (kf * cp * f * (1.0 - f)).abs() + gamma(5) * gf.abs()
  e_go = (e_dh * (tc * o * (1.0 - o)).abs() + (dh * o * (1.0 - o)).abs() * e_tc +
          gamma(4) * go.abs())
  return {
      'dg': (torch.cat([gi, gg, gf, go], -1), torch.cat([e_gi, e_gg, e_gf, e_go], -1)),
      'dc0': (carry, e_carry),
      'tie_share': tie_share,
  }


def ref_lstm(xw, done, c0, h0, w_h):
  """Free-running reference in the dtype of its inputs (autograd-friendly),
  the recurrence of tests/test_kernels_gpu.py::_ref_lstm on projected inputs.
  Returns (hs, cs, acts)."""
  hs, cs, acts = [], [], []
  c, h = c0, h0
  for t in range(xw.shape[0]):
    keep = (done[t] == 0).to(xw.dtype).unsqueeze(-1)
    c, h = c * keep, h * keep
    i, ci, f, o = (xw[t] + h @ w_h).chunk(4, -1)
    i, ci, f, o = torch.sigmoid(i), torch.tanh(ci), torch.sigmoid(f + 1.0), torch.sigmoid(o)
    c = ci * i + c * f
    h = torch.tanh(c) * o
    hs.append(h)
    cs.append(c)
    acts.append(torch.cat([i, ci, f, o], -1))
  return torch.stack(hs), torch.stack(cs), torch.stack(acts)


def draw(seed, T, B, H, done=None):
  """Test inputs on the CPU from a fixed seed (the scales of the existing
  LSTM tests); done: uint8 [T, B], default rand < 0.1."""
  gen = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=gen)
  inp = {
      'xw': rn(T, B, 4 * H),
      'c0': rn(B, H) * 0.5,
      'h0': rn(B, H) * 0.5,
      'w_h': rn(H, 4 * H) * 0.05,
      'dh': rn(T, B, H),
      'dcl': rn(B, H),
  }
  rd = torch.rand(T, B, generator=gen) < 0.1
  inp['done'] = (rd if done is None else done).to(torch.uint8)
  return inp
