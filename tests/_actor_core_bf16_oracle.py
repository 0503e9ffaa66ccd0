"""Float64 one-step oracle of the bf16 fused actor core step (test helper;
csrc/kernels/actor_core_bf16.hip).  The constants and the cell's Lipschitz
propagation are those of tests/_lstm_oracle.py (`forward`); only the gate
pre-activation differs: one fp32-accumulated product over [h_aug[:, :K] |
keep ? h_in : 0] with bf16-rounded operands, then the bias.

Pre-activation bound per element, u = 2^-24:
  (kpad + 256 + C_SUM) u sum|a||b|  +  gamma_2 (|prod| + |b| + [forget])
bf16 x bf16 products are exact in fp32; a column's kpad + 256 terms are added
in fp32 MFMA chains (_lstm_oracle's K u sum|a||b| model) of 4 K-parts whose 4
partial sums are then added in fp32: C_SUM = 4.  The bias add and the forget
gate's + 1 are two more roundings of a sum (gamma_2)."""

import torch

from tests import _lstm_oracle as L

C_SUM = 4


def step(x, h_in, c_in, done, w_x, w_h, bias, kpad, chain=True):
  """x [R, K] / h_in / c_in / w_x [K, 1024] / w_h [256, 1024] / bias [1024]:
  CPU tensors, the operands NOT yet rounded (this rounds x, h_in, w_x, w_h to
  bf16 as the kernel does); done [R] bool.  chain=False: the sums are exact
  in fp32 (the exact case), no chain term.
  -> {'c2': (ref, bound), 'h2': (ref, bound)} in float64."""
  U, H = L.U, 256
  keep = (~done).double().unsqueeze(-1)
  hk = torch.where(done.unsqueeze(-1), torch.zeros_like(h_in), h_in)
  a = torch.cat([L.bf16_rne(x), L.bf16_rne(hk)], 1)
  w = torch.cat([L.bf16_rne(w_x), L.bf16_rne(w_h)], 0)
  prod = a @ w
  mag = a.abs() @ w.abs()
  b = bias.double()
  forget = torch.zeros(4 * H, dtype=torch.float64)
  forget[2 * H:3 * H] = 1.0
  pre = prod + b + forget
  e_pre = L.gamma(2) * (prod.abs() + b.abs() + forget)
  if chain:
    e_pre = e_pre + (kpad + H + C_SUM) * U * mag
  # from here on: _lstm_oracle.forward's propagation
  pi, pg, pf, po = pre.split(H, -1)
  ei, eg, ef, eo = e_pre.split(H, -1)
  act = L.ACT_ULPS * U
  i, g, f, o = torch.sigmoid(pi), torch.tanh(pg), torch.sigmoid(pf), torch.sigmoid(po)
  ei, eg, ef, eo = ei / 4 + act, eg + act, ef / 4 + act, eo / 4 + act
  kcp = keep * torch.where(done.unsqueeze(-1), torch.zeros_like(c_in), c_in).double()
  c = f * kcp + i * g
  e_c = (ef * kcp.abs() + ei * g.abs() + eg * i.abs() + ei * eg +
         L.gamma(3) * ((f * kcp).abs() + (i * g).abs()))
  tc = torch.tanh(c)
  e_tc = e_c + act
  h = o * tc
  e_h = eo * tc.abs() + o * e_tc + eo * e_tc + U * h.abs()
  return {'c2': (c, e_c), 'h2': (h, e_h)}
