"""CPU checks of the float64 LSTM oracle itself (tests/_lstm_oracle.py)."""

import pytest
import torch

from tests import _lstm_oracle as O


def test_bf16_rne_matches_torch_bfloat16():
  gen = torch.Generator().manual_seed(0)
  x = torch.randn(1 << 16, generator=gen) * torch.exp2(
      torch.randint(-20, 20, (1 << 16,), generator=gen).float())
  # exact midpoints (low half 0x8000) on even and odd upper halves, the
  # neighbours of a midpoint, and a carry into the next binade (0x3f7f8000)
  bits = x[:4096].view(torch.int32) & ~0xffff
  ties = torch.cat([bits | 0x8000, bits | 0x7fff, bits | 0x8001,
                    torch.tensor([0x3f7f8000, 0x3f7f7fff, 0x3f808000, 0x3f818000],
                                 dtype=torch.int32)]).view(torch.float32)
  x = torch.cat([x, ties, torch.zeros(1)])
  assert torch.equal(O.bf16_rne(x), x.to(torch.bfloat16).double())
  # a float64 just above a midpoint rounds up, where rounding through fp32
  # first (double rounding) would land on the tie and go to even
  mid = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)
  assert float(O.bf16_rne(mid)) == 1.0
  assert float(O.bf16_rne(mid + 2.0 ** -40)) == 1.0 + 2.0 ** -7


def test_near_tie_share_on_test_inputs():
  """dG ~ 0.1 N(0,1) U(0,1), W_h ~ 0.05 N(0,1): the rigorous delta masks a
  minority of the partials and at most MAX_TIE_SHARE of the elements."""
  gen = torch.Generator().manual_seed(1)
  dg = 0.1 * torch.randn(5, 32, 1024, generator=gen) * torch.rand(5, 32, 1024, generator=gen)
  w_h = 0.05 * torch.randn(256, 1024, generator=gen)
  rec, e_sum, allow, mask = O.recurrent_gang(dg, w_h)
  share = float(mask.double().mean())
  print('near-tie element share %.3f' % share)
  assert 0.0 < share <= O.MAX_TIE_SHARE
  assert torch.equal(allow > 0, mask)
  # against the exact product: off the mask only the operand rounding shows
  exact = O.bf16_rne(dg) @ O.bf16_rne(w_h).t()
  assert float((rec - exact).abs().max()) <= 8 * 2.0 ** -9 * float(exact.abs().max())


@pytest.mark.parametrize('T,B,H', [(5, 7, 64), (3, 4, 256)])
def test_identity_oracle_matches_float64_autograd(T, B, H):
  """With R = identity and float64 inputs, the teacher-forced oracle fed the
  free-running float64 reference's own outputs reproduces that reference,
  forward and backward (autograd), to 1e-12."""
  inp = {k: (v.double() if v.is_floating_point() else v)
         for k, v in O.draw(7, T, B, H).items()}
  inp['done'][0, 0] = 1
  inp['done'][T - 1, 1] = 1
  xw = inp['xw'].clone().requires_grad_()
  c0 = inp['c0'].clone().requires_grad_()
  hs, cs, acts = O.ref_lstm(xw, inp['done'], c0, inp['h0'], inp['w_h'])
  ((hs * inp['dh']).sum() + (cs[-1] * inp['dcl']).sum()).backward()
  hs, cs, acts = hs.detach(), cs.detach(), acts.detach()
  fwd = O.forward(inp['xw'], inp['done'], inp['c0'], inp['h0'], inp['w_h'], hs, cs, 0)
  for name, got in (('acts', acts), ('cs', cs), ('hs', hs)):
    torch.testing.assert_close(fwd[name][0], got, rtol=1e-12, atol=1e-12)
    assert float(fwd[name][1].min()) > 0
  bwd = O.backward(inp['dh'], inp['done'], inp['w_h'], acts, cs, inp['c0'],
                   inp['dcl'], xw.grad, 0)
  torch.testing.assert_close(bwd['dg'][0], xw.grad, rtol=1e-12, atol=1e-12)
  torch.testing.assert_close(bwd['dc0'][0], c0.grad, rtol=1e-12, atol=1e-12)
  # two chained chunks with the boundary's recurrent term folded into dh_out
  if T >= 4:
    a = T // 2
    keep = (inp['done'][a] == 0).double().unsqueeze(-1)
    dh = inp['dh'].clone()
    dh[a - 1] += keep * (xw.grad[a] @ inp['w_h'].t())
    cut = O.backward(dh, inp['done'], inp['w_h'], acts, cs, inp['c0'],
                     inp['dcl'], xw.grad, 0, cuts=(a - 1,))
    torch.testing.assert_close(cut['dg'][0], xw.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(cut['dc0'][0], c0.grad, rtol=1e-12, atol=1e-12)
