"""Float64 one-step oracle tests of the instruction encoder's two kernels
(csrc/kernels/lang_lstm.hip), called through the raw bindings
lang_lstm_fwd / lang_lstm_bwd.

Every step of every case is compared with tests/_lang_oracle.py: float64 fed
the kernel's own saved tensors (xh, cs forward; acts, cs, dgates[t+1]
backward; dx for the embedding scatter), with the bounds derived in that
module's docstring and no element left out; the bitwise properties listed
there are compared with torch.equal or as bits.  Inputs are drawn on the CPU
from fixed seeds and copied to the device, so oracle and kernel read the same
bits.  Each case prints max |pre| and the largest error / bound per tensor
(pytest -s).

The table (_lang_oracle.CASES, also walked on the CPU by
tests/test_lang_oracle.py with an fp32 emulation and planted faults):

  N = 1, 15, 16, 17, 33, 48   one partly filled 16-row workgroup, a full one,
                              one live row in a second, three workgroups
  L = 1, 2, 5, 16             first step == last step, no previous cell state
  lengths                     all 0; all L; 0 .. L with both ends; past L and
                              negative (clamped); a whole 16-row workgroup of
                              empty instructions next to a full one, both orders
  ids                         0, V-1; V, -1, 2^40 and their like (read row 0);
                              every word the same id; V = 1
"""

import pytest
import torch

from tests import _lang_oracle as O

pytestmark = pytest.mark.gpu

_WORST = {}


def _C():
  from scalable_agent_amd import ops
  ops.load()
  return ops.ext()


def _run(dev, inp):
  """Forward, backward without egrad, backward with ids and a prefilled
  egrad; everything back on the CPU in the layout verify() takes."""
  C = _C()
  d = {k: v.to(dev) for k, v in inp.items()}
  out, acts, cs, xh = C.lang_lstm_fwd(d['ids'], d['lengths'], d['embed'], d['kernel'],
                                      d['bias'])
  dg, dx = C.lang_lstm_bwd(d['lengths'], d['kernel'], d['dout'], acts, cs)
  egrad = d['prefill'].clone()
  dg2, dx2 = C.lang_lstm_bwd(d['lengths'], d['kernel'], d['dout'], acts, cs,
                             ids=d['ids'], egrad=egrad)
  torch.cuda.synchronize()
  got = {'out': out, 'acts': acts, 'cs': cs, 'xh': xh, 'dg': dg, 'dx': dx,
         'dg_fused': dg2, 'dx_fused': dx2, 'egrad': egrad}
  return {k: v.cpu() for k, v in got.items()}


@pytest.fixture(scope='module', autouse=True)
def _report():
  yield
  for name in sorted(_WORST):
    print('\nlargest err/bound  %-7s %.4f' % (name, _WORST[name]), end='')
  print()


def test_activation_constant(cuda):
  """The one term of the bounds that is measured, not derived: the gate
  outputs of an L = 1 case stay within the constant borrowed from the LSTM
  oracle (2 x its recorded measurement); the values by gate are printed and
  recorded in _lang_oracle."""
  inp = O.draw(O.ACT_CASE)
  got = _run(cuda, inp)
  ref = O.forward(inp, got['xh'], got['cs'])
  ulps = (got['acts'].double() - ref['acts'][0]).abs() / O.U
  per_gate = [float(x.max()) for x in ulps.split(O.H, -1)]
  print('  activation error in 2^-24 units: i %.3f c~ %.3f f %.3f o %.3f' % tuple(per_gate))
  assert max(per_gate) <= O.ACT_ULPS
  assert O.verify(inp, got)[0] == []


@pytest.mark.parametrize('case', O.CASES, ids=lambda c: c['name'])
def test_case(cuda, case):
  inp = O.draw(case)
  got = _run(cuda, inp)
  N, L = case['N'], case['L']
  assert got['out'].shape == (N, O.H) and got['acts'].shape == (L, N, O.G)
  assert got['cs'].shape == (L, N, O.H) and got['xh'].shape == (L, N, O.XH)
  assert got['dg'].shape == (L, N, O.G) and got['dx'].shape == (L, N, O.E)
  fails, stats, pre_max = O.verify(inp, got)
  print('  %s  max|pre| %.2f  ' % (case['name'], pre_max) +
        '  '.join('%s %.3f' % kv for kv in sorted(stats.items())))
  for name, ratio in stats.items():
    _WORST[name] = max(_WORST.get(name, 0.0), ratio)
  assert fails == []


def test_through_the_op_deterministic_and_atomic(cuda):
  """ops.language_lstm end to end: its output is the raw forward's bits, and
  embed.grad of the atomic path and of the deterministic one-hot product
  both hold the scatter bound (empty prefill) against the float64 sum of the
  kernel's dx, and agree with each other within it."""
  from scalable_agent_amd import ops
  case = next(c for c in O.CASES if c['name'] == 'N33-L5-V1000-rand-rand')
  inp = O.draw(case)
  direct = _run(cuda, inp)
  ref, bound, count = O.scatter(inp, direct['dx'], prefill=torch.zeros_like(inp['prefill']))
  grads = []
  for det in (False, True):
    p = [inp[k].to(cuda).requires_grad_() for k in ('embed', 'kernel', 'bias')]
    out = ops.language_lstm(inp['ids'].to(cuda), inp['lengths'].to(cuda), *p)
    assert O.same_bits(out.detach().cpu(), direct['out'])
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(det, warn_only=True)
    try:
      (out * inp['dout'].to(cuda)).sum().backward()
    finally:
      torch.use_deterministic_algorithms(prev)
    g = p[0].grad.cpu()
    err = (g.double() - ref).abs()
    print('  det %d  embed.grad max err / bound %.3f' %
          (det, float((err[count > 0] / bound[count > 0]).max())))
    assert bool((err <= bound).all())
    assert torch.equal(g[count == 0], torch.zeros(int((count == 0).sum()), O.E))
    grads.append(g)
  diff = (grads[0].double() - grads[1].double()).abs()
  assert bool((diff <= bound).all())


def test_backward_refuses_wrong_shapes(cuda):
  C = _C()
  inp = O.draw(O.CASES[7])
  d = {k: v.to(cuda) for k, v in inp.items()}
  out, acts, cs, xh = C.lang_lstm_fwd(d['ids'], d['lengths'], d['embed'], d['kernel'],
                                      d['bias'])
  L, N = acts.shape[0], acts.shape[1]
  bwd = lambda k, a, c: C.lang_lstm_bwd(d['lengths'], k, d['dout'], a, c)
  bwd(d['kernel'], acts, cs)
  for k in (d['kernel'][:83].contiguous(), d['kernel'][:, :255].contiguous(),
            d['kernel'].reshape(-1), d['kernel'].t().contiguous()):
    with pytest.raises(RuntimeError, match=r'kernel \[84, 256\]'):
      bwd(k, acts, cs)
  for a in (acts[..., :255].contiguous(), acts.reshape(L * N, O.G),
            acts.reshape(L, N * 4, O.H)):
    with pytest.raises(RuntimeError, match=r'acts \[L, N, 256\]'):
      bwd(d['kernel'], a, cs)
  for c in (cs[..., :63].contiguous(), cs[:L - 1].contiguous(), cs[:, :N - 1].contiguous(),
            cs.reshape(L * N, O.H), torch.cat([cs, cs], 0)):
    with pytest.raises(RuntimeError, match=r'cs \[L, N, 64\]'):
      bwd(d['kernel'], acts, c)
  torch.cuda.synchronize()


@pytest.mark.parametrize('N,L', [(0, 5), (7, 0), (0, 0)])
def test_empty_launches(cuda, N, L):
  """N = 0 or L = 0: nothing is launched, out comes back zero, the saved
  tensors and the gradients are empty, and a prefilled egrad keeps its bits."""
  C = _C()
  inp = O.draw(O.CASES[0])
  d = {k: inp[k].to(cuda) for k in ('embed', 'kernel', 'bias', 'prefill')}
  ids = torch.zeros(N, L, dtype=torch.int64, device=cuda)
  lengths = torch.full((N,), 3, dtype=torch.int64, device=cuda)
  out, acts, cs, xh = C.lang_lstm_fwd(ids, lengths, d['embed'], d['kernel'], d['bias'])
  assert out.shape == (N, O.H) and torch.equal(out, torch.zeros(N, O.H, device=cuda))
  assert acts.shape == (L, N, O.G) and cs.shape == (L, N, O.H) and xh.shape == (L, N, O.XH)
  dout = torch.ones(N, O.H, device=cuda)
  dg, dx = C.lang_lstm_bwd(lengths, d['kernel'], dout, acts, cs)
  assert dg.shape == (L, N, O.G) and dx.shape == (L, N, O.E)
  egrad = d['prefill'].clone()
  dg, dx = C.lang_lstm_bwd(lengths, d['kernel'], dout, acts, cs, ids=ids, egrad=egrad)
  torch.cuda.synchronize()
  assert dg.shape == (L, N, O.G) and dx.numel() == 0
  assert O.same_bits(egrad.cpu(), inp['prefill'])
