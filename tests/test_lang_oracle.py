"""CPU checks of the instruction encoder's float64 oracle itself
(tests/_lang_oracle.py): it reproduces a free-running float64 encoder and its
autograd, a correct fp32 implementation passes every bound at every case of
the GPU table with nothing excluded, and each planted fault fails exactly the
cases that exercise it."""

import pytest
import torch

from tests import _lang_oracle as O

_CACHE = {}


def _inputs(case):
  if case['name'] not in _CACHE:
    inp = O.draw(case)
    _CACHE[case['name']] = (inp, O.emulate(inp))
  return _CACHE[case['name']]


def test_case_table_covers_the_edges():
  """Every N meets every length pattern ('block' from the first N with two
  workgroups on), every L meets every pattern, every id pattern and V = 1
  appear, and the drawn inputs hold what the pattern names."""
  seen = {(c['N'], c['lens']) for c in O.CASES}
  for n in O.NS:
    for pat in O.LEN_PATTERNS:
      assert (n, pat) in seen or (pat == 'block' and n < 17), (n, pat)
  seen = {(c['L'], c['lens']) for c in O.CASES}
  assert seen >= {(l, p) for l in O.LS for p in O.LEN_PATTERNS}
  assert {c['ids'] for c in O.CASES} == set(O.ID_PATTERNS)
  assert any(c['V'] == 1 for c in O.CASES)
  assert len({c['name'] for c in O.CASES}) == len(O.CASES)
  assert O.LANG_ACT_MEASURED <= O.ACT_ULPS
  for c in O.CASES:
    inp = O.draw(c)
    lens, ids, N, L, V = inp['lengths'], inp['ids'], c['N'], c['L'], c['V']
    if c['lens'] == 'rand' and N >= 2:
      assert int(lens.min()) == 0 and int(lens.max()) == L
    if c['lens'] == 'beyond':
      assert int(lens.max()) > L and (N < 3 or int(lens.min()) < 0)
    if c['lens'] == 'block':
      a, b = lens[:16], lens[16:32]
      empty, full = (b, a) if c['flip'] else (a, b)
      assert bool((empty == 0).all()) and bool((full == L).all())
    if c['ids'] == 'edge':
      got = set(ids.view(-1).tolist())
      assert V in got
      if N * L >= 7:
        assert {V, -1, 2 ** 40, 0, V - 1} <= got
    if c['ids'] == 'same':
      assert len(set(ids.view(-1).tolist())) == 1
    assert bool((inp['prefill'] != 0).all())


@pytest.mark.parametrize('case', O.CASES[2::5] + O.CASES[-4:], ids=lambda c: c['name'])
def test_oracle_reproduces_float64_encoder_and_autograd(case):
  """Fed the float64 free-running encoder's own tensors, every one-step
  reference reproduces them to 1e-12, and the backward references are that
  encoder's float64 autograd, the embedding gradient included."""
  inp = O.draw(case)
  r = O.ref_encoder(inp)
  w = inp['dout'].double()
  (r['out'] * w).sum().backward()
  close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
  xh, cs = torch.stack(r['xh']).detach(), torch.stack(r['cs']).detach()
  acts = torch.stack(r['acts']).detach()
  L, N = xh.shape[0], xh.shape[1]
  zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
  dg = torch.stack([zero(p) for p in r['pre']])
  dx = torch.stack([zero(x) for x in r['x']])
  fwd = O.forward(inp, xh, cs)
  close(fwd['acts'][0], acts)
  close(fwd['cs'][0], cs)
  if L > 1:
    close(fwd['hs'][0][:-1], xh[1:, :, O.E:])
  inv = O.invariants(inp, xh)
  lens = inv['lens']
  assert torch.equal(lens, inp['lengths'].clamp(0, L))
  assert torch.equal(inv['x'], xh[..., :O.E].float())
  rows = torch.nonzero(lens > 0).view(-1)
  close(fwd['hs'][0][lens[rows] - 1, rows], r['out'].detach()[rows])
  assert torch.equal(r['out'].detach()[inv['zero_rows']],
                     torch.zeros(inv['zero_rows'].numel(), O.H, dtype=torch.float64))
  close(inv['out_vals'], r['out'].detach()[inv['out_rows']])
  bwd = O.backward(inp, acts, cs, dg)
  close(bwd['dg'][0], dg)
  close(bwd['dx'][0], dx)
  past = ~bwd['valid'].expand(L, N, O.G)
  assert float(dg[past].abs().sum()) == 0.0
  ref, bound, count = O.scatter(inp, dx, prefill=torch.zeros_like(inp['prefill']))
  close(ref, zero(r['embed']))
  assert int(count.sum()) == int(lens.sum())
  # the parameter gradients are the GEMMs the op forms from xh and dgates
  close(torch.einsum('lnk,lng->kg', xh, dg), zero(r['kernel']))
  close(dg.sum((0, 1)), zero(r['bias']))


@pytest.mark.parametrize('case', O.CASES + [O.ACT_CASE], ids=lambda c: c['name'])
def test_fp32_emulation_passes_every_bound(case):
  """The bounds are not too tight for a correct fp32 implementation: the
  kernel's structure in float32 torch passes every check, no element left
  out, and every bound is finite and positive where the check is not
  bitwise."""
  inp, got = _inputs(case)
  fails, stats, pre_max = O.verify(inp, got)
  print('  %s  max|pre| %.2f  ' % (case['name'], pre_max) +
        '  '.join('%s %.3f' % kv for kv in sorted(stats.items())))
  assert fails == []
  assert pre_max < 8.0
  for name, b in O.bounds_of(inp, got).items():
    assert bool(torch.isfinite(b).all()) and bool((b > 0).all()), name
  for name, ratio in stats.items():
    assert ratio <= 1.0, name


@pytest.mark.parametrize('fault', O.FAULTS)
def test_planted_fault_fails(fault):
  """Each fault fails every case of the table that exercises it (fault_hits
  names them) and no other; at least one case names it."""
  named, caught = [], []
  for case in O.CASES:
    inp, _ = _inputs(case)
    fails, _, _ = O.verify(inp, O.emulate(inp, fault))
    if O.fault_hits(fault, case, inp):
      named.append(case['name'])
    if fails:
      caught.append(case['name'])
  print('  %s fails %d of %d cases: %s' % (fault, len(caught), len(O.CASES), ', '.join(caught)))
  assert named, 'no case of the table exercises ' + fault
  assert caught == named
