"""CPU checks of the float64 GEMM oracle itself (tests/_gemm_oracle.py)."""

import pytest
import torch

from tests import _gemm_oracle as O


def _cases():
  return [
      O.spec('f32', 37, 28, 260, False, False, bias=True, relu=True, naug=12),
      O.spec('f32', 66, 29, 68, True, True, mask=True, accumulate=True, colsum=True),
      O.spec('bf16', 45, 24, 136, True, False, accumulate=True, colsum=True),
      O.spec('bf16', 40, 9, 72, False, True, bias=True, mask=True, c_bf16=True),
  ]


@pytest.mark.parametrize('s', _cases(), ids=O.name)
@pytest.mark.parametrize('kind', ['int', 'randn'])
def test_reference_matches_matmul_and_elementwise_epilogue(s, kind):
  """The product against torch.matmul in float64 on the un-embedded
  operands, the epilogue against a plain per-element loop."""
  c = O.make(s, kind)
  ref = O.reference(c)
  A = O.view(c['A'], c['A_at']).double()
  B = O.view(c['B'], c['B_at']).double()
  acc = torch.matmul(A.t() if s['ta'] else A, B.t() if s['tb'] else B)
  assert acc.shape == (s['M'], s['N']) and not torch.isnan(acc).any()
  C0 = O.view(c['C'], c['C_at']).double()
  want = torch.empty_like(acc)
  for m in range(s['M']):
    for n in range(s['N']):
      v = float(acc[m, n])
      if s['bias']:
        v += float(O.view1(c['bias'], c['bias_at'])[n])
      if s['mask'] and not float(O.view(c['mask'], c['mask_at'])[m, n]) > 0:
        v = 0.0
      if s['relu']:
        v = max(v, 0.0)
      if s['accumulate']:
        v += float(C0[m, n])
      want[m, n] = v
  assert torch.equal(ref['C'], want)
  if s['colsum']:
    opB = B.t() if s['tb'] else B
    cs0 = O.view1(c['colsum'], c['colsum_at']).double()
    assert torch.allclose(ref['colsum'], cs0 + torch.ones(1, s['K'], dtype=torch.float64)
                          .matmul(opB)[0], rtol=0, atol=1e-9)
  if s['naug']:
    r = O.view1(c['reward'], c['reward_at'])
    a = O.view1(c['action'], c['action_at'])
    assert ref['aug'].shape == (s['M'], s['naug'])
    for m in range(s['M']):
      row = [min(max(float(r[m]), -1.0), 1.0)] + [0.0] * (s['naug'] - 1)
      row[1 + int(a[m])] = 1.0
      assert ref['aug'][m].tolist() == row


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_embedding_is_poisoned_and_aligned(dtype):
  q = O.quad(dtype)
  s = O.spec(dtype, 37, 29, 8 * q + q, True, False, mask=True, bias=True, colsum=True,
             accumulate=True)
  c = O.make(s, 'int')
  for k in ('A', 'B', 'mask'):
    store, (off, cols) = c[k], c[k + '_at']
    assert store.stride(0) % q == 0 and off % q == 0 and off >= q
    assert store.shape[1] >= off + cols + q  # poison on both sides of a row
    inside = torch.zeros_like(store, dtype=torch.bool)
    O.view(inside, (off, cols))[:] = True
    assert torch.isnan(store[~inside]).all() and not torch.isnan(store[inside]).any()
    assert O.view(store, (off, cols)).shape[0] == store.shape[0] - 2
  inside = torch.zeros_like(c['C'], dtype=torch.bool)
  O.view(inside, c['C_at'])[:] = True
  assert (c['C'][~inside] == O.SENTINEL).all() and (c['C'][inside].abs() <= 4).all()
  assert torch.isnan(c['bias'][:8]).all() and torch.isnan(c['bias'][-8:]).all()
  assert (c['colsum'][:8] == O.SENTINEL).all() and (c['colsum'][-8:] == O.SENTINEL).all()
  assert float(torch.tensor(O.SENTINEL).to(O.BF)) == O.SENTINEL
  # the mask draws every special value, signed zeros included
  mv = O.view(c['mask'], c['mask_at']).float()
  assert set(mv.unique().tolist()) == set(O.MASK_VALUES)
  assert bool((torch.signbit(mv) & (mv == 0)).any()) and bool((~torch.signbit(mv) & (mv == 0)).any())


def test_integer_operands():
  gen = torch.Generator().manual_seed(0)
  v = O.int_operand(gen, 400, 400)
  assert set(v.unique().tolist()) == {float(i) for i in range(-4, 5)}
  zero = float((v == 0).double().mean())
  assert 0.23 <= zero <= 0.27
  assert torch.equal(v.to(O.BF).float(), v)  # exact as bf16 operands


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_exactness_premise_at_the_largest_k(dtype):
  """At K_MAX every |result| - and so every partial sum of any order, each
  bounded by 16 K + the epilogue's small integers - is below 2^24: fp32 holds
  it exactly, and an fp32 product summed in another order (and in 16 K
  slabs, as the split kernels do) equals the float64 reference bit for bit."""
  assert 16 * O.K_MAX + 4 + 4 < 2 ** 24
  s = O.spec(dtype, 70, 40, O.K_MAX, True, False, bias=True, accumulate=True, colsum=True)
  c = O.make(s, 'int')
  ref = O.reference(c)
  assert float(ref['C'].abs().max()) < 2 ** 24
  assert float(ref['colsum'].abs().max()) < 2 ** 24
  A = O.view(c['A'], c['A_at']).float().t()
  B = O.view(c['B'], c['B_at']).float()
  assert float((A.abs() @ B.abs()).max()) < 2 ** 24  # the worst partial sum of any order
  slabs = sum((A[:, k:k + 320] @ B[k:k + 320]) for k in reversed(range(0, O.K_MAX, 320)))
  v = slabs + O.view1(c['bias'], c['bias_at']) + O.view(c['C'], c['C_at'])
  assert torch.equal(v.double(), ref['C'])


def _emulate(c):
  """A correct 'kernel' on the CPU in the output type, for the checker."""
  ref = O.reference(c)
  s = c['spec']
  out = {'C': c['C'].clone()}
  cv = O.view(out['C'], c['C_at'])
  cv[:, :s['N']] = ref['C'].float().to(cv.dtype)
  if s['naug']:
    cv[:, s['N']:] = ref['aug'].float().to(cv.dtype)
  if s['colsum']:
    out['colsum'] = c['colsum'].clone()
    O.view1(out['colsum'], c['colsum_at'])[:] = ref['colsum'].float()
  return out


@pytest.mark.parametrize('s', _cases(), ids=O.name)
def test_checker_accepts_exact_and_rejects_small_faults(s):
  c = O.make(s, 'int')
  O.check(c, _emulate(c))
  one = 1.0 if not s['c_bf16'] else 4.0  # at least a bf16 ulp at these magnitudes
  # one dropped unit product in one element
  out = _emulate(c)
  O.view(out['C'], c['C_at'])[s['M'] - 1, s['N'] - 1] += one
  with pytest.raises(AssertionError, match='wrong elements'):
    O.check(c, out)
  # a store one column past N, one row past M
  for r, col in ((1, c['C_at'][0] + s['N'] + s['naug']), (s['M'] + 1, c['C_at'][0])):
    out = _emulate(c)
    if col < out['C'].shape[1]:
      out['C'][r, col] = 0.0
      with pytest.raises(AssertionError, match='outside'):
        O.check(c, out)
  # a NaN that came in from operand padding
  out = _emulate(c)
  O.view(out['C'], c['C_at'])[0, 0] = float('nan')
  with pytest.raises(AssertionError, match='NaN'):
    O.check(c, out)
  if s['colsum']:
    out = _emulate(c)
    O.view1(out['colsum'], c['colsum_at'])[s['N'] - 1] += 1.0
    with pytest.raises(AssertionError, match='colsum'):
      O.check(c, out)
  if s['naug']:
    out = _emulate(c)
    O.view(out['C'], c['C_at'])[3, s['N'] + s['naug'] - 1] = 1.0
    with pytest.raises(AssertionError, match='aug'):
      O.check(c, out)


def test_case_lists_name_every_path():
  """The shared case lists hold what the GPU file and its SA_GEMM_BL=0 child
  rely on: all four layouts, both kernels in-process, ids unique."""
  for dtype in ('f32', 'bf16'):
    pm, ones = O.path_matrix(dtype), O.ones_row(dtype)
    assert len(pm) == 24 and {(s['ta'], s['tb']) for s in pm} == set(O.LAYOUTS)
    assert {O.expect_bl(s) for s in pm} == {True, False}
    assert not any(O.expect_bl(s, child=True) for s in pm + ones)
    q = O.quad(dtype)
    both = [s for s in pm if s['M'] % q == 0 and s['N'] % q == 0 and s['K'] % q == 0]
    assert both and all(O.expect_bl(s) for s in both)
    names = [O.name(s) for s in pm + ones]
    assert len(set(names)) == len(names)
    assert any(s['empty_chunk'] for s in ones) and all(s['K'] <= O.K_MAX for s in pm + ones)
