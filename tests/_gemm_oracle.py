"""Float64 oracle of the MFMA GEMMs with their fused epilogues (test helper).

Kernels under test: csrc/kernels/gemm_f32.hip and gemm_bf16.hip, each a
branch-free buffer-load program ("bl") and a bounds-checked one, 1 - 16 K
splits with a reduction kernel that owns the epilogue, four (ta, tb) layouts.

Two ideas make a subtly wrong kernel visible at small shapes:

  * Integer operands.  Every entry of A and B is drawn from {-4 .. 4} (about
    a quarter zeros), so every product is an integer of magnitude <= 16 and,
    for K <= K_MAX = 4104, every partial sum in any order stays below
    16 * 4104 + small < 2^24.  fp32 represents all of them, so a correct
    kernel's result IS the float64 product, whatever the split count or the
    summation order: the comparison is torch.equal, and one dropped or
    doubled product anywhere shows.  Bias, the initial C of `accumulate` and
    the initial colsum are small integers too.  A bf16 C holds the exact fp32
    value rounded to nearest even, which is what torch's cast of the
    reference gives.
  * Poisoned storage.  A, B, C and mask are views [r, c] at a column offset
    inside a wider storage [r + 2, ld] (one row above, one below, columns on
    both sides; ld and the offset multiples of 4 floats / 8 bf16, which is
    what the bindings demand of row stride and base).  Outside the view the
    operands and the mask are NaN, so a load that lands in padding where it
    should not reaches the output; C's storage holds SENTINEL, so a store
    outside the written region is seen.  bias, colsum, rewards and actions
    are slices of poisoned vectors in the same way.

The reference is the epilogue exactly as kernels/gemm_f32.h states it:
  v = acc [+ bias[n]] [v if mask[m, n] > 0 else 0] [max(v, 0)] [+ C0[m, n]],
  colsum[n] = colsum0[n] + sum_k op(B)[k, n],
  C[m, N + j] = [clip(r[m], -1, 1), one_hot(a[m]), 0...][j]   (aug mode).

On randn operands at the same shapes the project's tolerances apply (max
error over max |reference|): TOL below, nothing new.
"""

import os

import torch

BF = torch.bfloat16
K_MAX = 4104
# exact in fp32 and bf16, far outside what the integer cases produce
SENTINEL = -24576.0
# (dtype, bf16 C) -> max |err| / max |ref| on randn data (test_gemm_f32_gpu.py,
# test_gemm_bf16_gpu.py)
TOL = {('f32', False): 2e-6, ('bf16', False): 3e-6, ('bf16', True): 8e-3}
MASK_VALUES = (0.0, -0.0, -2.0, -0.5, 0.5, 1.0, 3.0)
ACTIONS = 9


def quad(dtype):
  """Elements per 16 bytes: the alignment unit of rows, bases and bl shapes."""
  return 4 if dtype == 'f32' else 8


def spec(dtype, M, N, K, ta, tb, **kw):
  s = dict(dtype=dtype, M=M, N=N, K=K, ta=ta, tb=tb, bias=False, relu=False,
           mask=False, accumulate=False, colsum=False, naug=0, c_bf16=False,
           c_off=None, c_ld=None, splits=None, empty_chunk=False, tail=None,
           grid0=None)
  assert not set(kw) - set(s), kw
  s.update(kw)
  return s


def name(s):
  tags = [k for k in ('bias', 'relu', 'mask', 'accumulate', 'colsum', 'c_bf16') if s[k]]
  if s['naug']:
    tags.append('aug%d' % s['naug'])
  if s['c_ld']:
    tags.append('ldc%d' % s['c_ld'])
  return '%s-%dx%dx%d-%s%s%s' % (s['dtype'], s['M'], s['N'], s['K'],
                                 'T' if s['ta'] else 'N', 'T' if s['tb'] else 'N',
                                 ''.join('-' + t for t in tags))


def int_operand(gen, *shape):
  """Entries of {-4 .. 4}, about a quarter of them zero."""
  v = torch.randint(1, 5, shape, generator=gen).float()
  v = v * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
  return v * (torch.rand(shape, generator=gen) >= 0.25).float()


def embed(t, q, fill, off=None, ld=None):
  """t [r, c] inside a storage [r + 2, ld] of `fill`, at row 1, column off."""
  r, c = t.shape
  off = q if off is None else off
  ld = (off + c + q - 1) // q * q + q if ld is None else ld
  assert off % q == 0 and ld % q == 0 and off + c <= ld
  store = torch.full((r + 2, ld), fill, dtype=t.dtype)
  store[1:r + 1, off:off + c] = t
  return store, (off, c)


def view(store, where):
  off, c = where
  return store[1:store.shape[0] - 1, off:off + c]


def embed1(t, fill, pad=8):
  store = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype)
  store[pad:pad + t.numel()] = t
  return store, pad


def view1(store, pad):
  return store[pad:store.numel() - pad]


def make(s, kind, seed=0):
  """The CPU tensors of one case.  kind: 'int' (exact) or 'randn'."""
  assert s['K'] <= K_MAX
  gen = torch.Generator().manual_seed(1000 * seed + s['M'] + 3 * s['N'] + 7 * s['K'])
  q = quad(s['dtype'])
  odt = torch.float32 if s['dtype'] == 'f32' else BF
  M, N, K = s['M'], s['N'], s['K']
  if kind == 'int':
    draw = lambda *sh: int_operand(gen, *sh)
  else:
    draw = lambda *sh: torch.randn(*sh, generator=gen)
  nan = float('nan')
  c = dict(spec=s, kind=kind)
  c['A'], c['A_at'] = embed(draw(*((K, M) if s['ta'] else (M, K))).to(odt), q, nan)
  c['B'], c['B_at'] = embed(draw(*((N, K) if s['tb'] else (K, N))).to(odt), q, nan)
  cdt = BF if s['c_bf16'] else torch.float32
  cq = quad('bf16' if s['c_bf16'] else 'f32')
  if s['naug']:  # the bindings want the aug columns to fill C's row: [M, ldc]
    c0 = torch.full((M, N + s['naug']), SENTINEL)
    c['C'], c['C_at'] = embed(c0.to(cdt), cq, SENTINEL, off=0, ld=N + s['naug'])
  else:
    c0 = draw(M, N) if s['accumulate'] else torch.full((M, N), SENTINEL)
    c['C'], c['C_at'] = embed(c0.to(cdt), cq, SENTINEL, off=s['c_off'], ld=s['c_ld'])
  if s['bias']:
    c['bias'], c['bias_at'] = embed1(draw(N), nan)
  if s['mask']:
    pick = torch.randint(0, len(MASK_VALUES), (M, N), generator=gen)
    c['mask'], c['mask_at'] = embed(torch.tensor(MASK_VALUES)[pick].to(odt), q, nan)
  if s['colsum']:
    c['colsum'], c['colsum_at'] = embed1(draw(N), SENTINEL)
  if s['naug']:
    c['reward'], c['reward_at'] = embed1(torch.randn(M, generator=gen) * 3, nan)
    a = torch.randint(0, min(ACTIONS, s['naug'] - 1), (M,), generator=gen)
    c['action'], c['action_at'] = embed1(a, 2 ** 31 - 1)
  return c


def _op(t, tr):
  return t.t() if tr else t


def reference(c):
  """float64: {'C' [M, N], 'colsum' [N] or None, 'aug' [M, naug] or None}."""
  s = c['spec']
  A = _op(view(c['A'], c['A_at']).double(), s['ta'])
  B = _op(view(c['B'], c['B_at']).double(), s['tb'])
  v = A @ B
  if s['bias']:
    v = v + view1(c['bias'], c['bias_at']).double()
  if s['mask']:
    v = torch.where(view(c['mask'], c['mask_at']).double() > 0, v, torch.zeros_like(v))
  if s['relu']:
    v = v.clamp(min=0)
  if s['accumulate']:
    v = v + view(c['C'], c['C_at'])[:, :s['N']].double()
  out = dict(C=v, colsum=None, aug=None)
  if s['colsum']:
    out['colsum'] = view1(c['colsum'], c['colsum_at']).double() + B.sum(0)
  if s['naug']:
    aug = torch.zeros(s['M'], s['naug'], dtype=torch.float64)
    aug[:, 0] = view1(c['reward'], c['reward_at']).double().clamp(-1, 1)
    aug[torch.arange(s['M']), 1 + view1(c['action'], c['action_at'])] = 1.0
    out['aug'] = aug
  return out


def expect_bl(s, child=False):
  """The launcher's rule as the issue states it (operands here are far below
  the 4 GB offset limit): whole quads along M when ta and along N when !tb."""
  q = quad(s['dtype'])
  return (not child and (not s['ta'] or s['M'] % q == 0) and
          (s['tb'] or s['N'] % q == 0))


def check_path(C, c, child=False):
  """Asserts from the launch-info hook that the case takes the path it is
  there for; returns the hook's record."""
  s = c['spec']
  hook = C.gemm_f32_info if s['dtype'] == 'f32' else C.gemm_bf16_info
  info = hook(s['M'], s['N'], s['K'], c['A'].stride(0), c['B'].stride(0), s['ta'], s['tb'],
              s['colsum'])
  what = '%s: %r' % (name(s), info)
  assert info['bl'] == expect_bl(s, child), what
  bk = 32 if s['dtype'] == 'f32' else 64
  assert info['kchunk'] % bk == 0 and info['splits'] * info['kchunk'] >= s['K'], what
  Mr = s['M'] + int(s['colsum'])
  assert info['grid'] == ((Mr + 63) // 64, (s['N'] + 63) // 64, info['splits']), what
  if s['dtype'] == 'f32':
    assert info['rm'] == 1, what
  if s['splits'] is not None:
    assert info['splits'] == s['splits'], 'split heuristic changed: ' + what
  if s['empty_chunk']:
    assert (info['splits'] - 1) * info['kchunk'] >= s['K'], \
        'the split heuristic no longer yields an empty K chunk here: ' + what
  if s['tail'] is not None:
    assert s['K'] - (info['splits'] - 1) * info['kchunk'] == s['tail'], \
        'the last K chunk is no longer %d long: %s' % (s['tail'], what)
  if s['grid0'] is not None:
    assert info['grid'][0] == s['grid0'], what
  return info


def launch(C, dev, c):
  """Runs the kernel on device copies of the case's storages; returns the
  storages it may have written, on the CPU: {'C', 'colsum'}."""
  s = c['spec']
  d = {k: c[k].to(dev) for k in ('A', 'B', 'C', 'bias', 'mask', 'colsum', 'reward', 'action')
       if k in c}
  kw = dict(relu=s['relu'], accumulate=s['accumulate'])
  if s['bias']:
    kw['bias'] = view1(d['bias'], c['bias_at'])
  if s['mask']:
    kw['mask'] = view(d['mask'], c['mask_at'])
  if s['colsum']:
    kw['colsum'] = view1(d['colsum'], c['colsum_at'])
  if s['naug']:
    kw['aug_reward'] = view1(d['reward'], c['reward_at'])
    kw['aug_action'] = view1(d['action'], c['action_at'])
  fn = C.gemm_f32 if s['dtype'] == 'f32' else C.gemm_bf16
  fn(view(d['A'], c['A_at']), view(d['B'], c['B_at']), s['ta'], s['tb'],
     view(d['C'], c['C_at']), **kw)
  return {k: d[k].cpu() for k in ('C', 'colsum') if k in d}


def rel(a, ref):
  return (a.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def check(c, out, ref=None):
  """The poison checks and the comparison with the float64 reference: exact
  for kind 'int', the project's tolerance for 'randn'.  Prints each figure."""
  s = c['spec']
  ref = reference(c) if ref is None else ref
  N, what = s['N'], name(s) + ' ' + c['kind']
  cdt = c['C'].dtype
  tol = TOL[(s['dtype'], s['c_bf16'])]
  got = out['C']
  assert not torch.isnan(got).any(), what + ': NaN in C'
  # everything outside the written region is the untouched storage
  keep = torch.ones_like(c['C'], dtype=torch.bool)
  view(keep, c['C_at'])[:, :N + s['naug']] = False
  assert torch.equal(got[keep], c['C'][keep]), what + ': store outside C[:, :N]'
  gv = view(got, c['C_at'])
  if s['naug']:
    assert torch.equal(gv[:, N:], ref['aug'].float().to(cdt)), what + ': aug columns'
  if c['kind'] == 'int':
    assert float(ref['C'].abs().max()) < 2 ** 24
    bad = (gv[:, :N] != ref['C'].float().to(cdt)).nonzero()
    assert bad.numel() == 0, '%s: %d wrong elements, first at %s' % (
        what, bad.shape[0], bad[0].tolist())
  else:
    e = rel(gv[:, :N], ref['C'])
    print('%s: C rel err %.3g (tol %.1g)' % (what, e, tol))
    assert e <= tol, what
  if s['colsum']:
    gs = out['colsum']
    pad = c['colsum_at']
    assert torch.equal(gs[:pad], c['colsum'][:pad]) and \
        torch.equal(gs[-pad:], c['colsum'][-pad:]), what + ': store outside colsum'
    gs = view1(gs, pad)
    assert not torch.isnan(gs).any(), what + ': NaN in colsum'
    if c['kind'] == 'int':
      assert torch.equal(gs, ref['colsum'].float()), what + ': colsum'
    else:
      e = rel(gs, ref['colsum'])
      print('%s: colsum rel err %.3g' % (what, e))
      assert e <= TOL[(s['dtype'], False)], what


def run_case(C, dev, s, child=False):
  """One case end to end: path asserts, exact check on integer operands,
  tolerance check on randn operands (twice when split: bitwise repeatable)."""
  for kind in ('int', 'randn'):
    c = make(s, kind)
    info = check_path(C, c, child)
    ref = reference(c)
    out = launch(C, dev, c)
    check(c, out, ref)
    if kind == 'randn' and info['splits'] > 1:
      again = launch(C, dev, c)
      assert all(torch.equal(out[k].view(torch.int16 if out[k].dtype == BF else torch.int32),
                             again[k].view(torch.int16 if again[k].dtype == BF else torch.int32))
                 for k in out), name(s) + ': two runs differ'
  return info


# --- the cases shared by tests/test_gemm_edges_gpu.py and its SA_GEMM_BL=0 child

LAYOUTS = ((False, False), (False, True), (True, False), (True, True))
# both ragged inside one tile; an exact tile; one row and one quad into the
# next tile; two tiles, aligned for fp32 only; the production f_in
PATH_MN = ((37, 29), (64, 64), (65, 68), (132, 100), (266, 64), (330, 64))


def bk(dtype):
  return 32 if dtype == 'f32' else 64


def path_matrix(dtype):
  """K = two whole K steps and one quad: the K loop runs its steady state,
  its last step and a ragged tail."""
  K = 2 * bk(dtype) + quad(dtype)
  return [spec(dtype, M, N, K, ta, tb, splits=1)
          for ta, tb in LAYOUTS for M, N in PATH_MN]


def ones_row(dtype):
  """The ones row (bias gradient) with colsum and accumulate: last row of a
  tile (M = 63), alone in a second block row (M = 64) and - op(A) = A^T -
  inside a scalar-tail quad (M = 266: 266 = 4 * 66 + 2); unsplit, 2 splits
  with a short last chunk, 16 splits with empty chunks."""
  q, b = quad(dtype), bk(dtype)
  out = []
  for K, sp, empty in ((2 * b + q, 1, False), (8 * b + q, 2, False), (64 * b + q, 16, True)):
    for ta, M, g0 in ((False, 63, 1), (True, 63, 1), (False, 64, 2), (True, 64, 2),
                      (True, 266, 5)):
      out.append(spec(dtype, M, 72, K, ta, False, accumulate=True, colsum=True,
                      splits=sp, empty_chunk=empty, grid0=g0))
  # any K for the weight-gradient form: a K row past the last whole step
  out.append(spec(dtype, 266, 72, 8 * b + 1, True, False, accumulate=True, colsum=True,
                  splits=2, grid0=5))
  return out


def child_main():
  """The SA_GEMM_BL=0 process: the path matrix and the ones-row cases on the
  bounds-checked kernels.  One 'case <name> ok' line each."""
  assert os.environ.get('SA_GEMM_BL') == '0'
  from scalable_agent_amd import ops
  C = ops.ext()
  dev = torch.device('cuda', 0)
  n = 0
  for dtype in ('f32', 'bf16'):
    for s in path_matrix(dtype) + ones_row(dtype):
      info = run_case(C, dev, s, child=True)
      assert info['bl'] is False
      if dtype == 'bf16' and not s['accumulate']:
        run_case(C, dev, dict(s, c_bf16=True), child=True)
      n += 1
      print('case %s bl=%s splits=%d ok' % (name(s), info['bl'], info['splits']), flush=True)
  print('cases %d' % n, flush=True)


if __name__ == '__main__':  # python -m tests._gemm_oracle, from the repository root
  child_main()
