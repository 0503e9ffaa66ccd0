"""The MFMA GEMMs (csrc/kernels/gemm_f32.hip, gemm_bf16.hip) at their
dispatch edges against the float64 oracle of tests/_gemm_oracle.py.

Every case first asserts from the launch-info hook (gemm_f32_info /
gemm_bf16_info: the launchers' own decision functions) that its shape takes
the path it is here for - bl or bounds-checked kernel, the split count, an
empty or short last K chunk, the grid - so a retune of the heuristics fails
these tests instead of silently turning their edges into plain cases.  Then
  * integer operands: torch.equal with the float64 reference cast to C's type
    (exact whatever the split count or summation order, see the oracle);
  * randn operands at the same shape: the project's tolerances (2e-6 fp32,
    3e-6 bf16 operands with an fp32 C, 8e-3 for a bf16 C), and for every split
    case a second run that must be bitwise equal;
  * poison: operands, mask, bias, rewards sit in NaN storage and C / colsum in
    sentinel storage; no NaN may come out, nothing outside C[:, :N] (or the
    aug columns N .. ldc) may change.
A bf16 case runs with an fp32 C and, unless it accumulates, with a bf16 C.

The bounds-checked kernels get the shapes the bl kernels take in-process
from one child process with SA_GEMM_BL=0 (the knob is read once per process).
The opt-in 128-row tile SA_GEMM_RM=2 is a measure_knob, read only in
SA_MEASURE_KNOBS builds: out of scope here (the hook must report rm = 1).
"""

import os
import subprocess
import sys

import pytest

from tests import _gemm_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ('f32', 'bf16')


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _run(dev, s):
  info = O.run_case(_C(), dev, s)
  if s['dtype'] == 'bf16' and not s['accumulate']:
    O.run_case(_C(), dev, dict(s, c_bf16=True))
  return info


def _all(fn):
  return [s for d in DTYPES for s in fn(d)]


def _two_shapes(dtype):
  """Both ragged inside one tile; whole quads, one quad into the next tile."""
  return ((37, 29), (68, 72)) if dtype == 'f32' else ((37, 29), (72, 80))


@pytest.mark.parametrize('s', _all(O.path_matrix), ids=O.name)
def test_path_matrix(cuda, s):
  """All four layouts, (True, True) included, over tile-edge shapes and the
  production f_in (266, 330): bl exactly where M (ta) and N (!tb) are whole
  quads, the bounds-checked kernel with its scalar tails elsewhere."""
  info = _run(cuda, s)
  q = O.quad(s['dtype'])
  assert info['bl'] == ((not s['ta'] or s['M'] % q == 0) and (s['tb'] or s['N'] % q == 0))
  assert info['splits'] == 1


def _k_edges(dtype):
  q, b = O.quad(dtype), O.bk(dtype)
  out = []
  for M, N in _two_shapes(dtype):
    for ta, tb in O.LAYOUTS:
      ks = [q, b, b + q, 2 * b, 2 * b + q]  # fp32: 4, 32, 36, 64, 68
      if ta and not tb:
        ks += [1, b - 1, b + 1]  # any K for the weight-gradient form
      out += [O.spec(dtype, M, N, K, ta, tb, splits=1) for K in ks]
  return out


@pytest.mark.parametrize('s', _all(_k_edges), ids=O.name)
def test_k_edges_unsplit(cuda, s):
  """One quad, one step exactly, one step and a quad, two steps, two and a
  quad; single rows around a step for op(A) = A^T, op(B) = B."""
  assert _run(cuda, s)['splits'] == 1


def _split_edges(dtype):
  b, q = O.bk(dtype), O.quad(dtype)
  short, empty = 8 * b + q, 64 * b + q  # fp32 260, 2052; bf16 520, 4104
  out = []
  for M, N in _two_shapes(dtype):
    for ta, tb in O.LAYOUTS:
      # 2 splits of 5 K steps: the second chunk is 3 steps and a quad long
      out.append(O.spec(dtype, M, N, short, ta, tb, splits=2, tail=3 * b + q))
      # 16 splits of 5 K steps cover 80 steps of the 64 and a quad there are
      out.append(O.spec(dtype, M, N, empty, ta, tb, splits=16, empty_chunk=True))
      if ta and not tb:
        out.append(O.spec(dtype, M, N, short - q + 1, ta, tb, splits=2, tail=3 * b + 1))
        out.append(O.spec(dtype, M, N, empty - q + 1, ta, tb, splits=16, empty_chunk=True))
  return out


@pytest.mark.parametrize('s', _all(_split_edges), ids=O.name)
def test_split_k_edges(cuda, s):
  """A short last chunk and chunks wholly past K (their partial slabs must
  still be written, as zeros); the randn run is repeated and bitwise equal."""
  info = _run(cuda, s)
  assert info['splits'] == s['splits'] > 1
  if s['empty_chunk']:
    # chunks 13 .. 15 of 16 start past K
    assert 13 * info['kchunk'] >= s['K'] > 12 * info['kchunk'], info


@pytest.mark.parametrize('s', _all(O.ones_row), ids=O.name)
def test_ones_row_at_tile_edges(cuda, s):
  """The bias-gradient row with colsum and accumulate: last row of a tile,
  alone in a second block row, inside the scalar-tail quad of op(A) = A^T at
  the production M = 266; unsplit, split, split with empty chunks."""
  assert _run(cuda, s)['grid'][0] == s['grid0']


def _epilogues(dtype):
  q, b = O.quad(dtype), O.bk(dtype)
  one, two = 2 * b + q, 8 * b + q  # unsplit / 2 splits
  out = []
  # relu(x W + b) next to the core-input columns, M ragged, ldc = 40; N a
  # whole number of quads (bl for op(B) = B) and not (bounds-checked)
  for N in ((28, 27) if dtype == 'f32' else (24, 28)):
    for tb in (False, True):
      for K, sp in ((one, 1), (two, 2)):
        out.append(O.spec(dtype, 37, N, K, False, tb, bias=True, relu=True, naug=40 - N,
                          splits=sp))
  # more aug elements than outputs: the reduce kernel's aug-only threads
  out.append(O.spec(dtype, 37, q, two, False, False, bias=True, relu=True, naug=24 - q,
                    splits=2))
  # mask (ldm > N by the embedding), alone and with accumulate
  for tb in (True, False):
    for K, sp in ((one, 1), (two, 2)):
      out.append(O.spec(dtype, 37, 29, K, False, tb, mask=True, splits=sp))
      out.append(O.spec(dtype, 65, 72, K, False, tb, mask=True, accumulate=True, splits=sp))
  # accumulate into a column slice of a wider C
  for ta in (True, False):
    for K, sp in ((one, 1), (two, 2)):
      out.append(O.spec(dtype, 65, 72, K, ta, False, accumulate=True, c_off=12, c_ld=96,
                        splits=sp))
      out.append(O.spec(dtype, 66, 29, K, ta, False, accumulate=True, c_off=8, c_ld=48,
                        splits=sp))
  return out


@pytest.mark.parametrize('s', _all(_epilogues), ids=O.name)
def test_epilogues_at_ragged_shapes(cuda, s):
  info = _run(cuda, s)
  if s['naug'] and s['N'] == O.quad(s['dtype']):
    # work = max(total, aug) of the reduce launch is the aug term
    assert info['splits'] > 1 and s['M'] * s['naug'] > s['M'] * s['N']


def test_bounds_checked_kernels_child(cuda):
  """SA_GEMM_BL=0 in a fresh process: the path-matrix and ones-row cases -
  among them every shape the bl kernels took above - on the bounds-checked
  kernels, through the same helpers."""
  env = dict(os.environ, SA_GEMM_BL='0', PYTHONPATH=ROOT)
  r = subprocess.run([sys.executable, '-m', 'tests._gemm_oracle'], cwd=ROOT,
                     capture_output=True, text=True, timeout=120, env=env)
  assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
  lines = [l for l in r.stdout.splitlines() if l.startswith('case ')]
  want = sum(len(O.path_matrix(d)) + len(O.ones_row(d)) for d in DTYPES)
  assert len(lines) == want == 80, r.stdout[-2000:]
  assert all(' bl=False ' in l and l.endswith(' ok') for l in lines)
  assert 'cases %d' % want in r.stdout
  # the shapes both programs were given: whole quads in M, N and K
  both = [s for d in DTYPES for s in O.path_matrix(d)
          if O.expect_bl(s) and s['K'] % O.quad(d) == 0]
  assert both and all(any(O.name(s) in l for l in lines) for s in both)
