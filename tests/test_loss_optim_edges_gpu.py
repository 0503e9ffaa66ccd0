"""Float64 oracles at the dispatch edges of the loss and RMSProp kernels.

Kernels under test: learner_head_fwd / learner_head_bwd (learner_io.hip),
vtrace_loss_kernel (vtrace_loss.hip), rmsprop_kernel / finite_check_kernel
(rmsprop.hip).  Every oracle runs in float64 on the CPU through the project's
own vtrace.from_logits / losses.* / optim.polynomial_decay with autograd
gradients; inputs are drawn on the CPU from a fixed seed and copied to the
device, so oracle and kernel read identical bits.

Bounds (against float64): vs / pg_adv / PopArt targets rtol 1e-4 atol 1e-4;
loss terms rtol 1e-4 atol 1e-3; every gradient tensor relative Frobenius
error <= 1e-4; RMSProp ms rtol 1e-6 atol 1e-6, mom rtol 1e-5 atol 1e-8,
w rtol 1e-6 atol 1e-6.  Nothing is masked.  Each check prints error / bound;
the module prints the largest ratio per kernel when it finishes (pytest -s).

Case -> branch:

  heads (T, B, A)          branch
  (1, 1, 1)                smallest problem; A = 1 (policy gradient == 0)
  (15, 16, 15)             value column = last column of the 16-wide tile;
                           T1 = 16 (one full MFMA row tile); bwd N1 = 256 = ROWS
  (16, 3, 16)              MAXC 16 -> 32 switch (A + 1 = 17); T1 = 17
  (63, 2, 31)              full 32-wide tile; last lane of wave 0 of the scan
  (64, 2, 9), (65, 2, 9)   `lane < 63` hand-off, cross-wave scan_a/scan_b walk
  (255, 1, 15)             ntiles = 16 (T1 = 256), one tile per wave
  (256, 1, 16)             ntiles = 17 (T1 = 257), second tile pass; bwd
                           N1 = 257 = ROWS + 1
  (1023, 1, 3), (1024, 1, 3)  last thread of the scan, C = 1
  (1025, 2, 9)             T > 1024: C = 2, the `tid + kHeadThreads` prologue
                           loops (behaviour, rewards, actions, done)
  (3, 257, 9)              B beyond any tested ticket reduction; bwd N1 = 1028,
                           the last chunk holds only rows >= Ng
  done patterns (65, 4, 9) all-done, never-done, last-row-only, p = 0.5, and
                           the four of them side by side
  B = 5 then B = 3         ticket reset across differing grids
  A = 31 / 9 at T = max    LDS bound (static + dynamic LDS), max + 1 rejected
                           on the host

  PopArt (T, B, A, K)      bwd A + K
  (9, 5, 9, 7 / 8)         16 / 17 (MAXC 16 -> 32)
  (9, 5, 9, 23 / 24)       32 / 33 (MAXC 32 -> 64, ROWS 256 -> 128)
  (20, 6, 31, 33)          64 (the widest)
  (127, 1, 9, 24)          N1 = 128 = ROWS of the 64-wide kernel
  task 'last' / 'zero'     a batch that uses head K - 1 / only head 0

  vtrace_loss (T, B, A)    branch
  (1, 1, 1)                smallest problem
  (63, 16, 2)              C = 1 with a ragged last lane; B = 16 (all waves)
  (64, 17, 9)              C = 1 full; B = 17 wraps the 16-wave column stride
  (65, 1, 9)               C = 2
  (129, 33, 40)            C = 3, ragged; third column pass
  x clip (1, 1), (0.5, 2), (None, None) -> inf

  RMSProp                  branch
  n = 2048*256*4 + 192     second, partial grid-stride pass; 3 carried steps,
                           grad_scale = 0.25, momentum 0.9
  n = 4, 64, 64004         tail block partly idle
  frames = 2 F / 0         lr == 0 / lr == lr0
  nan / inf / -inf         at 0, n - 1, first element of the second pass
  lstm_err words           passed as plain data
"""

import pytest
import torch

from scalable_agent_amd import losses as losses_lib
from scalable_agent_amd import vtrace as vtrace_lib
from scalable_agent_amd.optim import polynomial_decay
from scalable_agent_amd.popart import PopArt

pytestmark = pytest.mark.gpu

_WORST = {}


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


def _note(kernel, what, ratio):
  print('  [%s] %-14s error/bound = %.4g' % (kernel, what, ratio))
  if not ratio <= _WORST.get(kernel, (0.0, ''))[0]:
    _WORST[kernel] = (ratio, what)


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
  yield
  for k in sorted(_WORST):
    print('\nworst error/bound vs float64, %s: %.4g (%s)' % ((k,) + _WORST[k]))


def _close(kernel, what, got, ref, rtol, atol):
  """Elementwise |got - ref| <= atol + rtol |ref| against the float64 ref."""
  got = got.detach().double().cpu()
  ref = ref.detach().double().cpu()
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  ratio = float(((got - ref).abs() / (atol + rtol * ref.abs())).max())
  _note(kernel, what, ratio)
  assert ratio <= 1.0, '%s: error/bound = %g' % (what, ratio)


def _frob(kernel, what, got, ref, bound=1e-4):
  """Relative Frobenius error <= bound (a zero reference wants exact zeros)."""
  got = got.detach().double().cpu()
  ref = ref.detach().double().cpu()
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  if float(ref.norm()) == 0.0:
    assert torch.count_nonzero(got) == 0, what
    return
  ratio = float((got - ref).norm() / ref.norm()) / bound
  _note(kernel, what, ratio)
  assert ratio <= 1.0, '%s: error/bound = %g' % (what, ratio)


def _done(gen, rows, B, pattern):
  """[rows, B] bool; the kernels read every row given to them."""
  if pattern == 'rand':
    return torch.rand(rows, B, generator=gen) < 0.05
  cols = {'all': torch.ones(rows, dtype=torch.bool),
          'never': torch.zeros(rows, dtype=torch.bool),
          'last': torch.zeros(rows, dtype=torch.bool),
          'half': None}
  cols['last'][-1] = True
  names = ['all', 'never', 'last', 'half'] if pattern == 'mixed' else [pattern]
  out = torch.empty(rows, B, dtype=torch.bool)
  for b in range(B):
    name = names[b % len(names)]
    out[:, b] = (torch.rand(rows, generator=gen) < 0.5 if name == 'half'
                 else cols[name])
  return out


_PATTERNS = ['all', 'never', 'last', 'half', 'mixed']


# ------------------------------------------------------------- fused heads

def _heads_inputs(T, B, A, K, seed, pattern='rand'):
  g = torch.Generator().manual_seed(seed)
  T1 = T + 1
  r = lambda *s: torch.randn(*s, generator=g)
  d = dict(core=r(T1, B, 256), wp=r(256, A) * 0.05, bp=r(A) * 0.1,
           wb=r(256, K) * 0.05, bb=r(K) * 0.1, beh=r(T1, B, A),
           act=torch.randint(0, A, (T1, B), generator=g), rew=r(T1, B) * 2)
  # row 0 of done is not read by the loss; rows 1..T carry the pattern
  d['done'] = torch.cat([torch.zeros(1, B, dtype=torch.bool),
                         _done(g, T, B, pattern)], 0)
  return d


_LEAVES = ('core', 'wp', 'bp', 'wb', 'bb')


def _heads_oracle(d, clip, bc, ec, task=None, mu=None, nu=None):
  """float64 loss, its gradients under a 2x incoming gradient, vs [T, B]."""
  leaves = [d[k].double().requires_grad_() for k in _LEAVES]
  core, wp, bp, wb, bb = leaves
  beh, act, rew, done = d['beh'].double(), d['act'], d['rew'].double(), d['done']
  logits = core @ wp + bp
  values_all = core @ wb + bb                            # [T1, B, K]
  B = core.shape[1]
  kt = torch.zeros(B, dtype=torch.int64) if task is None else task
  idx = kt.view(1, -1, 1).expand(values_all.shape[0], -1, 1)
  n = values_all.gather(-1, idx).squeeze(-1)             # normalised values
  if mu is None:
    sigma, m = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
  else:
    pa = PopArt(mu.numel())
    pa.mu, pa.nu = mu.double(), nu.double()
    sigma, m = pa.stats_for(kt)
  discounts = (~done[1:]).double() * 0.99
  vt = vtrace_lib.from_logits(
      behaviour_policy_logits=beh[1:], target_policy_logits=logits[:-1],
      actions=act[1:], discounts=discounts,
      rewards=losses_lib.clip_rewards(rew[1:], clip), values=n[:-1] * sigma + m,
      bootstrap_value=n[-1] * sigma + m)
  assert vt.vs.dtype == torch.float64
  err = (vt.vs - m) / sigma - n[:-1]
  total = losses_lib.compute_policy_gradient_loss(logits[:-1], act[1:],
                                                  vt.pg_advantages / sigma)
  total = total + bc * losses_lib.compute_baseline_loss(err)
  total = total + ec * losses_lib.compute_entropy_loss(logits[:-1])
  (2.0 * total).backward()
  return total.detach(), [t.grad for t in leaves], vt.vs


def _heads_check(cuda, d, clip, task=None, mu=None, nu=None):
  """Runs the fused pair on the device and checks loss, gradients (and the
  PopArt targets) against the oracle.  Returns the device gradients."""
  ops = _ops()
  bc, ec = 0.5, 0.01
  ref, gref, vs_ref = _heads_oracle(d, clip, bc, ec, task, mu, nu)
  leaves = [d[k].to(cuda).requires_grad_() for k in _LEAVES]
  kw, aux = {}, None
  if task is not None:
    kw['task_ids'] = task.to(cuda)
  if mu is not None:
    pa = PopArt(mu.numel(), device=cuda)
    pa.mu.copy_(mu)
    pa.nu.copy_(nu)
    aux = {}
    kw.update(popart=pa, aux=aux)
  loss = ops.heads_vtrace_loss(*leaves, d['beh'].to(cuda), d['act'].to(cuda),
                               d['rew'].to(cuda), d['done'].to(cuda), 0.99,
                               clip, bc, ec, **kw)
  _close('learner_head_fwd', 'loss', loss, ref, 1e-4, 1e-3)
  if aux is not None:
    _close('learner_head_fwd', 'targets', aux['targets'], vs_ref, 1e-4, 1e-4)
  (2.0 * loss).backward()
  for name, t, g in zip(_LEAVES, leaves, gref):
    assert t.grad is not None, name
    _frob('learner_head_bwd', 'd' + name, t.grad, g)
  return [t.grad for t in leaves]


_HEAD_CASES = [(1, 1, 1), (15, 16, 15), (16, 3, 16), (63, 2, 31), (64, 2, 9),
               (65, 2, 9), (255, 1, 15), (256, 1, 16), (1023, 1, 3),
               (1024, 1, 3), (1025, 2, 9), (3, 257, 9)]
_CLIPS = ['abs_one', 'soft_asymmetric']


@pytest.mark.parametrize('case', range(len(_HEAD_CASES)),
                         ids=['%d-%d-%d' % c for c in _HEAD_CASES])
def test_heads_edges_match_float64(cuda, case):
  T, B, A = _HEAD_CASES[case]
  d = _heads_inputs(T, B, A, 1, seed=100 + case)
  grads = _heads_check(cuda, d, _CLIPS[case % 2])
  if A == 1:  # one action: softmax == 1, no policy gradient at all
    assert torch.count_nonzero(grads[1]) == 0
    assert torch.count_nonzero(grads[2]) == 0


@pytest.mark.parametrize('pattern', _PATTERNS)
def test_heads_done_patterns_match_float64(cuda, pattern):
  d = _heads_inputs(65, 4, 9, 1, seed=200, pattern=pattern)
  if pattern == 'mixed':
    done = d['done'][1:]
    assert done[:, 0].all() and not done[:, 1].any()
    assert done[-1, 2] and not done[:-1, 2].any()
  _heads_check(cuda, d, _CLIPS[_PATTERNS.index(pattern) % 2])


def test_heads_ticket_resets_across_grids(cuda):
  """B = 5 then B = 3 back to back: the second launch's last workgroup is
  found only when the first one left the ticket at zero."""
  for B in (5, 3):
    _heads_check(cuda, _heads_inputs(12, B, 9, 1, seed=300 + B), 'abs_one')


_POPART_CASES = [(9, 5, 9, 7), (9, 5, 9, 8), (9, 5, 9, 23), (9, 5, 9, 24),
                 (20, 6, 31, 33), (127, 1, 9, 24)]


@pytest.mark.parametrize('tasks', ['last', 'zero'])
@pytest.mark.parametrize('case', range(len(_POPART_CASES)),
                         ids=['%d-%d-%d-%d' % c for c in _POPART_CASES])
def test_heads_popart_edges_match_float64(cuda, case, tasks):
  T, B, A, K = _POPART_CASES[case]
  d = _heads_inputs(T, B, A, K, seed=400 + case)
  g = torch.Generator().manual_seed(500 + case)
  mu = torch.randn(K, generator=g) * 3
  nu = mu * mu + torch.rand(K, generator=g) * 20 + 0.5
  if tasks == 'zero':
    task = torch.zeros(B, dtype=torch.int64)
  else:
    task = torch.randint(0, K, (B,), generator=g)
    task[B - 1] = K - 1
  grads = _heads_check(cuda, d, 'abs_one', task=task, mu=mu, nu=nu)
  # only the heads the batch uses get a value-head gradient
  unused = torch.ones(K, dtype=torch.bool)
  unused[task] = False
  assert unused.any()
  assert torch.count_nonzero(grads[3].cpu()[:, unused]) == 0
  assert torch.count_nonzero(grads[4].cpu()[unused]) == 0


@pytest.mark.parametrize('A', [31, 9])
def test_heads_lds_bound(cuda, A):
  """The longest unroll that fits the workgroup's LDS (dynamic and static
  together) matches the oracle; one step more is refused on the host."""
  ops = _ops()
  tmax = ops.learner_head_max_unroll(A)
  assert tmax >= 300  # the longest unroll of the older tests (A = 18) fits
  _heads_check(cuda, _heads_inputs(tmax, 2, A, 1, seed=600 + A), 'abs_one')
  d = _heads_inputs(tmax + 1, 2, A, 1, seed=700 + A)
  args = [d[k].to(cuda) for k in _LEAVES + ('beh', 'act', 'rew', 'done')]
  with pytest.raises(RuntimeError, match='unroll too long'):
    ops.heads_vtrace_loss(*args, 0.99, 'abs_one', 0.5, 0.01)
  torch.cuda.synchronize()


# ------------------------------------------------------ generic vtrace_loss

def _vtrace_inputs(T, B, A, seed, pattern='rand'):
  g = torch.Generator().manual_seed(seed)
  r = lambda *s: torch.randn(*s, generator=g)
  return dict(bl=r(T, B, A), tl=r(T, B, A),
              a=torch.randint(0, A, (T, B), generator=g), r=r(T, B) * 3,
              done=_done(g, T, B, pattern), v=r(T, B), boot=r(B))


def _vtrace_oracle(d, clip, bc, ec, clip_rho, clip_pg_rho):
  tl = d['tl'].double().requires_grad_()
  v = d['v'].double().requires_grad_()
  disc = (~d['done']).double() * 0.99
  vt = vtrace_lib.from_logits(d['bl'].double(), tl, d['a'], disc,
                              losses_lib.clip_rewards(d['r'].double(), clip), v,
                              d['boot'].double(), clip_rho_threshold=clip_rho,
                              clip_pg_rho_threshold=clip_pg_rho)
  assert vt.vs.dtype == torch.float64
  pg = losses_lib.compute_policy_gradient_loss(tl, d['a'], vt.pg_advantages)
  bl = losses_lib.compute_baseline_loss(vt.vs - v)
  en = losses_lib.compute_entropy_loss(tl)
  total = pg + bc * bl + ec * en
  total.backward()
  terms = torch.stack([total, pg, bl, en]).detach()
  return terms, tl.grad, v.grad, vt.vs, vt.pg_advantages


def _vtrace_check(cuda, d, clip, clip_rho, clip_pg_rho, wrapper):
  ops = _ops()
  bc, ec = 0.5, 0.01
  terms, dl_ref, dv_ref, vs_ref, pg_ref = _vtrace_oracle(d, clip, bc, ec,
                                                        clip_rho, clip_pg_rho)
  dev = {k: t.to(cuda) for k, t in d.items()}
  args = (dev['bl'], dev['tl'], dev['a'], dev['r'], dev['done'], dev['v'],
          dev['boot'])
  loss, dlogits, dvalues, vs, pga = ops.vtrace_fused_forward(
      *args, reward_clipping=clip, baseline_cost=bc, entropy_cost=ec,
      clip_rho=clip_rho, clip_pg_rho=clip_pg_rho)
  k = 'vtrace_loss'
  _close(k, 'vs', vs, vs_ref, 1e-4, 1e-4)
  _close(k, 'pg_adv', pga, pg_ref, 1e-4, 1e-4)
  _close(k, 'loss terms', loss, terms, 1e-4, 1e-3)
  _frob(k, 'dlogits', dlogits, dl_ref)
  _frob(k, 'dvalues', dvalues, dv_ref)
  if wrapper:  # the autograd wrapper runs the default thresholds (1, 1)
    tl = dev['tl'].clone().requires_grad_()
    v = dev['v'].clone().requires_grad_()
    total = ops.vtrace_loss(dev['bl'], tl, dev['a'], dev['r'], dev['done'], v,
                            dev['boot'], reward_clipping=clip, baseline_cost=bc,
                            entropy_cost=ec)
    _close(k, 'wrapper loss', total, terms[0], 1e-4, 1e-3)
    (2.0 * total).backward()
    _frob(k, 'wrapper dlogits', tl.grad, 2.0 * dl_ref)
    _frob(k, 'wrapper dvalues', v.grad, 2.0 * dv_ref)


_VTRACE_CASES = [(1, 1, 1), (63, 16, 2), (64, 17, 9), (65, 1, 9), (129, 33, 40)]
_RHO_CLIPS = [(1.0, 1.0), (0.5, 2.0), (None, None)]


@pytest.mark.parametrize('rho', range(len(_RHO_CLIPS)),
                         ids=['1-1', '0.5-2', 'none'])
@pytest.mark.parametrize('case', range(len(_VTRACE_CASES)),
                         ids=['%d-%d-%d' % c for c in _VTRACE_CASES])
def test_vtrace_loss_edges_match_float64(cuda, case, rho):
  T, B, A = _VTRACE_CASES[case]
  clip_rho, clip_pg_rho = _RHO_CLIPS[rho]
  d = _vtrace_inputs(T, B, A, seed=800 + case)
  _vtrace_check(cuda, d, _CLIPS[(case + rho) % 2], clip_rho, clip_pg_rho,
                wrapper=rho == 0)


@pytest.mark.parametrize('pattern', _PATTERNS)
def test_vtrace_loss_done_patterns_match_float64(cuda, pattern):
  d = _vtrace_inputs(65, 4, 9, seed=900, pattern=pattern)
  _vtrace_check(cuda, d, _CLIPS[_PATTERNS.index(pattern) % 2], 1.0, 1.0,
                wrapper=True)


# ------------------------------------------------------------------ RMSProp

_BIG_N = 2048 * 256 * 4 + 64 * 3     # one full grid-stride pass and a partial
_SECOND_PASS = 2048 * 256 * 4        # first element of the second pass
_LR0, _FRAMES_TOTAL, _DECAY, _EPS = 4.8e-4, 1e6, 0.99, 0.1
_STATE = {}


def _rms_state(n):
  """(w, ms, mom, three gradients) on the CPU, drawn once per size."""
  if n not in _STATE:
    g = torch.Generator().manual_seed(n)
    _STATE[n] = (torch.randn(n, generator=g),
                 torch.ones(n) + torch.rand(n, generator=g),
                 torch.randn(n, generator=g) * 0.01,
                 [torch.randn(n, generator=g) for _ in range(3)])
  return _STATE[n]


def _rms_ref(w, g, ms, mom, frames, momentum, grad_scale):
  """One step of the formula in rmsprop.hip's header, float64."""
  lr = polynomial_decay(_LR0, frames, _FRAMES_TOTAL)
  g = grad_scale * g.double()
  ms = ms + (g * g - ms) * (1 - _DECAY)
  mom = momentum * mom + lr * g / torch.sqrt(ms + _EPS)
  return w - mom, ms, mom


def _rms_close(w, ms, mom, ref):
  k = 'rmsprop'
  _close(k, 'ms', ms, ref[1], 1e-6, 1e-6)
  _close(k, 'mom', mom, ref[2], 1e-5, 1e-8)
  _close(k, 'w', w, ref[0], 1e-6, 1e-6)


def _frames(cuda, f):
  return torch.tensor(int(f), device=cuda, dtype=torch.int64)


def test_rmsprop_grid_stride_three_steps(cuda):
  ops = _ops()
  n = _BIG_N
  w0, ms0, mom0, grads = _rms_state(n)
  w, ms, mom = w0.to(cuda), ms0.to(cuda), mom0.to(cuda)
  ref = (w0.double(), ms0.double(), mom0.double())
  for step, g in enumerate(grads):
    frames = 123456 + 4000 * step
    ops.rmsprop_step(w, g.to(cuda), ms, mom, _frames(cuda, frames), _LR0,
                     _FRAMES_TOTAL, _DECAY, 0.9, _EPS, grad_scale=0.25)
    ref = _rms_ref(ref[0], g, ref[1], ref[2], frames, 0.9, 0.25)
  _rms_close(w, ms, mom, ref)
  # the second pass did run: its elements moved
  assert not torch.equal(w[_SECOND_PASS:].cpu(), w0[_SECOND_PASS:])


@pytest.mark.parametrize('n', [4, 64, 64 * 1000 + 4])
@pytest.mark.parametrize('frames', [0, 123456])
def test_rmsprop_small_and_odd_sizes(cuda, n, frames):
  """Tail block partly idle; frames == 0 is the undecayed lr0."""
  ops = _ops()
  if frames == 0:
    assert polynomial_decay(_LR0, 0, _FRAMES_TOTAL) == _LR0
  w0, ms0, mom0, grads = _rms_state(n)
  w, ms, mom = w0.to(cuda), ms0.to(cuda), mom0.to(cuda)
  ops.rmsprop_step(w, grads[0].to(cuda), ms, mom, _frames(cuda, frames), _LR0,
                   _FRAMES_TOTAL, _DECAY, 0.9, _EPS)
  _rms_close(w, ms, mom, _rms_ref(w0.double(), grads[0], ms0.double(),
                                  mom0.double(), frames, 0.9, 1.0))


def test_rmsprop_decay_exhausted(cuda):
  """frames past total_frames: lr == 0, so mom only decays and w moves by it
  (bitwise); ms still follows its formula."""
  ops = _ops()
  n = 64 * 1000 + 4
  frames = 2 * int(_FRAMES_TOTAL)
  assert polynomial_decay(_LR0, frames, _FRAMES_TOTAL) == 0.0
  w0, ms0, mom0, grads = _rms_state(n)
  w, ms, mom = w0.to(cuda), ms0.to(cuda), mom0.to(cuda)
  ops.rmsprop_step(w, grads[0].to(cuda), ms, mom, _frames(cuda, frames), _LR0,
                   _FRAMES_TOTAL, _DECAY, 0.9, _EPS, grad_scale=0.25)
  mom_exp = mom0 * 0.9            # one correctly rounded fp32 product
  assert torch.equal(mom.cpu(), mom_exp)
  assert torch.equal(w.cpu(), w0 - mom_exp)
  _rms_close(w, ms, mom, _rms_ref(w0.double(), grads[0], ms0.double(),
                                  mom0.double(), frames, 0.9, 0.25))


@pytest.mark.parametrize('pos,bad', [(0, 'nan'), (_BIG_N - 1, 'inf'),
                                     (_SECOND_PASS, '-inf')])
def test_rmsprop_guard_positions(cuda, pos, bad):
  ops = _ops()
  n = _BIG_N
  w0, ms0, mom0, grads = _rms_state(n)
  w, ms, mom = w0.to(cuda), ms0.to(cuda), mom0.to(cuda)
  guard = torch.zeros(4, dtype=torch.int32, device=cuda)
  g = grads[0].clone()
  g[pos] = float(bad)
  step = lambda grad: ops.rmsprop_step(
      w, grad.to(cuda), ms, mom, _frames(cuda, 123456), _LR0, _FRAMES_TOTAL,
      _DECAY, 0.9, _EPS, guard)
  step(g)
  assert guard.tolist()[:2] == [1, 1]
  assert torch.equal(w.cpu(), w0)
  assert torch.equal(ms.cpu(), ms0)
  assert torch.equal(mom.cpu(), mom0)
  step(grads[0])  # the next, finite step applies
  assert guard.tolist() == [0, 1, 0, 0]
  _rms_close(w, ms, mom, _rms_ref(w0.double(), grads[0], ms0.double(),
                                  mom0.double(), 123456, 0.9, 1.0))


@pytest.mark.parametrize('words,expect', [([1, 0, 0, 0], [2, 1, 1, 0]),
                                          ([1, 1, 0, 0], [2, 1, 1, 1])])
def test_rmsprop_error_words(cuda, words, expect):
  """The sticky error words given as plain data: the step is skipped and
  counted, the words are consumed, the next step applies."""
  ops = _ops()
  n = 64 * 1000 + 4
  w0, ms0, mom0, grads = _rms_state(n)
  w, ms, mom = w0.to(cuda), ms0.to(cuda), mom0.to(cuda)
  guard = torch.zeros(4, dtype=torch.int32, device=cuda)
  err = torch.tensor(words, dtype=torch.int32, device=cuda)
  step = lambda: ops.rmsprop_step(
      w, grads[0].to(cuda), ms, mom, _frames(cuda, 123456), _LR0,
      _FRAMES_TOTAL, _DECAY, 0.9, _EPS, guard, err)
  step()
  assert guard.tolist() == expect
  assert err.tolist() == [0, 0, 0, 0]
  assert torch.equal(w.cpu(), w0)
  assert torch.equal(ms.cpu(), ms0)
  assert torch.equal(mom.cpu(), mom0)
  step()
  assert guard.tolist() == [0] + expect[1:]
  _rms_close(w, ms, mom, _rms_ref(w0.double(), grads[0], ms0.double(),
                                  mom0.double(), 123456, 0.9, 1.0))
