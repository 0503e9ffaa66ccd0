"""The time-tiled fused learner heads (learner_head_fwd_tiled, learner_io.hip)
against a float64 oracle: any unroll length, up to 63 actions.

ops.heads_vtrace_loss(..., time_tile=TC) walks each batch column in tiles of
TC steps from the END of the unroll: the tiles of T steps are [T - TC, T),
[T - 2 TC, T - TC), ..., [0, remainder), the V-trace accumulator and vs of a
tile's first step carried into the next tile.  The oracle runs in float64 on
the CPU through vtrace.from_logits / losses.* with autograd gradients (under
a 2x incoming gradient); inputs are drawn on the CPU from a fixed seed and
copied to the device, so oracle and kernel read identical bits.

Bounds (the project's, tests/test_loss_optim_edges_gpu.py): vs / PopArt
targets rtol 1e-4 atol 1e-4; loss rtol 1e-4 atol 1e-3; every gradient tensor
(dcore, dwp, dbp, dwb, dbb) relative Frobenius error <= 1e-4.  Past the old
unroll limit (T > 436) the torch fp32 loss path (compute_loss,
use_fused=False) runs on the same inputs on the CPU, e_torch is its error
against float64, and the bound is max(project bound, 1.5 e_torch) (the rule
of tests/test_learner_parity_gpu.py).  Nothing is masked.  Each check prints
error / bound (pytest -s); the module prints the largest ratio at its end.

Case -> branch:

  time_tile 16, T = 1, 15, 16   one tile: of 1 step, of 15, exactly full
            17, 33              remainder tile of 1 step (2 / 3 tiles)
            31                  remainder tile of 15 steps
            32, 48              exact multiples (2 / 3 tiles)
  time_tile 32, T = 33, 65      remainder 1; 64: exact; 100: remainder 4
    each x B in {1, 3} x A in {1, 9, 15, 16, 31} (A + 1 = 16 | 17: MAXC 16 ->
    32; 32: the full 32-wide image)
  carries (T 40, tile 16: tiles [24,40) [8,24) [0,8)), one column each:
    done at step 23 (a tile's last step), at step 24 (a tile's first step),
    all of tile [8,24), none (the carry crosses every tile); rho > 1 and
    |reward| > 1 forced at steps 7, 8, 23, 24; both reward clippings
  wide heads (MAXC 64)          A = 32, 33, 47, 63 at T 20, tile 16; PopArt
                                A 40 + K 24
  PopArt K 3                    columns of tasks 0 / 2 over 3 tiles, targets,
                                head 1 unused: exactly zero gradient
  (437, 2, 31), (1400, 2, 9)    past learner_head_max_unroll, tile 'auto'
  T 100, tiles 16 / 48 / 112    and the untiled kernel: one answer; bitwise
                                repeatable per tile
  B = 5, 2, 7                   ticket re-armed across differing grids
  graph                         captured forward + backward replays bitwise
  refusals                      tile 20, 2048, A 64, a tile past the LDS; the
                                untiled path still refuses T = max + 1
"""

import types

import pytest
import torch

from scalable_agent_amd import losses as losses_lib
from scalable_agent_amd import vtrace as vtrace_lib
from scalable_agent_amd.learner import compute_loss
from scalable_agent_amd.popart import PopArt
from scalable_agent_amd.structs import ActorOutput, AgentOutput, StepOutput

pytestmark = pytest.mark.gpu

_WORST = {}
_LEAVES = ('core', 'wp', 'bp', 'wb', 'bb')
_BC, _EC, _GAMMA = 0.5, 0.01, 0.99


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


def _note(kernel, what, ratio):
  print('  [%s] %-10s error/bound = %.4g' % (kernel, what, ratio))
  if not ratio <= _WORST.get(kernel, (0.0, ''))[0]:
    _WORST[kernel] = (ratio, what)


@pytest.fixture(scope='module', autouse=True)
def _report_worst():
  yield
  for k in sorted(_WORST):
    print('\nworst error/bound vs float64, %s: %.4g (%s)' % ((k,) + _WORST[k]))


def _close(kernel, what, got, ref, rtol, atol, e_torch=None):
  """Elementwise |got - ref| <= max(atol + rtol |ref|, 1.5 e_torch)."""
  got = got.detach().double().cpu()
  ref = ref.detach().double().cpu()
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  bound = atol + rtol * ref.abs()
  if e_torch is not None:
    bound = torch.maximum(bound, 1.5 * e_torch)
  ratio = float(((got - ref).abs() / bound).max())
  _note(kernel, what, ratio)
  assert ratio <= 1.0, '%s: error/bound = %g' % (what, ratio)


def _frob_err(got, ref):
  return float((got.detach().double().cpu() - ref).norm() / ref.norm())


def _frob(kernel, what, got, ref, e_torch=None):
  """Relative Frobenius error <= max(1e-4, 1.5 e_torch) (a zero reference
  wants exact zeros)."""
  ref = ref.detach().double().cpu()
  assert got.shape == ref.shape, (what, got.shape, ref.shape)
  if float(ref.norm()) == 0.0:
    assert torch.count_nonzero(got) == 0, what
    return
  bound = 1e-4 if e_torch is None else max(1e-4, 1.5 * e_torch)
  ratio = _frob_err(got, ref) / bound
  _note(kernel, what, ratio)
  assert ratio <= 1.0, '%s: error/bound = %g' % (what, ratio)


def _inputs(T, B, A, K, seed, done=None):
  g = torch.Generator().manual_seed(seed)
  T1 = T + 1
  r = lambda *s: torch.randn(*s, generator=g)
  d = dict(core=r(T1, B, 256), wp=r(256, A) * 0.05, bp=r(A) * 0.1,
           wb=r(256, K) * 0.05, bb=r(K) * 0.1, beh=r(T1, B, A),
           act=torch.randint(0, A, (T1, B), generator=g), rew=r(T1, B) * 2)
  # row 0 of done is not read by the loss; step t reads row t + 1
  d['done'] = torch.zeros(T1, B, dtype=torch.bool)
  d['done'][1:] = (torch.rand(T, B, generator=g) < 0.05) if done is None else done
  return d


def _oracle(d, clip, task=None, mu=None, nu=None):
  """float64: loss, its gradients under a 2x incoming gradient, vs [T, B],
  log rho [T, B]."""
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
    sigma = torch.ones(B, dtype=torch.float64)
    m = torch.zeros(B, dtype=torch.float64)
  else:
    pa = PopArt(mu.numel())
    pa.mu, pa.nu = mu.double(), nu.double()
    sigma, m = pa.stats_for(kt)
  discounts = (~done[1:]).double() * _GAMMA
  vt = vtrace_lib.from_logits(
      behaviour_policy_logits=beh[1:], target_policy_logits=logits[:-1],
      actions=act[1:], discounts=discounts,
      rewards=losses_lib.clip_rewards(rew[1:], clip), values=n[:-1] * sigma + m,
      bootstrap_value=n[-1] * sigma + m)
  assert vt.vs.dtype == torch.float64
  err = (vt.vs - m) / sigma - n[:-1]
  total = losses_lib.compute_policy_gradient_loss(logits[:-1], act[1:],
                                                  vt.pg_advantages / sigma)
  total = total + _BC * losses_lib.compute_baseline_loss(err)
  total = total + _EC * losses_lib.compute_entropy_loss(logits[:-1])
  (2.0 * total).backward()
  return (total.detach(), [t.grad for t in leaves], vt.vs.detach(),
          vt.log_rhos.detach())


class _HeadsOnlyAgent(object):
  """compute_loss's unfused path over given core outputs: the heads in torch."""

  def __init__(self, leaves):
    self.core, self.wp, self.bp, self.wb, self.bb = leaves

  def unroll(self, actions, env_outputs, state, sample=False, task_ids=None):
    logits = self.core @ self.wp + self.bp
    baseline = (self.core @ self.wb + self.bb).squeeze(-1)
    return AgentOutput(actions, logits, baseline), state


def _torch_fp32_errors(d, clip, ref, gref):
  """The torch fp32 loss path on the CPU against float64: (|loss error|,
  [relative Frobenius error per gradient])."""
  leaves = [d[k].clone().requires_grad_() for k in _LEAVES]
  flags = types.SimpleNamespace(discounting=_GAMMA, reward_clipping=clip,
                                baseline_cost=_BC, entropy_cost=_EC)
  data = ActorOutput(
      level_name=None, agent_state=None,
      env_outputs=StepOutput(d['rew'], None, d['done'], (None, None)),
      agent_outputs=AgentOutput(d['act'], d['beh'], None))
  loss = compute_loss(_HeadsOnlyAgent(leaves), data, flags, use_fused=False)
  assert loss.dtype == torch.float32
  (2.0 * loss).backward()
  return (abs(float(loss.detach().double() - ref)),
          [_frob_err(t.grad, g) for t, g in zip(leaves, gref)])


def _run(cuda, d, clip, time_tile, task=None, mu=None, nu=None):
  """The fused pair on the device -> (loss, leaves, aux)."""
  ops = _ops()
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
  if time_tile is not None:
    kw['time_tile'] = time_tile
  loss = ops.heads_vtrace_loss(*leaves, d['beh'].to(cuda), d['act'].to(cuda),
                               d['rew'].to(cuda), d['done'].to(cuda), _GAMMA,
                               clip, _BC, _EC, **kw)
  return loss, leaves, aux


def _check(cuda, d, clip, time_tile, task=None, mu=None, nu=None,
           oracle=None, torch_bound=False):
  """Loss, gradients (and the PopArt targets) of the device run against the
  oracle.  Returns the device gradients."""
  ref, gref, vs_ref, _ = oracle or _oracle(d, clip, task, mu, nu)
  e_loss, e_grads = None, [None] * len(_LEAVES)
  if torch_bound:
    e_loss, e_grads = _torch_fp32_errors(d, clip, ref, gref)
    print('  torch fp32 vs float64: loss %.3g, gradients %s'
          % (e_loss, ' '.join('%.3g' % e for e in e_grads)))
    e_loss = torch.tensor(e_loss, dtype=torch.float64)
  fwd = 'learner_head_fwd' + ('' if time_tile is None else '_tiled')
  loss, leaves, aux = _run(cuda, d, clip, time_tile, task, mu, nu)
  _close(fwd, 'loss', loss, ref, 1e-4, 1e-3, e_loss)
  if aux is not None:
    _close(fwd, 'targets', aux['targets'], vs_ref, 1e-4, 1e-4)
  (2.0 * loss).backward()
  for name, t, g, e in zip(_LEAVES, leaves, gref, e_grads):
    assert t.grad is not None, name
    _frob(fwd + '+bwd', 'd' + name, t.grad, g, e)
  return [t.grad for t in leaves]


_CLIPS = ['abs_one', 'soft_asymmetric']
_EDGE_CASES = [(16, T) for T in (1, 15, 16, 17, 31, 32, 33, 48)] + [
    (32, T) for T in (33, 64, 65, 100)]


@pytest.mark.parametrize('tile,T', _EDGE_CASES,
                         ids=['tile%d-T%d' % c for c in _EDGE_CASES])
def test_tile_edges_match_float64(cuda, tile, T):
  case = 0
  for B in (1, 3):
    for A in (1, 9, 15, 16, 31):
      d = _inputs(T, B, A, 1, seed=1000 + 37 * T + 5 * A + B)
      grads = _check(cuda, d, _CLIPS[case % 2], tile)
      case += 1
      if A == 1:  # one action: softmax == 1, no policy gradient at all
        assert torch.count_nonzero(grads[1]) == 0
        assert torch.count_nonzero(grads[2]) == 0


def _carry_inputs(K=1, seed=2000):
  """T 40 under tile 16: tiles [24, 40), [8, 24), [0, 8).  Columns: done at
  step 23 / at step 24 / over all of [8, 24) / never.  At the steps on both
  sides of either tile edge the behaviour policy is made to dislike the
  action taken (rho >> 1) and the reward is large, so both clips bind."""
  T, B, A = 40, 4, 9
  done = torch.zeros(T, B, dtype=torch.bool)
  done[23, 0] = True
  done[24, 1] = True
  done[8:24, 2] = True
  d = _inputs(T, B, A, K, seed, done=done)
  for t in (7, 8, 23, 24):
    for b in range(B):
      d['beh'][t + 1, b, d['act'][t + 1, b]] -= 6.0
    d['rew'][t + 1] = torch.tensor([7.0, -6.0, 5.0, -8.0])
  return d


@pytest.mark.parametrize('clip', _CLIPS)
def test_carries_across_tiles_match_float64(cuda, clip):
  d = _carry_inputs()
  oracle = _oracle(d, clip)
  log_rhos = oracle[3]
  for t in (7, 8, 23, 24):
    assert (log_rhos[t] > 1.0).all()  # the rho clips bind on both sides
  assert not d['done'][1:, 3].any()
  _check(cuda, d, clip, 16, oracle=oracle)
  # the targets themselves, through the PopArt output with identity statistics
  _, _, aux = _run(cuda, d, clip, 16, task=torch.zeros(4, dtype=torch.int64),
                   mu=torch.zeros(1), nu=torch.ones(1))
  _close('learner_head_fwd_tiled', 'vs', aux['targets'], oracle[2], 1e-4, 1e-4)


@pytest.mark.parametrize('A', [32, 33, 47, 63])
def test_wide_heads_match_float64(cuda, A):
  d = _inputs(20, 3, A, 1, seed=3000 + A)
  _check(cuda, d, _CLIPS[A % 2], 16)


def _popart_stats(K, seed):
  g = torch.Generator().manual_seed(seed)
  mu = torch.randn(K, generator=g) * 3
  nu = mu * mu + torch.rand(K, generator=g) * 20 + 0.5
  return mu, nu


def test_wide_popart_heads_match_float64(cuda):
  """A + K = 64: the 64-wide forward image and the widest backward."""
  A, K, B = 40, 24, 3
  d = _inputs(20, B, A, K, seed=3100)
  mu, nu = _popart_stats(K, 3101)
  task = torch.tensor([23, 0, 11])
  grads = _check(cuda, d, 'abs_one', 16, task=task, mu=mu, nu=nu)
  unused = torch.ones(K, dtype=torch.bool)
  unused[task] = False
  assert torch.count_nonzero(grads[3].cpu()[:, unused]) == 0
  assert torch.count_nonzero(grads[4].cpu()[unused]) == 0


def test_popart_across_tiles_matches_float64(cuda):
  """K = 3, columns of tasks 0 and 2 over three tiles (the carry patterns):
  targets checked, the unused head 1 gets exactly zero gradient."""
  K = 3
  d = _carry_inputs(K=K, seed=3200)
  mu, nu = _popart_stats(K, 3201)
  task = torch.tensor([0, 2, 0, 2])
  grads = _check(cuda, d, 'abs_one', 16, task=task, mu=mu, nu=nu)
  assert torch.count_nonzero(grads[3].cpu()[:, 1]) == 0
  assert torch.count_nonzero(grads[4].cpu()[1]) == 0
  assert torch.count_nonzero(grads[3].cpu()[:, 0]) > 0
  assert torch.count_nonzero(grads[3].cpu()[:, 2]) > 0


@pytest.mark.parametrize('T,B,A', [(437, 2, 31), (1400, 2, 9)])
def test_past_the_untiled_limit_matches_float64(cuda, T, B, A):
  ops = _ops()
  assert T > ops.learner_head_max_unroll(A)
  tile = ops.learner_head_tile(A)
  assert 16 <= tile <= 1024 and tile % 16 == 0
  d = _inputs(T, B, A, 1, seed=4000 + T)
  _check(cuda, d, 'abs_one', 'auto', torch_bound=True)


def _raw_fwd(cuda, d, time_tile):
  """The forward binding itself -> (loss[4], dlogits, dvalues)."""
  from scalable_agent_amd.ops import heads as heads_mod
  ext = heads_mod.ext()
  args = [d[k].to(cuda).contiguous() for k in _LEAVES]
  args[3], args[4] = args[3].reshape(-1), args[4].reshape(-1)
  args += [d['beh'].to(cuda), d['act'].to(cuda), d['rew'].to(cuda),
           d['done'].to(cuda), heads_mod._ticket(cuda), _GAMMA, 0, 1.0, 1.0,
           _BC, _EC]
  if time_tile is None:
    return ext.learner_head_fwd(*args)
  return ext.learner_head_fwd_tiled(*args, time_tile=time_tile)


def test_same_answer_for_every_tile(cuda):
  d = _inputs(100, 3, 9, 1, seed=5000)
  oracle = _oracle(d, 'abs_one')
  for tile in (16, 48, 112, None):
    _check(cuda, d, 'abs_one', tile, oracle=oracle)
  for tile in (16, 48, 112):
    a = _raw_fwd(cuda, d, tile)
    b = _raw_fwd(cuda, d, tile)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
      assert torch.equal(x, y), tile


def test_ticket_rearmed_across_grids(cuda):
  """B = 5, 2, 7 back to back: each launch's last workgroup is found only
  when the launch before left the ticket at zero."""
  for B in (5, 2, 7):
    _check(cuda, _inputs(40, B, 9, 1, seed=6000 + B), 'abs_one', 16)


def test_graph_replay_is_bitwise_eager(cuda):
  ops = _ops()
  T, B, A, tile = 40, 3, 9, 16
  sets = [_inputs(T, B, A, 1, seed=7000 + i) for i in range(3)]
  names = _LEAVES + ('beh', 'act', 'rew', 'done')
  static = {k: sets[0][k].to(cuda) for k in names}
  leaves = [static[k].requires_grad_() for k in _LEAVES]

  def step():
    loss = ops.heads_vtrace_loss(
        *leaves, static['beh'], static['act'], static['rew'], static['done'],
        _GAMMA, 'abs_one', _BC, _EC, time_tile=tile)
    return (loss,) + torch.autograd.grad(loss, leaves)

  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side):
    step()
  torch.cuda.current_stream(cuda).wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    outs = step()
  for d in sets[1:]:
    with torch.no_grad():
      for k in names:
        static[k].copy_(d[k])
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    want = step()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
      assert torch.equal(g, w)
    _close('learner_head_fwd_tiled', 'graph loss', got[0],
           _oracle(d, 'abs_one')[0], 1e-4, 1e-3)


def test_refusals(cuda):
  ops = _ops()

  def call(A, T, tile):
    d = _inputs(T, 2, A, 1, seed=8000 + A)
    args = [d[k].to(cuda) for k in _LEAVES + ('beh', 'act', 'rew', 'done')]
    return ops.heads_vtrace_loss(*args, _GAMMA, 'abs_one', _BC, _EC,
                                 time_tile=tile)

  with pytest.raises(RuntimeError, match='multiple of 16'):
    call(9, 20, 20)
  with pytest.raises(RuntimeError, match='multiple of 16'):
    call(9, 20, 2048)
  with pytest.raises(RuntimeError, match='num_actions <= 63'):
    call(64, 20, 16)
  with pytest.raises(RuntimeError, match='num_actions <= 63'):
    ops.learner_head_tile(64)
  # 1024 steps x (2 x 31 + 9) words next to the 32 KB image: 324 KB
  with pytest.raises(RuntimeError, match='time_tile too large'):
    call(31, 20, 1024)
  with pytest.raises(ValueError):
    call(9, 20, 'widest')
  with pytest.raises(RuntimeError, match='unroll too long'):
    call(31, ops.learner_head_max_unroll(31) + 1, None)
  torch.cuda.synchronize()
  # the refused calls launched nothing: the next launch finds the ticket armed
  _check(cuda, _inputs(20, 2, 9, 1, seed=8100), 'abs_one', 16)
