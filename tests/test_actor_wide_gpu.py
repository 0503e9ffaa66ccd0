"""Actor inference for 33..63 actions: the 64-wide instances of the heads +
Gumbel-max sampler (csrc/kernels/actor_io.hip) and of the fused actor core's
finisher (csrc/kernels/actor_core.hip), both from csrc/kernels/head_sample.h,
and the torch sampler past 63 actions.

Conventions of tests/test_actor_gpu.py and tests/test_actor_core_gpu.py (the
helpers are copies): the host Philox4x32-10, a float64 oracle, the tie band
TIE = 1e-4 and the parity rule - per output tensor the max-abs error against
the float64 oracle is <= max(2e-5, 1.5 * e_ops), e_ops being the error of the
ops path (gemm_f32 -> lstm_fwd at T = 1 -> actor_heads_sample) on the same
inputs.  The inputs are made on the CPU, so the seeds' oracle keys are
checked without a GPU (test_oracle_keys_leave_out_no_row) and the GPU
comparisons demand equal actions on EVERY row."""

import statistics

import numpy as np
import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent

gpu = pytest.mark.gpu

M32 = np.uint64(0xFFFFFFFF)
SEED, OFFSET = 1234567890123, 7
TIE = 1e-4

# ---- the sampler's cases: (B, A) -> seed of the inputs
SAMPLER = {(1, 33): 134, (5, 48): 548, (37, 63): 3763, (1024, 40): 102440}
SAMPLER_OFFSET = 5
COUNTER_CASE, COUNTER_SEED = (63, 40), 5  # device counter stream: offsets 0, 1

# ---- the fused core's cases
ROWS = (1, 17, 40)
HEADS = ((33, 1), (48, 5), (63, 30))
CASES = [(R, A, Kv, instr) for R in ROWS for A, Kv in HEADS
         for instr in (False, True)]


def _philox_u(rows, lanes, offset, seed):
  """Host Philox4x32-10, first output word -> uniform in (0,1) (float64);
  the algorithm of tests/test_actor_gpu.py."""
  c0 = rows.astype(np.uint64)
  c1 = lanes.astype(np.uint64)
  c2 = np.full_like(c0, np.uint64(offset & 0xFFFFFFFF))
  c3 = np.full_like(c0, np.uint64(offset >> 32))
  k0 = np.uint64(seed & 0xFFFFFFFF)
  k1 = np.uint64(seed >> 32)
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c0
    p1 = np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32,
                      (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32)
    k0 = (k0 + np.uint64(0x9E3779B9)) & M32
    k1 = (k1 + np.uint64(0xBB67AE85)) & M32
  return ((c0 >> np.uint64(8)).astype(np.float64) + 0.5) / float(1 << 24)


def _gumbel(R, A, offset=OFFSET, seed=SEED):
  u = _philox_u(np.repeat(np.arange(R), A), np.tile(np.arange(A), R), offset,
                seed).reshape(R, A)
  return -np.log(-np.log(u))


def _top2_gap(keys):
  s = np.sort(keys, -1)
  return s[:, -1] - s[:, -2]


_SAMPLER_INPUTS = {}


def _sampler_inputs(B, A):
  """CPU inputs of one sampler case (the input scaling of
  test_actor_head_sample_matches_reference) and its float64 oracle."""
  key = (B, A)
  if key in _SAMPLER_INPUTS:
    return _SAMPLER_INPUTS[key]
  seed = SAMPLER[key] if key in SAMPLER else 1000 * B + A
  g = torch.Generator().manual_seed(seed)
  h = torch.randn(B, 256, generator=g)
  wp = torch.randn(256, A, generator=g) * 0.1
  bp = torch.randn(A, generator=g)
  wb = torch.randn(256, 1, generator=g) * 0.1
  bb = torch.randn(1, generator=g)
  logits = h.double() @ wp.double() + bp.double()
  base = (h.double() @ wb.double() + bb.double()).squeeze(-1)
  out = dict(args=(h, wp, bp, wb, bb), logits=logits, baseline=base)
  _SAMPLER_INPUTS[key] = out
  return out


def _core_oracle(x, kernel, bias, done, c, h):
  """float64 LSTMBlockCell step with done-reset: x [R, f] core input."""
  f = x.shape[1]
  keep = (~done).double().unsqueeze(-1)
  gates = x @ kernel[:f] + bias + (keep * h) @ kernel[-256:]
  i, g, fg, o = gates.chunk(4, -1)
  c2 = torch.sigmoid(fg + 1.0) * keep * c + torch.sigmoid(i) * torch.tanh(g)
  return c2, torch.sigmoid(o) * torch.tanh(c2)


_INPUTS = {}


def _inputs(R, A, Kv, instr):
  """CPU tensors of one fused-core case (deterministic) and its float64
  oracle.  A = 63 with instruction columns is K = 384 = actor_core_max_k():
  every wave runs all 20 MFMA steps, none of them padding."""
  key = (R, A, Kv, instr)
  if key in _INPUTS:
    return _INPUTS[key]
  seed = 100 + 1000 * R + 10 * A + int(instr)
  g = torch.Generator().manual_seed(seed)
  agent = Agent(A, torso='shallow', frame_shape=(16, 16, 3), seed=seed,
                num_value_heads=Kv)
  for p in (agent.lstm_bias, agent.policy_b, agent.baseline_b):
    p.data.copy_(0.5 * torch.randn(p.shape, generator=g))
  f_in = 257 + A + 64
  K = (f_in + 15) // 16 * 16 if instr else (257 + A + 15) // 16 * 16
  h_aug = torch.zeros(R, K)
  h_aug[:, :256] = torch.relu(torch.randn(R, 256, generator=g))
  h_aug[:, 256] = (3.0 * torch.randn(R, generator=g)).clamp(-1, 1)
  last = torch.randint(0, A, (R,), generator=g)
  h_aug[torch.arange(R), 257 + last] = 1.0
  if instr:
    h_aug[:, 257 + A:f_in] = torch.randn(R, 64, generator=g)
  done = torch.arange(R) % 3 == 1  # both values once R >= 2
  if R == 1:
    done[0] = True
  c = torch.randn(R, 256, generator=g)
  h = torch.randn(R, 256, generator=g)
  kernel = agent.lstm_kernel.detach()
  c2, h2 = _core_oracle(h_aug[:, :f_in if instr else 257 + A].double(),
                        kernel.double()[:f_in + 256], agent.lstm_bias.detach().double(),
                        done, c.double(), h.double())
  logits = h2 @ agent.policy_w.detach().double() + agent.policy_b.detach().double()
  base = h2 @ agent.baseline_w.detach().double()[:, 0] + float(agent.baseline_b.detach()[0])
  out = dict(agent=agent, h_aug=h_aug, done=done, c=c, h=h, K=K, f_in=f_in,
             oracle=dict(c2=c2, h2=h2, logits=logits, baseline=base))
  _INPUTS[key] = out
  return out


def test_oracle_keys_leave_out_no_row():
  """The seeds of every sampler case: no row's two largest float64 oracle
  keys (logits + Gumbel) are closer than the tie band, so the GPU tests
  below leave out no row.  (Runs without a GPU.)"""
  for B, A in SAMPLER:
    logits = _sampler_inputs(B, A)['logits'].numpy()
    keys = logits + _gumbel(B, A, SAMPLER_OFFSET)
    assert (_top2_gap(keys) >= TIE).all(), (B, A)
    # ... and the next offset draws another action in some row (B = 1 too)
    nxt = logits + _gumbel(B, A, SAMPLER_OFFSET + 1)
    assert (_top2_gap(nxt) >= TIE).all(), (B, A)
    assert (nxt.argmax(-1) != keys.argmax(-1)).any(), (B, A)
  B, A = COUNTER_CASE
  for offset in (0, 1):
    keys = _sampler_inputs(B, A)['logits'].numpy() + _gumbel(
        B, A, offset, COUNTER_SEED)
    assert (_top2_gap(keys) >= TIE).all(), (B, A, offset)
  for R, A, Kv, instr in CASES:
    case = _inputs(R, A, Kv, instr)
    keys = case['oracle']['logits'].numpy() + _gumbel(R, A)
    assert (_top2_gap(keys) >= TIE).all(), (R, A, Kv, instr)
  assert _inputs(1, 63, 30, True)['K'] == 384


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


# ---- 1. actor_heads_sample -------------------------------------------------
@gpu
@pytest.mark.parametrize('B,A', list(SAMPLER))
def test_actor_head_sample_wide(cuda, B, A):
  ops = _ops()
  case = _sampler_inputs(B, A)
  args = [t.to(cuda) for t in case['args']]
  stream = ops.PhiloxStream(SEED)
  stream.offset = SAMPLER_OFFSET
  action, logits, baseline = ops.actor_heads_sample(*args, stream)
  assert stream.offset == SAMPLER_OFFSET + 1
  assert logits.shape == (B, A) and baseline.shape == (B,)
  torch.testing.assert_close(logits.double().cpu(), case['logits'], atol=1e-4,
                             rtol=1e-4)
  torch.testing.assert_close(baseline.double().cpu(), case['baseline'],
                             atol=1e-4, rtol=1e-4)
  keys = case['logits'].numpy() + _gumbel(B, A, SAMPLER_OFFSET)
  got = action.cpu().numpy()
  assert action.dtype == torch.int64 and got.min() >= 0 and got.max() < A
  assert (got == keys.argmax(-1)).all()
  # same (seed, offset) -> same sample; next offset -> a different draw
  stream.offset = SAMPLER_OFFSET
  a2, l2, b2 = ops.actor_heads_sample(*args, stream)
  assert torch.equal(a2, action) and torch.equal(l2, logits)
  assert torch.equal(b2, baseline)
  a3, _, _ = ops.actor_heads_sample(*args, stream)
  keys3 = case['logits'].numpy() + _gumbel(B, A, SAMPLER_OFFSET + 1)
  assert (a3.cpu().numpy() == keys3.argmax(-1)).all()
  assert not torch.equal(a3, action)


@gpu
def test_actor_head_sample_action_limit(cuda):
  ops = _ops()
  h, _, _, wb, bb = [t.to(cuda) for t in _sampler_inputs(5, 48)['args']]
  wp = torch.zeros(256, 64, device=cuda)
  bp = torch.zeros(64, device=cuda)
  with pytest.raises(RuntimeError, match='num_actions <= 63'):
    ops.actor_heads_sample(h, wp, bp, wb, bb, ops.PhiloxStream(1))


# ---- 2. distribution ---------------------------------------------------------
def _chi2_upper(dof, p):
  """Upper-p quantile of chi-square(dof), Wilson-Hilferty."""
  z = statistics.NormalDist().inv_cdf(1.0 - p)
  return dof * (1.0 - 2.0 / (9.0 * dof) + z * (2.0 / (9.0 * dof)) ** 0.5) ** 3


@gpu
def test_actor_head_sample_distribution_wide(cuda):
  ops = _ops()
  A, B = 48, 8192
  # actions 32..47 carry 67 % of the mass
  logits_row = torch.linspace(-1.5, 1.5, A, device=cuda)
  # h = e_0 and W row 0 = the logits: every row has the same distribution
  h = torch.zeros(B, 256, device=cuda)
  h[:, 0] = 1.0
  wp = torch.zeros(256, A, device=cuda)
  wp[0] = logits_row
  bp = torch.zeros(A, device=cuda)
  wb = torch.zeros(256, 1, device=cuda)
  bb = torch.zeros(1, device=cuda)
  stream = ops.PhiloxStream(7)
  counts = torch.zeros(A, device=cuda)
  for _ in range(8):
    a, lg, _ = ops.actor_heads_sample(h, wp, bp, wb, bb, stream)
    counts += torch.bincount(a, minlength=A).float()
  assert torch.equal(lg[B - 1], logits_row)
  n = float(counts.sum())
  p = torch.softmax(logits_row.double(), 0).cpu().numpy()
  obs = counts.double().cpu().numpy()
  chi2 = float((((obs - n * p) ** 2) / (n * p)).sum())
  bound = _chi2_upper(A - 1, 1e-4)
  print('chi2 %.2f bound %.2f upper-half share %.3f (p %.3f)' % (
      chi2, bound, obs[32:].sum() / n, p[32:].sum()))
  assert n == 8 * B and chi2 < bound, (chi2, bound)


# ---- 3. device counter stream --------------------------------------------------
@gpu
def test_device_counter_stream_wide(cuda):
  ops = _ops()
  B, A = COUNTER_CASE  # a partial last workgroup
  case = _sampler_inputs(B, A)
  args = [t.to(cuda) for t in case['args']]
  s = ops.PhiloxStream(COUNTER_SEED, device=cuda)
  a1, _, _ = ops.actor_heads_sample(*args, s)
  a2, _, _ = ops.actor_heads_sample(*args, s)
  # the kernel advanced its own counter: offset 2, wave count re-armed
  assert s.device_offset == 2 and int(s.counter[1].item()) == 0
  assert s.offset == 0
  host = ops.PhiloxStream(COUNTER_SEED)
  b1, _, _ = ops.actor_heads_sample(*args, host)
  b2, _, _ = ops.actor_heads_sample(*args, host)
  assert torch.equal(a1, b1) and torch.equal(a2, b2)
  assert not torch.equal(a1, a2)
  for got, offset in ((a1, 0), (a2, 1)):
    keys = case['logits'].numpy() + _gumbel(B, A, offset, COUNTER_SEED)
    assert (got.cpu().numpy() == keys.argmax(-1)).all(), offset


# ---- 4. the fused core -----------------------------------------------------------
_RUNS = {}


def _run(cuda, R, A, Kv, instr):
  """Fused and ops-path outputs of one case (computed once)."""
  key = (R, A, Kv, instr)
  if key in _RUNS:
    return _RUNS[key]
  ops = _ops()
  C = ops.ext()
  case = _inputs(R, A, Kv, instr)
  ag = case['agent']
  d = lambda t: t.detach().to(cuda).contiguous()
  kernel, bias = d(ag.lstm_kernel), d(ag.lstm_bias)
  wp, bp, wb, bb = d(ag.policy_w), d(ag.policy_b), d(ag.baseline_w), d(ag.baseline_b)
  h_aug, done, c, h = d(case['h_aug']), d(case['done']), d(case['c']), d(case['h'])
  wpk = ops.actor_core_pack(kernel, A)
  stream = ops.PhiloxStream(SEED)
  stream.offset = OFFSET
  fused = ops.actor_core_step(h_aug, done, c, h, wpk, bias, wp, bp, wb, bb, stream)
  assert stream.offset == OFFSET + 1
  # the ops path
  K, f_in = case['K'], case['f_in']
  xw = torch.empty(R, 1024, device=cuda)
  C.gemm_f32(h_aug, kernel[:K], False, False, xw, bias=bias)
  mode = C.lstm_mode(256, R, 1, True)
  hs, cs, _, _, _ = C.lstm_fwd(xw.view(1, R, 1024), done.view(1, R).view(torch.uint8),
                               c, h, kernel[f_in:], mode, None)
  stream.offset = OFFSET
  a_o, l_o, b_o = ops.actor_heads_sample(hs[0], wp, bp, wb[:, :1].contiguous(),
                                         bb[:1].contiguous(), stream)
  torch.cuda.synchronize()
  names = ('action', 'logits', 'baseline', 'c2', 'h2')
  out = dict(fused=dict(zip(names, [t.cpu() for t in fused])),
             ops=dict(action=a_o.cpu(), logits=l_o.cpu(), baseline=b_o.cpu(),
                      c2=cs[0].cpu(), h2=hs[0].cpu()))
  _RUNS[key] = out
  return out


def _check_rule(fused, ops_out, oracle, what):
  for name in ('c2', 'h2', 'logits', 'baseline'):
    want = oracle[name]
    e_ops = float((ops_out[name].double() - want).abs().max())
    e_fused = float((fused[name].double() - want).abs().max())
    bound = max(2e-5, 1.5 * e_ops)
    print('%s %s: e_fused %.3g e_ops %.3g bound %.3g' % (what, name, e_fused,
                                                       e_ops, bound))
    assert e_fused <= bound, (what, name, e_fused, e_ops)


@gpu
@pytest.mark.parametrize('R,A,Kv,instr', CASES)
def test_fused_core_wide(cuda, R, A, Kv, instr):
  run = _run(cuda, R, A, Kv, instr)
  f, o = run['fused'], run['ops']
  assert f['action'].dtype == torch.int64 and f['action'].shape == (R,)
  assert f['logits'].shape == (R, A) and f['baseline'].shape == (R,)
  assert f['c2'].shape == (R, 256) and f['h2'].shape == (R, 256)
  oracle = _inputs(R, A, Kv, instr)['oracle']
  _check_rule(f, o, oracle, 'R%d A%d Kv%d instr%d' % (R, A, Kv, instr))
  want = (oracle['logits'].numpy() + _gumbel(R, A)).argmax(-1)
  for path in (f, o):
    got = path['action'].numpy()
    assert got.min() >= 0 and got.max() < A
    assert (got == want).all()


def _dev_case(cuda, R, A, Kv, instr):
  ops = _ops()
  case = _inputs(R, A, Kv, instr)
  ag = case['agent']
  d = lambda t: t.detach().to(cuda).contiguous()
  args = [d(case['h_aug']), d(case['done']), d(case['c']), d(case['h']),
          ops.actor_core_pack(d(ag.lstm_kernel), A), d(ag.lstm_bias),
          d(ag.policy_w), d(ag.policy_b), d(ag.baseline_w), d(ag.baseline_b)]
  return ops, args


@gpu
def test_fused_core_wide_graph_replay(cuda):
  R = 17
  ops, args = _dev_case(cuda, R, 63, 30, True)
  tk = torch.zeros(8, dtype=torch.int32, device=cuda)
  eager_stream = ops.PhiloxStream(SEED, device=cuda)
  eager = [[t.clone() for t in ops.actor_core_step(*args, eager_stream,
                                                   ticket_words=tk)]
           for _ in range(3)]
  assert eager_stream.device_offset == 3
  assert not torch.equal(eager[0][0], eager[1][0])
  stream = ops.PhiloxStream(SEED, device=cuda)
  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side):
    ops.actor_core_step(*args, stream, ticket_words=tk)  # warm-up
    side.synchronize()
    stream.manual_seed(SEED)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      outs = ops.actor_core_step(*args, stream, ticket_words=tk)
    for n in range(3):
      g.replay()
      side.synchronize()
      for a, b in zip(outs, eager[n]):
        assert torch.equal(a, b), n
  assert stream.device_offset == 3
  assert int(stream.counter[1].item()) == 0
  assert int(tk.abs().sum().item()) == 0


def _row_bytes(board, block, r):
  s, m = divmod(r, board.M)
  blk = block[s * board.slot_out_bytes:(s + 1) * board.slot_out_bytes]
  out = []
  for _, _, _, o, nb in board.out_fields:
    per = nb // board.M
    out.append(blk[o + m * per:o + (m + 1) * per])
  return torch.cat(out)


@gpu
def test_fused_core_wide_board_epilogue(cuda):
  """A = 63: the logits field is 252 bytes per row, no 16-byte multiple."""
  from scalable_agent_amd.ops.actor_core import BoardEpilogue
  from scalable_agent_amd.runtime.inference_board import InferenceBoard
  S, M, A = 2, 20, 63
  R = S * M
  ops, args = _dev_case(cuda, R, A, 30, False)
  board = InferenceBoard(S, M, (8, 8, 3), A)
  offs = [o for _, _, _, o, _ in board.out_fields]
  assert board.out_fields[1][4] == M * 252
  mask = torch.zeros(R, 1, device=cuda)
  mask[:M + M // 2] = 1.0  # one and a half slots
  c0, h0 = args[2], args[3]
  stream = ops.PhiloxStream(SEED)

  def step(c, h, epilogue):
    stream.offset = OFFSET
    a = list(args)
    a[2], a[3] = c, h
    return ops.actor_core_step(*a, stream, epilogue=epilogue)

  # A: the step, then the separate epilogue launch
  c_a, h_a = c0.clone(), h0.clone()
  out_a = torch.full((board.out_bytes,), 0x5A, dtype=torch.uint8, device=cuda)
  action, logits, baseline, c2, h2 = step(c_a, h_a, None)
  ops.ext().board_epilogue([action, logits, baseline, c2, h2], offs, out_a, M,
                           board.slot_out_bytes, mask, c2, h2, c_a, h_a)
  # B: one launch; B2: masked rows only, into an address
  c_b, h_b = c0.clone(), h0.clone()
  out_b = torch.full_like(out_a, 0x5A)
  res_b = step(c_b, h_b, BoardEpilogue(mask, offs, M, board.slot_out_bytes,
                                       out_b, 0))
  c_b2, h_b2 = c0.clone(), h0.clone()
  out_b2 = torch.full_like(out_a, 0x5A)
  step(c_b2, h_b2, BoardEpilogue(mask, offs, M, board.slot_out_bytes, out_b2,
                                 out_b2.data_ptr()))
  torch.cuda.synchronize()
  for a, b in zip((action, logits, baseline, c2, h2), res_b):
    assert torch.equal(a, b)
  for c, h in ((c_b, h_b), (c_b2, h_b2)):
    assert torch.equal(c, c_a) and torch.equal(h, h_a)
  n = M + M // 2
  assert torch.equal(c_a[:n], c2[:n]) and torch.equal(c_a[n:], c0[n:])
  assert torch.equal(h_a[:n], h2[:n]) and torch.equal(h_a[n:], h0[n:])
  assert torch.equal(out_a, out_b)  # every row packed, pad bytes untouched
  for r in range(R):
    want = _row_bytes(board, out_a, r)
    got = _row_bytes(board, out_b2, r)
    if r < n:
      assert torch.equal(got, want), r
    else:
      assert bool((got == 0x5A).all()), r
  board.close()


# ---- 5. through the public interface ----------------------------------------------
SHAPE = (16, 16, 3)
A_PUB = 40


def _model(cuda, core, num_actions=A_PUB, backend='hip'):
  agent = Agent(num_actions, torso='shallow', frame_shape=SHAPE, seed=1,
                backend=backend, actor_core=core)
  return inference.InferenceModel(agent, cuda, use_instruction=False, seed=3)


def _infer_inputs(B, num_actions):
  rng = np.random.RandomState(4)
  return (rng.randint(0, num_actions, B).astype(np.int64),
          (2.0 * rng.randn(B)).astype(np.float32), np.arange(B) % 4 == 2,
          rng.randint(0, 256, (B,) + SHAPE).astype(np.uint8),
          np.zeros((B, 16), np.int64), np.zeros(B, np.int64),
          rng.randn(B, 256).astype(np.float32),
          rng.randn(B, 256).astype(np.float32))


@gpu
@pytest.mark.parametrize('core', ['ops', 'fused'])
def test_inference_model_40_actions(cuda, core):
  """On the parent commit: TypeError, multinomial(): argument 'generator'
  must be torch.Generator, not PhiloxStream."""
  _ops()
  from scalable_agent_amd.structs import StepOutput
  model = _model(cuda, core)
  assert model.actor_core == core
  B = 5
  ins = _infer_inputs(B, A_PUB)
  action, logits, baseline, c2, h2 = model.infer(*ins)
  assert action.shape == (B,) and action.dtype == np.int64
  assert action.min() >= 0 and action.max() < A_PUB
  assert logits.shape == (B, A_PUB)
  # the torch-backend agent with the same weights
  ref = Agent(A_PUB, torso='shallow', frame_shape=SHAPE, seed=1).to(cuda)
  for p, q in zip(ref.parameters(), model.agent.parameters()):
    assert torch.equal(p, q)
  t = [torch.from_numpy(np.ascontiguousarray(x)).to(cuda) for x in ins]
  with torch.no_grad():
    out, (rc, rh) = ref.step(
        t[0], StepOutput(t[1], None, t[2], (t[3], None)), (t[6], t[7]),
        generator=torch.Generator(cuda).manual_seed(0))
  d = lambda x: torch.from_numpy(x).to(cuda)
  torch.testing.assert_close(d(logits), out.policy_logits, atol=1e-4, rtol=1e-4)
  torch.testing.assert_close(d(baseline), out.baseline, atol=1e-4, rtol=1e-4)
  torch.testing.assert_close(d(h2), rh)
  torch.testing.assert_close(d(c2), rc)


def _agent_oracle(agent, feats, reward, last, done, c, h):
  """float64 oracle of everything after the (shared) torso features."""
  dd = lambda t: t.detach().double()
  A = agent.num_actions
  x = torch.relu(dd(feats) @ dd(agent.linear_w) + dd(agent.linear_b))
  one_hot = (last.view(-1, 1) == torch.arange(A, device=last.device)).double()
  x = torch.cat([x, dd(reward).clamp(-1, 1).view(-1, 1), one_hot], 1)
  c2, h2 = _core_oracle(x, dd(agent.lstm_kernel), dd(agent.lstm_bias), done,
                        dd(c), dd(h))
  logits = h2 @ dd(agent.policy_w) + dd(agent.policy_b)
  base = h2 @ dd(agent.baseline_w)[:, 0] + dd(agent.baseline_b)[0]
  return dict(c2=c2.cpu(), h2=h2.cpu(), logits=logits.cpu(), baseline=base.cpu())


@gpu
def test_board_server_40_actions(cuda):
  from scalable_agent_amd.runtime import native
  from scalable_agent_amd.runtime.inference_board import (
      REQUEST, RESPONSE, BoardClient, BoardServer, InferenceBoard)
  _ops()
  g = torch.Generator().manual_seed(8)
  c0, h0 = torch.randn(12, 256, generator=g), torch.randn(12, 256, generator=g)
  res = {}
  for core in ('fused', 'ops'):
    board = InferenceBoard(3, 4, SHAPE, A_PUB)
    server = BoardServer(_model(cuda, core), board, use_graph=True)
    assert server.model.actor_core == core
    server.prepare(has_instr=False)
    server.c.copy_(c0)
    server.h.copy_(h0)
    rng = np.random.RandomState(5)
    cl = BoardClient(board, 1, 3)
    cl.inputs['frame'][:] = rng.randint(0, 256, cl.inputs['frame'].shape)
    cl.inputs['reward'][:] = 2.0 * rng.randn(3)
    cl.inputs['last_action'][:] = rng.randint(0, A_PUB, 3)
    cl.inputs['done'][:] = [False, True, False]
    native.atomic_store_u32(board.state_addr(1), REQUEST)
    assert server.serve_once(timeout_ms=10)
    assert board.state(1) == RESPONSE
    action, logits, baseline, c, h = [torch.from_numpy(x.copy())
                                      for x in cl.wait()]
    assert logits.shape == (3, A_PUB)
    res[core] = dict(action=action, logits=logits, baseline=baseline, c2=c,
                     h2=h)
    st_c, st_h = server.c.cpu(), server.h.cpu()
    # rows 4..6 asked; every other row keeps its state bitwise
    keep = [r for r in range(12) if not 4 <= r < 7]
    assert torch.equal(st_c[keep], c0[keep]) and torch.equal(st_h[keep], h0[keep])
    assert torch.equal(st_c[4:7], c) and torch.equal(st_h[4:7], h)
    if core == 'ops':
      ins = [torch.from_numpy(np.ascontiguousarray(cl.inputs[k])).to(cuda)
             for k in ('last_action', 'reward', 'done', 'frame')]
      with torch.no_grad():
        feats = server.model.agent.conv_features(ins[3])
      oracle = _agent_oracle(server.model.agent, feats, ins[1], ins[0], ins[2],
                             c0[4:7].to(cuda), h0[4:7].to(cuda))
    board.close()
  _check_rule(res['fused'], res['ops'], oracle, 'board')
  for core in res:
    assert int(res[core]['action'].min()) >= 0
    assert int(res[core]['action'].max()) < A_PUB


# ---- 6. past the limit --------------------------------------------------------------
@gpu
def test_past_the_limit_samples_with_torch(cuda):
  from scalable_agent_amd.ops.heads import ACTOR_MAX_ACTIONS, PhiloxStream
  from scalable_agent_amd.runtime.inference_board import (BoardServer,
                                                          InferenceBoard)
  _ops()
  assert ACTOR_MAX_ACTIONS == 63
  assert isinstance(_model(cuda, 'ops', 63)._gen, PhiloxStream)
  model = _model(cuda, 'ops', 70)
  assert isinstance(model._gen, torch.Generator)
  assert model.actor_core == 'ops'
  action, logits, _, _, _ = model.infer(*_infer_inputs(5, 70))
  assert logits.shape == (5, 70)
  assert action.min() >= 0 and action.max() < 70
  board = InferenceBoard(3, 4, SHAPE, 70)
  server = BoardServer(model, board)
  assert not server._native_ok()
  board.close()
