"""The fused actor core step (csrc/kernels/actor_core.hip, ops.actor_core_step)
against a float64 oracle, the existing ops path (gemm_f32 -> lstm_fwd at T = 1
-> actor_heads_sample), a host Philox, captured graphs, the board epilogue,
and through Agent / InferenceModel / BoardServer; multi-head agents on both
cores.

Parity rule (tests/test_learner_parity_gpu.py): per output tensor the
max-abs error against the float64 oracle is <= max(2e-5, 1.5 * e_ops), e_ops
being the error of the existing path on the same inputs."""

import numpy as np
import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent

gpu = pytest.mark.gpu

M32 = np.uint64(0xFFFFFFFF)
SEED, OFFSET = 1234567890123, 7
ROWS = (1, 5, 16, 17, 40)
HEADS = ((3, 1), (9, 1), (9, 5), (32, 30))
CASES = [(R, A, Kv, instr) for R in ROWS for A, Kv in HEADS
         for instr in (False, True)]
TIE = 1e-4


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
  if keys.shape[1] == 1:
    return np.full(keys.shape[0], np.inf)
  s = np.sort(keys, -1)
  return s[:, -1] - s[:, -2]


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
  """CPU tensors of one case (deterministic) and its float64 oracle."""
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
  """The seeds of the cases: no row's two largest float64 oracle keys are
  closer than the tie band, so the sampler check below drops a row only for
  a kernel-side reason.  (Runs without a GPU.)"""
  for R, A, Kv, instr in CASES:
    case = _inputs(R, A, Kv, instr)
    keys = case['oracle']['logits'].numpy() + _gumbel(R, A)
    assert (_top2_gap(keys) >= TIE).all(), (R, A, Kv, instr)


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


_RUNS = {}


def _run(cuda, R, A, Kv, instr):
  """Fused and existing-path outputs of one case (computed once)."""
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
  # the existing path
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
def test_oracle_parity(cuda, R, A, Kv, instr):
  run = _run(cuda, R, A, Kv, instr)
  f = run['fused']
  assert f['action'].dtype == torch.int64 and f['action'].shape == (R,)
  assert f['logits'].shape == (R, A) and f['baseline'].shape == (R,)
  assert f['c2'].shape == (R, 256) and f['h2'].shape == (R, 256)
  _check_rule(f, run['ops'], _inputs(R, A, Kv, instr)['oracle'],
              'R%d A%d Kv%d instr%d' % (R, A, Kv, instr))


@gpu
@pytest.mark.parametrize('R,A,Kv,instr', CASES)
def test_sampler_matches_host_philox(cuda, R, A, Kv, instr):
  f = _run(cuda, R, A, Kv, instr)['fused']
  keys = f['logits'].double().numpy() + _gumbel(R, A)
  sure = _top2_gap(keys) >= TIE
  assert (~sure).sum() <= 1
  got = f['action'].numpy()
  assert got.min() >= 0 and got.max() < A
  assert (got[sure] == keys.argmax(-1)[sure]).all()
  # equal logits -> the action actor_heads_sample draws
  o = _run(cuda, R, A, Kv, instr)['ops']
  same = (o['logits'] == f['logits']).all(-1).numpy()
  assert (o['action'].numpy()[same] == got[same]).all()


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
def test_same_offset_same_actions_next_offset_differs(cuda):
  ops, args = _dev_case(cuda, 40, 9, 1, False)
  stream = ops.PhiloxStream(SEED)
  outs = []
  for off in (OFFSET, OFFSET, OFFSET + 1):
    stream.offset = off
    outs.append(ops.actor_core_step(*args, stream))
  for a, b in zip(outs[0], outs[1]):  # two eager launches: bitwise equal
    assert torch.equal(a, b)
  assert not torch.equal(outs[0][0], outs[2][0])
  for a, b in zip(outs[0][1:], outs[2][1:]):
    assert torch.equal(a, b)


@gpu
def test_graph_replay_matches_eager_and_rearms(cuda):
  R = 17
  ops, args = _dev_case(cuda, R, 9, 5, True)
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
def test_board_epilogue_in_the_step(cuda):
  from scalable_agent_amd.ops.actor_core import BoardEpilogue
  from scalable_agent_amd.runtime.inference_board import InferenceBoard
  S, M, A = 2, 20, 9
  R = S * M
  ops, args = _dev_case(cuda, R, A, 1, False)
  board = InferenceBoard(S, M, (8, 8, 3), A)
  offs = [o for _, _, _, o, _ in board.out_fields]
  mask = torch.zeros(R, 1, device=cuda)
  mask[:M + M // 2] = 1.0  # one and a half slots
  c0, h0 = args[2], args[3]
  stream = ops.PhiloxStream(SEED)

  def step(c, h, epilogue):
    stream.offset = OFFSET
    a = list(args)
    a[2], a[3] = c, h
    return ops.actor_core_step(*a, stream, epilogue=epilogue)

  # A: the step, then the existing epilogue launch
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


# ---- through the agent ------------------------------------------------------
SHAPE = (72, 96, 3)


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


def _model(cuda, core, heads=1, shape=SHAPE):
  agent = Agent(9, torso='deep', frame_shape=shape, seed=1, backend='hip',
                num_value_heads=heads, actor_core=core)
  return inference.InferenceModel(agent, cuda, use_instruction=False, seed=3)


def _step_inputs(cuda, B, shape=SHAPE):
  g = torch.Generator().manual_seed(4)
  frame = torch.randint(0, 255, (B,) + shape, generator=g, dtype=torch.uint8)
  reward = 2.0 * torch.randn(B, generator=g)
  done = torch.arange(B) % 4 == 2
  last = torch.randint(0, 9, (B,), generator=g)
  c, h = torch.randn(B, 256, generator=g), torch.randn(B, 256, generator=g)
  ids = torch.zeros(B, 16, dtype=torch.int64)
  ln = torch.zeros(B, dtype=torch.int64)
  return [t.to(cuda) for t in (last, reward, done, frame, ids, ln, c, h)]


def _step_device(model, ins):
  with model._lock, torch.cuda.stream(model.stream):
    outs = model.step_device(*ins, has_instr=False)
    model.stream.synchronize()
  return dict(zip(('action', 'logits', 'baseline', 'c2', 'h2'),
                  [o.cpu() for o in outs]))


@gpu
def test_step_device_fused_matches_ops(cuda):
  _ops()
  fused, plain = _model(cuda, 'fused'), _model(cuda, 'ops')
  assert fused.actor_core == 'fused' and plain.actor_core == 'ops'
  assert fused.agent._inference_cache.get('wpk') is not None
  assert 'wpk' not in plain.agent._inference_cache
  ins = _step_inputs(cuda, 12)
  f, o = _step_device(fused, ins), _step_device(plain, ins)
  last, reward, done, frame, _, _, c, h = ins
  with torch.no_grad():
    feats = plain.agent.conv_features(frame)
    assert torch.equal(feats, fused.agent.conv_features(frame))
  oracle = _agent_oracle(plain.agent, feats, reward, last, done, c, h)
  _check_rule(f, o, oracle, 'step_device')
  assert int(f['action'].min()) >= 0 and int(f['action'].max()) < 9


@gpu
def test_board_server_fused_matches_ops(cuda):
  from scalable_agent_amd.runtime import native
  from scalable_agent_amd.runtime.inference_board import (
      REQUEST, RESPONSE, BoardClient, BoardServer, InferenceBoard)
  _ops()
  shape = (24, 32, 3)
  g = torch.Generator().manual_seed(8)
  c0, h0 = torch.randn(12, 256, generator=g), torch.randn(12, 256, generator=g)
  res = {}
  for core in ('fused', 'ops'):
    board = InferenceBoard(3, 4, shape, 9)
    server = BoardServer(_model(cuda, core, shape=shape), board,
                         use_graph=True)
    server.prepare(has_instr=False)
    server.c.copy_(c0)
    server.h.copy_(h0)
    rng = np.random.RandomState(5)
    cl = BoardClient(board, 1, 3)
    cl.inputs['frame'][:] = rng.randint(0, 256, cl.inputs['frame'].shape)
    cl.inputs['reward'][:] = 2.0 * rng.randn(3)
    cl.inputs['last_action'][:] = rng.randint(0, 9, 3)
    cl.inputs['done'][:] = [False, True, False]
    native.atomic_store_u32(board.state_addr(1), REQUEST)
    assert server.serve_once(timeout_ms=10)
    assert board.state(1) == RESPONSE
    action, logits, baseline, c, h = [torch.from_numpy(x.copy())
                                      for x in cl.wait()]
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
  assert int(res['fused']['action'].min()) >= 0
  assert int(res['fused']['action'].max()) < 9


@gpu
@pytest.mark.parametrize('core,heads', [('ops', 5), ('fused', 30)])
def test_multi_head_actor_inference(cuda, core, heads):
  _ops()
  model = _model(cuda, core, heads=heads)
  assert model.actor_core == core
  f = _step_device(model, _step_inputs(cuda, 12))
  with torch.no_grad():
    want = model.agent.heads(f['h2'].to(cuda).unsqueeze(0))[1][0].cpu()
  assert f['baseline'].shape == (12,)
  assert float((f['baseline'] - want).abs().max()) <= 1e-4
  assert int(f['action'].min()) >= 0 and int(f['action'].max()) < 9
