"""The bf16 MFMA fused actor core step (csrc/kernels/actor_core_bf16.hip,
ops.actor_core_step(dtype=torch.bfloat16)): exact and random cases against the
float64 one-step oracle of tests/_actor_core_bf16_oracle.py, the heads and the
sample against actor_heads_sample and a host Philox, the board epilogue, graph
replay, accuracy against the unrounded step, and through Agent /
InferenceModel / BoardServer."""

import numpy as np
import pytest
import torch

from scalable_agent_amd import inference
from scalable_agent_amd.models import Agent
from tests import _actor_core_bf16_oracle as O
from tests.test_actor_core_gpu import (_gumbel, _row_bytes, _step_device,
                                       _step_inputs, _top2_gap, TIE)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SEED, OFFSET = 1234567890123, 7
# (R, A, Kv, instr): every R in {1, 15, 16, 17, 76}, every A in {9, 31, 32,
# 33, 63}, Kv in {1, 30}, both instr; A = 31 (K = 288 = 9 x 32) and A = 32
# (K = 289) with done rows (every case with R >= 2 has some)
CASES = [(1, 9, 1, False), (15, 31, 1, False), (16, 32, 30, False),
         (17, 33, 1, True), (76, 63, 30, True), (76, 31, 30, True),
         (17, 32, 1, True), (15, 63, 1, False), (16, 9, 30, True)]
SENTINEL = -12345.0
PAD_ROWS = 3


def _ops():
  from scalable_agent_amd import ops
  ops.load()
  return ops


def _k(A, instr):
  return 257 + A + (64 if instr else 0)


def _done(R):
  done = torch.arange(R) % 3 == 1
  if R == 1:
    done[0] = True
  return done


def _assert_info(ops, R, A, instr):
  K = _k(A, instr)
  info = ops.actor_core.actor_core_bf16_info(R, K, A)
  kpad = (K + 31) // 32 * 32
  assert info['kpad'] == kpad == ops.actor_core.padded_k_bf16(K)
  assert info['ksteps'] == kpad // 32 + 8
  assert info['grid'] == (32, (R + 15) // 16)
  assert info['width'] == (32 if A <= 32 else 64)
  assert ops.actor_core.packed_rows_bf16(A) <= info['max_k']
  return kpad


def _heads(A, Kv, g):
  return (0.1 * torch.randn(256, A, generator=g), 0.5 * torch.randn(A, generator=g),
          0.1 * torch.randn(256, Kv, generator=g), 0.5 * torch.randn(Kv, generator=g))


def _launch(ops, cuda, x, done, c, h, kernel, bias, heads, A, offset=OFFSET,
            **kw):
  """x [R, K] (CPU) is placed in a NaN-filled [R, K + 5] buffer at column 3;
  the outputs are the first R rows of sentinel-filled buffers of R + PAD_ROWS
  rows.  -> (outs, full buffers)."""
  R, K = x.shape
  buf = torch.full((R, K + 5), float('nan'), device=cuda)
  buf[:, 3:3 + K] = x.to(cuda)
  wpk = ops.actor_core.actor_core_bf16_pack(kernel.to(cuda), A)
  n = R + PAD_ROWS
  full = [torch.full((n,), int(SENTINEL), dtype=torch.int64, device=cuda),
          torch.full((n, A), SENTINEL, device=cuda),
          torch.full((n,), SENTINEL, device=cuda),
          torch.full((n, 256), SENTINEL, device=cuda),
          torch.full((n, 256), SENTINEL, device=cuda)]
  stream = ops.PhiloxStream(SEED)
  stream.offset = offset
  d = lambda t: t.to(cuda).contiguous()
  outs = ops.actor_core_step(buf[:, 3:3 + K], d(done), d(c), d(h), wpk, d(bias),
                             *[d(t) for t in heads], stream, dtype=BF,
                             outs=full, **kw)
  torch.cuda.synchronize()
  assert stream.offset == offset + 1
  for o, f in zip(outs, full):
    assert o.data_ptr() == f.data_ptr() and o.shape[0] == R
    assert bool((f[R:] == SENTINEL).all()), 'rows past R were written'
    assert bool(torch.isfinite(o.double()).all())
  return [o.cpu() for o in outs]


def _check(got, ref, what):
  for name, t in zip(('c2', 'h2'), got[3:]):
    want, bound = ref[name]
    err = (t.double() - want).abs()
    worst = float((err / bound).max())
    print('%s %s: max err %.3g, max err/bound %.3g' % (what, name,
                                                      float(err.max()), worst))
    assert bool((err <= bound).all()), (what, name, worst)


# ---------------------------------------------------------------- a. exact
def _exact_case(R, A, instr, seed):
  """Integer / dyadic operands, exact in bf16 with exact fp32 sums, and every
  row's product the same per column: W_x[k, n] = w(n) for every k, every row
  of x sums to S; W_h's rows come in (w, -w) pairs met by equal h_in pairs."""
  g = torch.Generator().manual_seed(seed)
  K, f_in = _k(A, instr), 257 + A + 64
  S = 5
  x = torch.randint(-2, 3, (R, K), generator=g).float()
  x[:, K - 1] = S - x[:, :K - 1].sum(1)
  wcol = torch.randint(-8, 9, (1024,), generator=g).float() / 8
  kernel = torch.empty(f_in + 256, 1024)
  kernel[:f_in] = wcol
  wh = torch.randint(-8, 9, (128, 1024), generator=g).float() / 8
  kernel[f_in::2] = wh
  kernel[f_in + 1::2] = -wh
  h = torch.randint(-3, 4, (R, 128), generator=g).float().repeat_interleave(2, 1)
  c = torch.randint(-8, 9, (R, 256), generator=g).float() / 4
  done = _done(R)
  h[done] = 3e30  # a done row's state is garbage
  c[done] = -3e30
  return x, h, c, done, kernel, S * wcol


@pytest.mark.parametrize('R,A,Kv,instr', CASES)
@pytest.mark.parametrize('big', [False, True])
def test_exact_case(cuda, R, A, Kv, instr, big):
  ops = _ops()
  kpad = _assert_info(ops, R, A, instr)
  x, h, c, done, kernel, colsum = _exact_case(R, A, instr, 7 + R + A)
  forget = torch.zeros(1024)
  forget[512:768] = 1.0
  bias = -colsum - forget + (24.0 if big else 0.0)
  heads = _heads(A, Kv, torch.Generator().manual_seed(3))
  got = _launch(ops, cuda, x, done, c, h, kernel, bias, heads, A)
  f_in, K = 257 + A + 64, _k(A, instr)
  ref = O.step(x, h, c, done, kernel[:K], kernel[f_in:], bias, kpad, chain=False)
  if not big:  # every pre-activation is exactly 0
    keep = (~done).double().unsqueeze(-1)
    c0 = torch.where(done.unsqueeze(-1), torch.zeros_like(c), c).double()
    assert torch.equal(ref['c2'][0], 0.5 * keep * c0)
  _check(got, ref, 'exact R%d A%d instr%d big%d' % (R, A, instr, big))


# --------------------------------------------------------------- b. random
_RANDOM = {}


def _random_case(R, A, Kv, instr):
  key = (R, A, Kv, instr)
  if key not in _RANDOM:
    g = torch.Generator().manual_seed(100 + 1000 * R + 10 * A + int(instr))
    K, f_in = _k(A, instr), 257 + A + 64
    x = torch.zeros(R, K)
    x[:, :256] = torch.relu(torch.randn(R, 256, generator=g))
    x[:, 256] = (3.0 * torch.randn(R, generator=g)).clamp(-1, 1)
    x[torch.arange(R), 257 + torch.randint(0, A, (R,), generator=g)] = 1.0
    if instr:
      x[:, 257 + A:] = torch.randn(R, 64, generator=g)
    kernel = 0.05 * torch.randn(f_in + 256, 1024, generator=g)
    bias = 0.5 * torch.randn(1024, generator=g)
    c = torch.randn(R, 256, generator=g)
    h = torch.randn(R, 256, generator=g)
    _RANDOM[key] = dict(x=x, kernel=kernel, bias=bias, c=c, h=h, done=_done(R),
                        heads=_heads(A, Kv, g), K=K, f_in=f_in)
  return _RANDOM[key]


_RUNS = {}


def _random_run(cuda, R, A, Kv, instr):
  key = (R, A, Kv, instr)
  if key not in _RUNS:
    ops = _ops()
    case = _random_case(R, A, Kv, instr)
    _RUNS[key] = _launch(ops, cuda, case['x'], case['done'], case['c'],
                         case['h'], case['kernel'], case['bias'],
                         case['heads'], A)
  return _RUNS[key]


@pytest.mark.parametrize('R,A,Kv,instr', CASES)
def test_random_case(cuda, R, A, Kv, instr):
  ops = _ops()
  kpad = _assert_info(ops, R, A, instr)
  case = _random_case(R, A, Kv, instr)
  got = _random_run(cuda, R, A, Kv, instr)
  K, f_in, done = case['K'], case['f_in'], case['done']
  ref = O.step(case['x'], case['h'], case['c'], done, case['kernel'][:K],
               case['kernel'][f_in:], case['bias'], kpad)
  _check(got, ref, 'random R%d A%d instr%d' % (R, A, instr))
  # done rows: large finite garbage in the state == the zero state, bitwise
  c, h = case['c'].clone(), case['h'].clone()
  c[done], h[done] = 3e38, -3e38
  c0, h0 = case['c'].clone(), case['h'].clone()
  c0[done], h0[done] = 0.0, 0.0
  run = lambda cc, hh: _launch(ops, cuda, case['x'], done, cc, hh,
                               case['kernel'], case['bias'], case['heads'], A)
  for a, b in zip(run(c, h), run(c0, h0)):
    assert torch.equal(a, b)


# ------------------------------------------------------ c. heads and sample
@pytest.mark.parametrize('R,A,Kv,instr', CASES)
def test_heads_and_sample(cuda, R, A, Kv, instr):
  ops = _ops()
  case = _random_case(R, A, Kv, instr)
  action, logits, baseline, _, h2 = _random_run(cuda, R, A, Kv, instr)
  wp, bp, wb, bb = [t.to(cuda) for t in case['heads']]
  stream = ops.PhiloxStream(SEED)
  stream.offset = OFFSET
  a_o, l_o, b_o = ops.actor_heads_sample(h2.to(cuda), wp, bp,
                                         wb[:, :1].contiguous(),
                                         bb[:1].contiguous(), stream)
  assert torch.equal(a_o.cpu(), action)
  assert torch.equal(l_o.cpu(), logits)
  assert torch.equal(b_o.cpu(), baseline)
  keys = logits.double().numpy() + _gumbel(R, A, OFFSET, SEED)
  sure = _top2_gap(keys) >= TIE
  assert (~sure).sum() <= 1
  assert (action.numpy()[sure] == keys.argmax(-1)[sure]).all()


def test_same_offset_same_actions_next_offset_differs(cuda):
  ops = _ops()
  case = _random_case(76, 63, 30, True)
  run = lambda off: _launch(ops, cuda, case['x'], case['done'], case['c'],
                            case['h'], case['kernel'], case['bias'],
                            case['heads'], 63, offset=off)
  a, b, c = run(OFFSET), run(OFFSET), run(OFFSET + 1)
  for s, t in zip(a, b):
    assert torch.equal(s, t)
  assert not torch.equal(a[0], c[0])
  for s, t in zip(a[1:], c[1:]):
    assert torch.equal(s, t)


def _dev_args(ops, cuda, R, A, Kv, instr):
  case = _random_case(R, A, Kv, instr)
  d = lambda t: t.to(cuda).contiguous()
  return [d(case['x']), d(case['done']), d(case['c']), d(case['h']),
          ops.actor_core.actor_core_bf16_pack(d(case['kernel']), A),
          d(case['bias'])] + [d(t) for t in case['heads']]


# -------------------------------------------------------- d. board epilogue
def test_board_epilogue_in_the_step(cuda):
  from scalable_agent_amd.ops.actor_core import BoardEpilogue
  from scalable_agent_amd.runtime.inference_board import InferenceBoard
  S, M, A = 4, 19, 63
  R = S * M  # 76
  ops = _ops()
  args = _dev_args(ops, cuda, R, A, 30, True)
  board = InferenceBoard(S, M, (8, 8, 3), A)
  offs = [o for _, _, _, o, _ in board.out_fields]
  mask = torch.zeros(R, 1, device=cuda)
  mask[::3] = 1.0  # mixed, in every row tile and slot
  mask[:M] = 1.0
  kept = mask.view(-1) > 0
  c0, h0 = args[2], args[3]
  stream = ops.PhiloxStream(SEED)

  def step(c, h, epilogue):
    stream.offset = OFFSET
    a = list(args)
    a[2], a[3] = c, h
    return ops.actor_core_step(*a, stream, epilogue=epilogue, dtype=BF)

  c_a, h_a = c0.clone(), h0.clone()
  out_a = torch.full((board.out_bytes,), 0x5A, dtype=torch.uint8, device=cuda)
  action, logits, baseline, c2, h2 = step(c_a, h_a, None)
  ops.ext().board_epilogue([action, logits, baseline, c2, h2], offs, out_a, M,
                           board.slot_out_bytes, mask, c2, h2, c_a, h_a)
  c_b, h_b = c0.clone(), h0.clone()  # commit into the step's own c_in / h_in
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
  assert torch.equal(c_a[kept], c2[kept]) and torch.equal(c_a[~kept], c0[~kept])
  assert torch.equal(h_a[kept], h2[kept]) and torch.equal(h_a[~kept], h0[~kept])
  assert torch.equal(out_a, out_b)
  for r in range(R):
    got = _row_bytes(board, out_b2, r)
    if bool(kept[r]):
      assert torch.equal(got, _row_bytes(board, out_a, r)), r
    else:
      assert bool((got == 0x5A).all()), r
  board.close()


# ----------------------------------------------------------- e. graph replay
def test_graph_replay_matches_eager_and_rearms(cuda):
  ops = _ops()
  args = _dev_args(ops, cuda, 17, 33, 1, True)
  tk = torch.zeros(8, dtype=torch.int32, device=cuda)
  step = lambda s: ops.actor_core_step(*args, s, ticket_words=tk, dtype=BF)
  eager_stream = ops.PhiloxStream(SEED, device=cuda)
  eager = [[t.clone() for t in step(eager_stream)] for _ in range(2)]
  assert eager_stream.device_offset == 2
  assert not torch.equal(eager[0][0], eager[1][0])
  stream = ops.PhiloxStream(SEED, device=cuda)
  side = torch.cuda.Stream(cuda)
  side.wait_stream(torch.cuda.current_stream(cuda))
  with torch.cuda.stream(side):
    step(stream)  # warm-up
    side.synchronize()
    stream.manual_seed(SEED)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      outs = step(stream)
    for n in range(2):
      g.replay()
      side.synchronize()
      for a, b in zip(outs, eager[n]):
        assert torch.equal(a, b), n
  assert stream.device_offset == 2
  assert int(stream.counter[1].item()) == 0
  assert int(tk.abs().sum().item()) == 0


# ------------------------------- f. accuracy against the unrounded fp64 step
def test_realistic_weights_track_the_unrounded_step(cuda):
  """max|err| / max|ref| of h2 and the logits against the float64 step on the
  UNROUNDED operands (the agent's own initialisation, R = 12): at most 1.5 x
  that of a torch emulation (operands cast to bf16, fp32 matmul, fp32 cell);
  1.5 allows for the different summation order.
  Measured on an MI355X (profiles/actor_core_bf16_step.txt): h2 kernel
  1.4670e-03 / emulation 1.4670e-03, logits 9.5320e-04 / 9.5318e-04."""
  ops = _ops()
  R, A = 12, 9
  agent = Agent(A, torso='shallow', frame_shape=(72, 96, 3), seed=5)
  g = torch.Generator().manual_seed(6)
  K, f_in = 257 + A, 257 + A + 64
  x = torch.zeros(R, K)
  x[:, :256] = torch.relu(torch.randn(R, 256, generator=g))
  x[:, 256] = torch.randn(R, generator=g).clamp(-1, 1)
  x[torch.arange(R), 257 + torch.randint(0, A, (R,), generator=g)] = 1.0
  c, h = torch.randn(R, 256, generator=g), torch.randn(R, 256, generator=g).tanh()
  done = _done(R)
  kernel, bias = agent.lstm_kernel.detach(), agent.lstm_bias.detach()
  heads = [t.detach() for t in (agent.policy_w, agent.policy_b,
                                agent.baseline_w, agent.baseline_b)]
  got = _launch(ops, cuda, x, done, c, h, kernel, bias, heads, A)

  def cell(gates, cc, dt):
    keep = (~done).to(dt).unsqueeze(-1)
    i, gg, f, o = gates.chunk(4, -1)
    c2 = torch.sigmoid(f + 1.0) * keep * cc.to(dt) + torch.sigmoid(i) * torch.tanh(gg)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2, h2 @ heads[0].to(dt) + heads[1].to(dt)

  hk = torch.where(done.unsqueeze(-1), torch.zeros_like(h), h)
  cz = torch.where(done.unsqueeze(-1), torch.zeros_like(c), c)
  a = torch.cat([x, hk], 1)
  w = torch.cat([kernel[:K], kernel[f_in:]], 0)
  ref_h, ref_l = cell(a.double() @ w.double() + bias.double(), cz, torch.float64)
  emu_h, emu_l = cell(a.to(BF).float() @ w.to(BF).float() + bias, cz, F32)
  for name, ref, emu, out in (('h2', ref_h, emu_h, got[4]),
                              ('logits', ref_l, emu_l, got[1])):
    scale = float(ref.abs().max())
    e_k = float((out.double() - ref).abs().max()) / scale
    e_e = float((emu.double() - ref).abs().max()) / scale
    print('bf16 core %s: err kernel %.4e emulation %.4e (max|ref| %.4g)' % (
        name, e_k, e_e, scale))
    assert e_k <= 1.5 * e_e, (name, e_k, e_e)


# -------------------------------------------------- g. agent and board level
SHAPE = (72, 96, 3)


def _model(cuda, core, torso, dtype=BF, seed=1, shape=SHAPE, instr=False):
  agent = Agent(9, torso=torso, frame_shape=shape, seed=seed, backend='hip',
                compute_dtype=dtype, actor_core=core)
  return inference.InferenceModel(agent, cuda, use_instruction=instr, seed=3)


def _cos(a, b):
  a, b = a.double().flatten(), b.double().flatten()
  return float(a @ b / (a.norm() * b.norm()))


@pytest.mark.parametrize('torso', ['shallow', 'deep'])
def test_step_device_fused_tracks_ops(cuda, torso):
  _ops()
  fused, plain = _model(cuda, 'fused', torso), _model(cuda, 'ops', torso)
  twin = _model(cuda, 'ops', torso, dtype=F32)
  assert fused.actor_core == 'fused' and plain.actor_core == 'ops'
  cache = fused.agent._inference_cache
  assert cache.get('wpk16') is not None and cache['wpk16'].dtype == BF
  assert 'wpk16' not in plain.agent._inference_cache
  ins = _step_inputs(cuda, 12)
  off0 = [m._gen.device_offset for m in (fused, plain)]
  f, o, t = (_step_device(m, ins) for m in (fused, plain, twin))
  assert [m._gen.device_offset for m in (fused, plain)] == [x + 1 for x in off0]
  for name in f:
    assert f[name].shape == o[name].shape and f[name].dtype == o[name].dtype
  assert int(f['action'].min()) >= 0 and int(f['action'].max()) < 9
  # the bar of test_shallow_bf16_infer_gpu.py: the bf16 / fp32 twins' cosine
  # minus 0.01
  bar = _cos(o['logits'], t['logits']) - 0.01
  got = _cos(f['logits'], o['logits'])
  print('%s step-logit cosine fused/ops %.6f (bf16/fp32 twins %.6f)' % (
      torso, got, bar + 0.01))
  assert got >= bar
  assert float((f['h2'] - o['h2']).abs().max()) <= 2e-2


def test_instruction_agent_fused_tracks_ops(cuda):
  _ops()
  fused = _model(cuda, 'fused', 'shallow', instr=True)
  plain = _model(cuda, 'ops', 'shallow', instr=True)
  assert fused.actor_core == 'fused'
  ins = _step_inputs(cuda, 12)
  g = torch.Generator().manual_seed(2)
  ins[4] = torch.randint(1, 50, (12, 16), generator=g).to(cuda)
  ins[5] = torch.randint(1, 17, (12,), generator=g).to(cuda)
  outs = []
  for m in (fused, plain):
    with m._lock, torch.cuda.stream(m.stream):
      r = m.step_device(*ins, has_instr=True)
      m.stream.synchronize()
    outs.append([x.cpu() for x in r])
  assert _cos(outs[0][1], outs[1][1]) >= 0.99
  assert float((outs[0][4] - outs[1][4]).abs().max()) <= 2e-2


def test_publish_refreshes_wpk16(cuda):
  _ops()
  from scalable_agent_amd.optim import FlatParams
  model = _model(cuda, 'fused', 'shallow', seed=1)
  other = _model(cuda, 'fused', 'shallow', seed=2)
  ins = _step_inputs(cuda, 12)
  ins[2] = torch.zeros_like(ins[2])  # every row keeps its h: W_h matters
  before = _step_device(model, ins)
  want = _step_device(other, ins)
  ptr = model.agent._inference_cache['wpk16'].data_ptr()
  model.publish(FlatParams(other.agent).params)
  torch.cuda.synchronize()
  cache = model.agent._inference_cache
  assert cache['wpk16'].data_ptr() == ptr  # refreshed in place
  assert torch.equal(cache['wpk16'], other.agent._inference_cache['wpk16'])
  after = _step_device(model, ins)
  assert not torch.equal(before['h2'], after['h2'])
  for name in ('logits', 'baseline', 'c2', 'h2'):
    assert torch.equal(after[name], want[name]), name


def test_board_server_native_matches_python_loop(cuda):
  """One launch of the native board server with the fused bf16 core returns
  the rows the Python serve loop returns (test_board_native_gpu.py's check;
  the two launches draw from consecutive Philox offsets, so the actions are
  not compared)."""
  from scalable_agent_amd.runtime import native
  from scalable_agent_amd.runtime.inference_board import (
      REQUEST, RESPONSE, BoardClient, BoardServer, InferenceBoard)
  ops = _ops()
  board = InferenceBoard(3, 4, SHAPE, 9)
  model = _model(cuda, 'fused', 'shallow')
  assert model.actor_core == 'fused'
  server = BoardServer(model, board)
  assert server._native_ok() and server.direct_out
  server.prepare(has_instr=False)
  g = torch.Generator().manual_seed(8)
  c0, h0 = torch.randn(12, 256, generator=g), torch.randn(12, 256, generator=g)
  rng = np.random.RandomState(5)
  cl = BoardClient(board, 1, 3)
  cl.inputs['frame'][:] = rng.randint(0, 256, cl.inputs['frame'].shape)
  cl.inputs['reward'][:] = 2.0 * rng.randn(3)
  cl.inputs['last_action'][:] = rng.randint(0, 9, 3)
  cl.inputs['done'][:] = [False, True, False]
  outs = []
  for loop in ('python', 'native'):
    server.c.copy_(c0)
    server.h.copy_(h0)
    board.buf[board.HDR + board.in_bytes:] = 0x5A
    native.atomic_store_u32(board.state_addr(1), REQUEST)
    if loop == 'python':
      assert server.serve_once(timeout_ms=10)
    else:
      b, m = board, server.model
      off = [o for n, _, _, o, _ in b.in_fields if n == 'instr_len'][0]
      ns = ops.ext().NativeBoardServer(
          b.base, b.HDR, b.in_bytes, b.slot_out_bytes, b.S, b.M, off,
          server.in_dev.data_ptr(), server.out_dev.data_ptr(),
          server.mask_dev.data_ptr(), server.mask_host.data_ptr(),
          m.stream.cuda_stream, server._graphs[False].raw_cuda_graph_exec(),
          0, cuda.index or 0)
      ns.set_direct_output(server.direct_out)
      assert ns.serve_once(10) and ns.rows_served() == 3
    assert board.state(1) == RESPONSE
    action, logits, baseline, c, h = [torch.from_numpy(x.copy())
                                      for x in cl.wait()]
    assert int(action.min()) >= 0 and int(action.max()) < 9
    st_c, st_h = server.c.cpu(), server.h.cpu()
    keep = [r for r in range(12) if not 4 <= r < 7]
    assert torch.equal(st_c[keep], c0[keep]) and torch.equal(st_h[keep], h0[keep])
    assert torch.equal(st_c[4:7], c) and torch.equal(st_h[4:7], h)
    outs.append((logits, baseline, c, h))
  for a, b in zip(*outs):
    assert torch.equal(a, b)
  assert not torch.equal(outs[0][3], h0[4:7])
  board.close()
