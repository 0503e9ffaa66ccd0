"""Numerics of the hand-written gfx950 HIP kernels vs fp32 PyTorch references.

Each kernel is compared with a plain PyTorch fp32 implementation of the same
op (reference semantics documented in the kernel sources).
"""

import pytest
import torch

from scalable_agent_amd import losses as L
from scalable_agent_amd import vtrace as V
from scalable_agent_amd.optim import polynomial_decay

pytestmark = pytest.mark.gpu


def _ops():
  from scalable_agent_amd import ops
  ops.load()  # fail loudly if the extension is missing on a GPU box
  return ops


def test_rmsprop_matches_tf_formula(cuda):
  ops = _ops()
  torch.manual_seed(0)
  n = 64 * 1000
  w = torch.randn(n, device=cuda)
  g = torch.randn(n, device=cuda)
  ms = torch.ones(n, device=cuda) + torch.rand(n, device=cuda)
  mom = torch.randn(n, device=cuda) * 0.01
  frames = torch.tensor(123456, device=cuda, dtype=torch.int64)
  lr0, F, decay, momentum, eps = 4.8e-4, 1e6, 0.99, 0.9, 0.1
  lr = polynomial_decay(lr0, 123456, F)
  ms_ref = ms + (g * g - ms) * (1 - decay)
  mom_ref = momentum * mom + lr * g / torch.sqrt(ms_ref + eps)
  w_ref = w - mom_ref
  ops.rmsprop_step(w, g, ms, mom, frames, lr0, F, decay, momentum, eps)
  torch.testing.assert_close(ms, ms_ref, rtol=1e-6, atol=1e-6)
  torch.testing.assert_close(mom, mom_ref, rtol=1e-5, atol=1e-8)
  torch.testing.assert_close(w, w_ref, rtol=1e-6, atol=1e-6)


def test_rmsprop_nonfinite_guard(cuda):
  """A NaN/inf anywhere in the gradient skips the whole update on the
  device and counts it; the next finite step applies normally."""
  ops = _ops()
  n = 64 * 300
  w = torch.randn(n, device=cuda)
  ms = torch.ones(n, device=cuda)
  mom = torch.zeros(n, device=cuda)
  frames = torch.zeros((), device=cuda, dtype=torch.int64)
  guard = torch.zeros(4, dtype=torch.int32, device=cuda)
  g = torch.randn(n, device=cuda)
  g[n - 7] = float('inf')
  w0, ms0 = w.clone(), ms.clone()
  ops.rmsprop_step(w, g, ms, mom, frames, 1e-3, 1e6, 0.99, 0., 0.1, guard)
  assert torch.equal(w, w0) and torch.equal(ms, ms0)
  assert guard.tolist() == [1, 1, 0, 0]
  g[n - 7] = 0.5
  ops.rmsprop_step(w, g, ms, mom, frames, 1e-3, 1e6, 0.99, 0., 0.1, guard)
  assert not torch.equal(w, w0)
  assert guard.tolist() == [0, 1, 0, 0]


def _ref_loss(bl, tl, a, r, done, v, boot, clip, bc, ec):
  cr = L.clip_rewards(r, clip)
  disc = (~done).float() * 0.99
  vt = V.from_logits(bl, tl, a, disc, cr, v, boot)
  pg = L.compute_policy_gradient_loss(tl, a, vt.pg_advantages)
  b = L.compute_baseline_loss(vt.vs - v)
  e = L.compute_entropy_loss(tl)
  return pg + bc * b + ec * e, (pg, b, e), vt


@pytest.mark.parametrize('clip', ['abs_one', 'soft_asymmetric'])
@pytest.mark.parametrize('T,B,A', [(100, 32, 9), (7, 5, 3), (130, 3, 18)])
def test_vtrace_loss_matches_reference(cuda, clip, T, B, A):
  ops = _ops()
  torch.manual_seed(1)
  bl = torch.randn(T, B, A, device=cuda)
  tl = torch.randn(T, B, A, device=cuda, requires_grad=True)
  a = torch.randint(0, A, (T, B), device=cuda)
  r = torch.randn(T, B, device=cuda) * 3
  done = torch.rand(T, B, device=cuda) < 0.05
  v = torch.randn(T, B, device=cuda, requires_grad=True)
  boot = torch.randn(B, device=cuda)
  bc, ec = 0.5, 0.01
  ref, (pg, b, e), vt = _ref_loss(bl, tl, a, r, done, v, boot, clip, bc, ec)
  ref.backward()
  out = ops.vtrace_fused_forward(bl, tl.detach(), a, r, done, v.detach(), boot,
                                 reward_clipping=clip, baseline_cost=bc,
                                 entropy_cost=ec)
  loss, dlogits, dvalues, vs, pga = out
  torch.testing.assert_close(vs, vt.vs, rtol=1e-4, atol=1e-4)
  torch.testing.assert_close(pga, vt.pg_advantages, rtol=1e-4, atol=1e-4)
  torch.testing.assert_close(loss[1], pg.detach(), rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(loss[2], b.detach(), rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(loss[3], e.detach(), rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(loss[0], ref.detach(), rtol=1e-4, atol=1e-3)
  torch.testing.assert_close(dlogits, tl.grad, rtol=1e-4, atol=1e-5)
  torch.testing.assert_close(dvalues, v.grad, rtol=1e-4, atol=1e-5)
  # autograd wrapper
  tl2 = tl.detach().clone().requires_grad_(True)
  v2 = v.detach().clone().requires_grad_(True)
  total = ops.vtrace_loss(bl, tl2, a, r, done, v2, boot, reward_clipping=clip,
                          baseline_cost=bc, entropy_cost=ec)
  (2.0 * total).backward()
  torch.testing.assert_close(tl2.grad, 2 * tl.grad, rtol=1e-4, atol=1e-5)
  torch.testing.assert_close(v2.grad, 2 * v.grad, rtol=1e-4, atol=1e-5)


def _ref_lstm(x, done, c, h, kernel, bias):
  F_in = x.shape[-1]
  kx, kh = kernel[:F_in], kernel[F_in:]
  outs = []
  for t in range(x.shape[0]):
    keep = (~done[t]).float().unsqueeze(-1)
    c = c * keep
    h = h * keep
    g = x[t] @ kx + bias + h @ kh
    i, ci, f, o = g.chunk(4, -1)
    c = torch.tanh(ci) * torch.sigmoid(i) + c * torch.sigmoid(f + 1.0)
    h = torch.tanh(c) * torch.sigmoid(o)
    outs.append(h)
  return torch.stack(outs), c


@pytest.fixture(params=['step', 'gang'])
def recurrence(request):
  """Runs an LSTM test on the exact-fp32 per-step kernels and on the default
  8-workgroup bf16 gang kernels (lstm_gang.hip; used for H == 256, B <= 32)."""
  from scalable_agent_amd.ops import lstm as lstm_ops
  _ops()
  prev = lstm_ops.set_gang(request.param == 'gang')
  yield request.param
  lstm_ops.set_gang(prev)


def _lstm_close(a, b, rtol, atol, bf16):
  """fp32 tolerances for the per-step kernels; bf16-operand accuracy (relative
  Frobenius error < 1e-2 and loose elementwise bounds) for the gang kernels.
  These free-running comparisons are the coarse check; the tight one, every
  step against float64 with derived bounds, is tests/test_lstm_oracle_gpu.py."""
  if not bf16:
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)
    return
  rel = float((a - b).norm() / b.norm().clamp_min(1e-12))
  assert rel < 1e-2, rel
  torch.testing.assert_close(a, b, rtol=0.1, atol=0.05 * float(b.abs().max()))


@pytest.mark.parametrize('T,B,H', [(101, 32, 256), (9, 5, 256), (13, 40, 64)])
def test_lstm_unroll_fwd_bwd(cuda, T, B, H, recurrence):
  ops = _ops()
  bf = recurrence == 'gang' and H == 256 and B <= 32
  torch.manual_seed(2)
  F_in = 330
  x = torch.randn(T, B, F_in, device=cuda, requires_grad=True)
  done = torch.rand(T, B, device=cuda) < 0.1
  c0 = torch.randn(B, H, device=cuda) * 0.5
  h0 = torch.randn(B, H, device=cuda) * 0.5
  kernel = (torch.randn(F_in + H, 4 * H, device=cuda) * 0.05).requires_grad_()
  bias = (torch.randn(4 * H, device=cuda) * 0.1).requires_grad_()
  hs_ref, c_ref = _ref_lstm(x, done, c0, h0, kernel, bias)
  go = torch.randn_like(hs_ref)
  (hs_ref * go).sum().backward()
  gx, gk, gb = x.grad.clone(), kernel.grad.clone(), bias.grad.clone()
  x.grad = kernel.grad = bias.grad = None
  hs, (c_last, h_last) = ops.lstm_unroll(x, done, (c0, h0), kernel, bias)
  _lstm_close(hs, hs_ref, 1e-4, 1e-5, bf)
  _lstm_close(c_last, c_ref, 1e-4, 1e-5, bf)
  (hs * go).sum().backward()
  _lstm_close(x.grad, gx, 1e-3, 1e-4, bf)
  _lstm_close(kernel.grad, gk, 1e-3, 1e-3, bf)
  _lstm_close(bias.grad, gb, 1e-3, 1e-3, bf)


@pytest.mark.parametrize('T,B,H', [(25, 32, 256), (7, 5, 64)])
def test_lstm_state_grads_and_chunking(cuda, T, B, H, recurrence):
  """dc0/dh0 from the HIP recurrence match autograd through the fp32
  reference, and an unroll split into chained time chunks (the pipelined
  learner) gives the same outputs and gradients as one unroll."""
  ops = _ops()
  bf = recurrence == 'gang' and H == 256 and B <= 32
  torch.manual_seed(3)
  F_in = 330
  x = torch.randn(T, B, F_in, device=cuda, requires_grad=True)
  done = torch.rand(T, B, device=cuda) < 0.1
  done[0, 0] = True
  c0 = (torch.randn(B, H, device=cuda) * 0.5).requires_grad_()
  h0 = (torch.randn(B, H, device=cuda) * 0.5).requires_grad_()
  kernel = (torch.randn(F_in + H, 4 * H, device=cuda) * 0.05).requires_grad_()
  bias = (torch.randn(4 * H, device=cuda) * 0.1).requires_grad_()
  leaves = [x, c0, h0, kernel, bias]
  hs_ref, c_ref = _ref_lstm(x, done, c0, h0, kernel, bias)
  go = torch.randn_like(hs_ref)
  gc = torch.randn_like(c_ref)
  ((hs_ref * go).sum() + (c_ref * gc).sum()).backward()
  ref = [t.grad.clone() for t in leaves]
  for split in (None, [0, T // 3, T // 2 + 1, T]):
    for t in leaves:
      t.grad = None
    if split is None:
      hs, (c_last, _) = ops.lstm_unroll(x, done, (c0, h0), kernel, bias)
    else:
      state, outs = (c0, h0), []
      w_x, w_h = kernel[:F_in], kernel[F_in:]
      for a, b in zip(split[:-1], split[1:]):
        h_k, state = ops.lstm_unroll(x[a:b], done[a:b], state, kernel, bias,
                                     w_x=w_x, w_h=w_h)
        outs.append(h_k)
      hs, c_last = torch.cat(outs), state[0]
    _lstm_close(hs, hs_ref, 1e-4, 1e-5, bf)
    _lstm_close(c_last, c_ref, 1e-4, 1e-5, bf)
    ((hs * go).sum() + (c_last * gc).sum()).backward()
    for t, g in zip(leaves, ref):
      _lstm_close(t.grad, g, 1e-3, 1e-3, bf)


@pytest.mark.parametrize('T,B', [(101, 32), (37, 7), (1, 32)])
def test_lstm_persistent_matches_per_step(cuda, T, B):
  """The opt-in whole-unroll persistent kernels (granule hand-offs between
  workgroups) reproduce the per-step kernels to fp32 rounding, identically
  over repeated launches (stale-tag / race check), and leave the error word
  clear."""
  ops = _ops()
  from scalable_agent_amd.ops import lstm as lstm_ops
  C = ops.ext()
  torch.manual_seed(9)
  H = 256
  xw = torch.randn(T, B, 4 * H, device=cuda)
  done = (torch.rand(T, B, device=cuda) < 0.1).to(torch.uint8)
  c0 = torch.randn(B, H, device=cuda) * 0.5
  h0 = torch.randn(B, H, device=cuda) * 0.5
  w_h = torch.randn(H, 4 * H, device=cuda) * 0.05
  dh = torch.randn(T, B, H, device=cuda)
  dcl = torch.randn(B, H, device=cuda)
  outs = {}
  prev = lstm_ops.set_persistent(False)
  try:
    for mode in (False, True):
      lstm_ops.set_persistent(mode)
      m = 1 if mode else 0  # explicit recurrence mode (persistent / step)
      runs = []
      for _ in range(3 if mode else 1):
        hs, cs, acts, hpm, wt = C.lstm_fwd(xw, done, c0, h0, w_h, m)
        dg, dc0, dg16 = C.lstm_bwd(dh, done, wt, acts, cs, c0, dcl, True, m)
        runs.append([hs, cs, acts, hpm, dg, dc0, dg16.float()])
      for r in runs[1:]:
        for a, b in zip(runs[0], r):
          assert torch.equal(a, b)
      outs[mode] = runs[0]
  finally:
    lstm_ops.set_persistent(prev)
  torch.cuda.synchronize()
  assert lstm_ops.persistent_error(cuda) == 0
  for i, (a, b) in enumerate(zip(outs[False], outs[True])):
    tol = 1e-2 if i == 6 else 1e-5  # bf16 copy of dG: one rounding step
    torch.testing.assert_close(b, a, rtol=tol, atol=tol * 0.1,
                               msg='output %d' % i)


@pytest.mark.parametrize('ws', [0, 1])
@pytest.mark.parametrize('T,B', [(101, 32), (37, 7), (2, 32), (2, 5)])
def test_lstm_gang_matches_per_step(cuda, T, B, ws):
  """The 8-workgroup gang kernels (bf16 recurrent product, granule
  all-gather fwd / reduce-scatter bwd) track the fp32 per-step kernels to
  bf16-operand accuracy, are bitwise repeatable over launches (stale-tag /
  race check) and leave the error word clear."""
  ops = _ops()
  from scalable_agent_amd.ops import lstm as lstm_ops
  C = ops.ext()
  torch.manual_seed(11)
  H = 256
  xw = torch.randn(T, B, 4 * H, device=cuda)
  done = (torch.rand(T, B, device=cuda) < 0.1).to(torch.uint8)
  c0 = torch.randn(B, H, device=cuda) * 0.5
  h0 = torch.randn(B, H, device=cuda) * 0.5
  w_h = torch.randn(H, 4 * H, device=cuda) * 0.05
  dh = torch.randn(T, B, H, device=cuda)
  dcl = torch.randn(B, H, device=cuda)
  outs = {}
  prev_p = lstm_ops.set_persistent(False)
  prev_g = lstm_ops.set_gang(False)
  prev_ws = C.lstm_gang_ws(ws)  # 1: the opt-in wave-specialised kernels
  try:
    for mode in (False, True):
      lstm_ops.set_gang(mode)
      m = 2 if mode else 0  # explicit recurrence mode (gang / step)
      runs = []
      for _ in range(3 if mode else 1):
        hs, cs, acts, hpm, wt = C.lstm_fwd(xw, done, c0, h0, w_h, m)
        dg, dc0, dg16 = C.lstm_bwd(dh, done, wt, acts, cs, c0, dcl, True, m)
        runs.append([hs, cs, acts, hpm, dg, dc0, dg16.float()])
      for r in runs[1:]:
        for a, b in zip(runs[0], r):
          assert torch.equal(a, b)
      outs[mode] = runs[0]
  finally:
    C.lstm_gang_ws(prev_ws)
    lstm_ops.set_gang(prev_g)
    lstm_ops.set_persistent(prev_p)
  torch.cuda.synchronize()
  assert lstm_ops.persistent_error(cuda) == 0
  names = ['hs', 'cs', 'acts', 'hpm', 'dg', 'dc0', 'dg16']
  for name, a, b in zip(names, outs[False], outs[True]):
    rel = float((b - a).norm() / a.norm().clamp_min(1e-12))
    assert rel < 1e-2, (name, rel)
    torch.testing.assert_close(b, a, rtol=0.1, atol=0.05, msg=name)


def test_instruction_encoder_hip_matches_torch(cuda):
  """Language LSTM (K7) on the H=64 fused step kernels vs the per-word
  PyTorch loop: outputs and gradients."""
  from scalable_agent_amd.models import Agent
  torch.manual_seed(3)
  ref = Agent(9, torso='shallow').to(cuda)
  hip = Agent(9, torso='shallow', backend='hip').to(cuda)
  hip.load_state_dict(ref.state_dict())
  N, L = 300, 7
  ids = torch.randint(0, 1000, (N, L), device=cuda)
  lengths = torch.randint(0, L + 1, (N,), device=cuda)
  lengths[:3] = torch.tensor([0, 1, L], device=cuda)
  out_r = ref.instruction_encoding((ids, lengths), N, cuda)
  out_h = hip.instruction_encoding((ids, lengths), N, cuda)
  torch.testing.assert_close(out_h, out_r, atol=2e-5, rtol=2e-5)
  assert float(out_h[0].detach().abs().max()) == 0.0
  gy = torch.randn_like(out_r)
  gr = torch.autograd.grad(out_r, [ref.language_lstm_kernel,
                                   ref.language_lstm_bias, ref.embed], gy)
  gh = torch.autograd.grad(out_h, [hip.language_lstm_kernel,
                                   hip.language_lstm_bias, hip.embed], gy)
  for a, b in zip(gh, gr):
    torch.testing.assert_close(a, b, atol=1e-4, rtol=1e-4)
