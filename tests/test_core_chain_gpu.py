"""The fused core's autograd chain (ops/core.py: _CoreLSTM for bf16 operands,
_CoreLSTMF32 for exact fp32), layer by layer against the float64 oracle of
the NETWORK (tests/_core_chain_oracle.py, tied to the model definition by
tests/test_core_chain_oracle.py).

The kernels themselves are held to float64 one at a time (test_gemm_*_gpu.py,
test_lstm_oracle_gpu.py, test_glue_edges_gpu.py); what strings them together
- which slice of lstm_kernel is W_x, W_h or the instruction rows, which saved
tensor masks which GEMM, K against f_in against ld, c_instr, keep0 on dh0,
dc_last / dhs arriving as None, which gradient view gets which product, the
side stream, the inference cache - was only checked by a cosine.  Here every
gemm_bf16, gemm_f32, lstm_fwd, lstm_bwd and colsum_f32_ call of the public
path (ops.core_lstm, then .backward) is recorded by a proxy around the
extension and checked TEACHER-FORCED: the oracle's layer is applied to the
chain's own recorded output of the previous layer, with the operands the
MODEL names for that layer (slices of kernel, w_fc, ... by the model's
layout, rounded to bf16 on the bf16 path as the kernels round them; never
the arguments of the call under check).

Cases (tests/_core_chain_oracle.py CASES; T, B -> branch):

  3, 5   A = 9, 15, 16, 1, 31, 63  N = 15 ragged tile; 6 / 0 / 15 pad columns;
                                   narrow and wide one-hot; mode 0 (the bf16
                                   calls pass allow_gang=False)
  3, 5   A = 9, 15, 16, instr      K = 336 / 336 exact / 352: pad columns meet
                                   W_h's first rows; d_instr
  3, 5   A = 9, Fd = 3456          the deep torso's feature width (else 136:
                                   a K tail of the FC GEMM)
  4, 32 and 5, 17, bf16            the gang (mode 2), with and without instr
  2, 33  bf16                      B past the gang: mode 0 under bf16 GEMMs
                                   (T = 2 has no interior step to reset at)
  4, 32  fp32                      mode 0, and the persistent mode 1 with
                                   lstm_set_persistent(True)
  6, 17  instr, both dtypes        state gradients, loss variants, two chunks,
                                   allow_gang False against True, sinks
Every case runs with c0 and h0 requiring grad and the loss on hs and c_last.
Out-of-range actions (-1, A, A + 1, the pad columns' indices, an index in the
instruction block, 2^32 + a valid index) sit in every case's input.

Bounds (the project's; nothing is fitted to the output):

  * GEMM outputs, max error over max |reference|: _gemm_oracle.TOL - fp32
    2e-6, bf16 operands with fp32 out 3e-6, bf16 out 8e-3.  Weight gradients
    are the after-minus-before delta of the view the call received, against
    the float64 product of the operands the kernel reads (bf16(h_aug), dg16,
    dh as recorded).
  * acts / cs / hs / dG / dc0: the derived per-element bounds of
    _lstm_oracle.forward / backward fed the recorded xw, hs, cs, dG.
  * db_lstm on the bf16 path (colsum_f32_): gamma_n sum|dG| + gamma_1
    |prefill|, n = 64 + ceil(N / 64) + 2 (test_glue_edges_gpu.py).
  * exact (torch.equal) on the recorded h_aug: the reward column is clip(r)
    rounded once, the one-hot columns, every pad column +0, the instruction
    columns; out-of-range rows are all zero; without instructions
    kernel.grad[257 + A : f_in] is exactly zero; kernel.grad[f_in:] is
    bitwise the hpm^T dG call's own result (the pad rows add exactly zero).
  * end to end against the exact float64 chain, relative L2 of hs and every
    gradient: fp32 <= 1e-4 and cosine >= 0.999999 (test_learner_parity_gpu.py);
    bf16 e_hip <= 2 e_emul, e_emul the emulated chain's error (both are sums
    of the same roundings at the same points; the emulated chain rounds
    dfeats too, which the kernel stores in bf16 like feats).

Each check prints error / bound; the module prints the worst ratio per kind
at its end (pytest -s).

Measured on an MI355X (pytest -s), worst over all cases:
  GEMM outputs, error / tolerance   h 0.39, xw 0.18, dh 0.38, dfeats 0.44,
                                    dW_h 0.24, dW_x 0.17, dW_fc 0.14, db_fc
                                    0.12, db_lstm (fp32) 0.18, d_instr 0.18,
                                    dh0 0.23
  recurrence, error / bound         acts 0.22, cs 0.14, hs 0.08 (any mode);
                                    dG 0.70 / 0.54 / 0.9997, dc0 0.32 / 0.28 /
                                    0.995 for modes 0 / 1 / 2 (mode 2: the
                                    near-tie allowance of whole bf16 ulps,
                                    near-tie share <= 0.345, limit 0.60)
  db_lstm (colsum_f32_)             0.057 of its gamma_n bound
  direct sink minus prefill         2.4e-7 (tol 1e-4); side stream bitwise
  fp32 end to end                   rel L2 <= 3.1e-7 (limit 1e-4)
  bf16 e_hip / e_emul               0.95 .. 1.008 for every tensor and case,
                                    chunked runs included (limit 2); e_emul is
                                    2e-3 for hs, 1e-3 .. 3e-3 for kernel, bias,
                                    instr_enc, c0, h0 and 1e-2 .. 4e-2 for
                                    feats, w_fc, b_fc
Before the epilogues were told num_actions, the out-of-range rows failed
"a pad column is not +0" on both paths, with and without instructions.
"""

import pytest
import torch

from scalable_agent_amd.ops import core, grad_sink
from tests import _core_chain_oracle as K
from tests import _gemm_oracle as G
from tests import _lstm_oracle as L

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
RECORDED = ('gemm_bf16', 'gemm_f32', 'lstm_fwd', 'lstm_bwd', 'colsum_f32_')
GEMMS = ('gemm_bf16', 'gemm_f32')
SINK_TOL = 1e-4  # test_deep_torso_chain_gpu.py: direct sink against fresh zeros
F32_L2, F32_COS = 1e-4, 0.999999  # test_learner_parity_gpu.py

_WORST = {}


def _note(kind, ratio):
  _WORST[kind] = max(_WORST.get(kind, 0.0), ratio)


@pytest.fixture(scope='module', autouse=True)
def _report():
  yield
  for kind in sorted(_WORST):
    print('\nCORECHAIN worst error/bound  %-28s %.4f' % (kind, _WORST[kind]), end='')
  print()


def _C():
  from scalable_agent_amd import ops
  ops.load()
  return ops.ext()


def _bits(x):
  x = x.contiguous()
  return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def _same(a, b, what):
  assert a.shape == b.shape and a.dtype == b.dtype, what
  assert torch.equal(_bits(a), _bits(b)), what


class Call:

  def __init__(self, name, args, kw, out, after, ptr):
    self.name, self.args, self.kw, self.out, self.after = name, args, kw, out, after
    self.ptr = ptr  # data_ptr of the tensor written in place, as passed

  def __repr__(self):
    return 'Call(%s)' % self.name


class Recorder:
  """Proxy around the extension: logs every core kernel call (scalars, clones
  of the tensor arguments before the call, the outputs, clones after the call
  of the arguments written in place: a GEMM's C and colsum, colsum_f32_'s
  out)."""

  def __init__(self, real):
    self._real = real
    self.calls = []

  def __getattr__(self, name):
    attr = getattr(self._real, name)
    if name not in RECORDED:
      return attr

    def wrapped(*args, **kw):
      cl = lambda a: a.detach().clone() if torch.is_tensor(a) else a
      before = tuple(cl(a) for a in args)
      kwb = {k: cl(v) for k, v in kw.items()}
      out = attr(*args, **kw)
      after, ptr = {}, None
      if name in GEMMS:
        after['C'], ptr = cl(args[4]), args[4].data_ptr()
        if kw.get('colsum') is not None:
          after['colsum'] = cl(kw['colsum'])
      elif name == 'colsum_f32_':
        after['out'], ptr = cl(args[1]), args[1].data_ptr()
      self.calls.append(Call(name, before, kwb, out, after, ptr))
      return out
    return wrapped


# ------------------------------------------------------------------- running

LEAVES = K.LEAVES


def device_inputs(c, inp, dev, state_grad=True):
  dt = BF if c['dtype'] == 'bf16' else torch.float32
  d = {}
  for k in LEAVES:
    if inp[k] is None:
      d[k] = None
      continue
    t = inp[k].to(dev)
    if k == 'feats':
      t = t.to(dt)
    d[k] = t.requires_grad_(state_grad or k not in ('c0', 'h0'))
  for k in ('rewards', 'actions', 'done', 'g_hs', 'g_c'):
    d[k] = inp[k].to(dev)
  return d


def call_core(c, d, t0=None, t1=None, state=None, allow_gang=None, cache=None):
  B = c['B']
  # the whole unroll passes the tensors themselves: no slice node stands
  # between the core and whatever produced feats
  cut = (lambda x: x) if t0 is None else (lambda x: x[t0 * B:t1 * B])
  done = d['done'] if t0 is None else d['done'][t0:t1]
  return core.core_lstm(
      cut(d['feats']), d['w_fc'], d['b_fc'], d['kernel'], d['bias'], cut(d['rewards']),
      cut(d['actions']), done, state or (d['c0'], d['h0']), c['A'],
      instr_enc=None if d['instr_enc'] is None else cut(d['instr_enc']),
      allow_gang=c['gang'] if allow_gang is None else allow_gang, cache=cache)


def loss_of(d, hs, c_last, loss):
  total = 0.0
  if loss in ('both', 'hs', 'hs+0c'):
    total = total + (hs * d['g_hs']).sum()
  if loss in ('both', 'c'):
    total = total + (c_last * d['g_c']).sum()
  if loss == 'hs+0c':  # an explicit all-zero dc_last
    total = total + (c_last * torch.zeros_like(d['g_c'])).sum()
  return total


def run(monkeypatch, c, inp, dev, loss='both', allow_gang=None, state_grad=True):
  """One recorded pass through the public path.  Returns (d, hs, c_last,
  calls); gradients are in the leaves' .grad."""
  d = device_inputs(c, inp, dev, state_grad)
  keep = {k: v.detach().clone() for k, v in d.items() if v is not None}
  rec = Recorder(_C())
  monkeypatch.setattr(core, 'ext', lambda: rec)
  hs, (c_last, h_last) = call_core(c, d, allow_gang=allow_gang)
  n_fwd = len(rec.calls)
  loss_of(d, hs, c_last, loss).backward()
  torch.cuda.synchronize()
  monkeypatch.undo()
  for k, v in keep.items():
    _same(d[k].detach(), v, 'the chain modified its input ' + k)
  _same(h_last.detach(), hs[-1].detach(), 'h_T is hs[-1]')
  return d, hs.detach(), c_last.detach(), rec.calls[:n_fwd], rec.calls[n_fwd:]


# ----------------------------------------------------------- layer checks

def held(kind, got, ref, bound):
  """Per-element derived bound (the LSTM oracles', the colsum's)."""
  ref, bound = ref.detach(), bound.detach()
  err = (K.d64(got) - ref).abs()
  ratio = float((err / bound.clamp_min(1e-300)).max())
  print('CORECHAIN %-26s max err %.3e  err/bound %.4f' % (kind, float(err.max()), ratio))
  _note(kind, ratio)
  bad = int((err > bound).sum())
  assert bad == 0, '%s: %d elements beyond the bound, worst ratio %g' % (kind, bad, ratio)


def gemm_close(kind, got, ref, tol):
  """max error over max |reference| under a _gemm_oracle.TOL entry."""
  assert tuple(got.shape) == tuple(ref.shape), (kind, got.shape, ref.shape)
  scale = float(ref.abs().max())
  assert scale > 0, kind + ': the reference is all zero'
  e = float((K.d64(got) - ref).abs().max()) / scale
  print('CORECHAIN %-26s rel err %.3e  err/tol %.4f' % (kind, e, e / tol))
  _note(kind, e / tol)
  assert e <= tol, '%s: %g > %g' % (kind, e, tol)


def model_weights(c, inp):
  """(w_fc, kernel) in float64 as the path's kernels read them: the model's,
  with w_fc and W_x = kernel[:f_in] rounded once to bf16 on the bf16 path."""
  w_fc, kernel = K.d64(inp['w_fc']), K.d64(inp['kernel']).clone()
  if c['dtype'] == 'bf16':
    w_fc = K.bf16(w_fc)
    kernel[:inp['f_in']] = K.bf16(kernel[:inp['f_in']])
  return w_fc, kernel


def check_h_aug(c, inp, h_aug):
  """The exact checks on the stored core input."""
  A, f_in, c_instr, Kc = inp['A'], inp['f_in'], inp['c_instr'], inp['K']
  dt = h_aug.dtype
  assert h_aug.shape == (inp['T'] * inp['B'], Kc), h_aug.shape
  h = h_aug.cpu()
  what = K.case_id(c)
  assert torch.equal(h[:, 256], inp['rewards'].clamp(-1, 1).to(dt)), what + ': reward column'
  oh = K.one_hot(inp['actions'], A).to(dt)
  assert torch.equal(h[:, 257:257 + A], oh), what + ': one-hot columns'
  pad = h[:, f_in:Kc] if inp['instr'] else h[:, c_instr:Kc]
  assert int(_bits(pad).count_nonzero()) == 0, what + ': a pad column is not +0'
  if inp['instr']:
    assert torch.equal(h[:, c_instr:f_in], inp['instr_enc'].to(dt)), what + ': instr columns'
  rows = inp['special_rows']
  assert int(_bits(h[rows][:, 257:257 + A]).count_nonzero()) == 0, \
      what + ': an out-of-range action set a one-hot column'
  tail = h[rows][:, f_in:] if inp['instr'] else h[rows][:, c_instr:]
  assert int(_bits(tail).count_nonzero()) == 0, \
      what + ': an out-of-range action set a pad column'


def model_x(inp, h_aug):
  """The model's core input [N, f_in] from the recorded h_aug."""
  h = K.d64(h_aug)
  if inp['instr']:
    return h[:, :inp['f_in']]
  return torch.cat([h[:, :inp['c_instr']],
                    torch.zeros(h.shape[0], K.INSTR, dtype=torch.float64)], 1)


def check_forward(c, inp, fwd, mode, hs, c_last, w4=False):
  bf = c['dtype'] == 'bf16'
  gemm = 'gemm_bf16' if bf else 'gemm_f32'
  assert [x.name for x in fwd] == [gemm, gemm, 'lstm_fwd'], fwd
  T, B, f_in = inp['T'], inp['B'], inp['f_in']
  w_fc, kernel = model_weights(c, inp)
  fc, xp, rc = fwd
  h_aug = xp.args[0]  # as it stood after the FC GEMM and the instruction copy
  assert h_aug.dtype == (BF if bf else torch.float32)
  check_h_aug(c, inp, h_aug)
  keepcols = torch.ones(h_aug.shape[1], dtype=torch.bool)
  if inp['instr']:
    keepcols[inp['c_instr']:f_in] = False
  _same(fc.after['C'].cpu()[:, keepcols], h_aug.cpu()[:, keepcols],
        'h_aug outside the instruction copy')
  ref = (K.d64(inp['feats']) @ w_fc + K.d64(inp['b_fc'])).relu()
  zeros = float((ref == 0).double().mean())
  assert 0.2 <= zeros <= 0.8, zeros
  gemm_close('h (torso FC)', h_aug[:, :256], ref, G.TOL[(c['dtype'], bf)])
  x = model_x(inp, h_aug)
  xw = xp.after['C']
  assert xw.dtype == torch.float32
  gemm_close('xw', xw, K.xproj(x, kernel, K.d64(inp['bias'])), G.TOL[(c['dtype'], False)])
  # the recurrence on the recorded xw, W_h the model's rows [f_in:]
  assert rc.args[5] == mode, 'lstm_fwd ran mode %r, expected %r' % (rc.args[5], mode)
  given = len(rc.args) > 6 and rc.args[6] is not None
  assert given == w4, 'packed w4 %s' % ('missing' if w4 else 'passed')
  o_hs, o_cs, o_acts, o_hpm = (t.cpu() for t in rc.out[:4])
  w_h = inp['kernel'][f_in:]
  done = inp['done'].to(torch.uint8)
  ref = L.forward(xw.cpu().view(T, B, -1), done, inp['c0'], inp['h0'], w_h, o_hs, o_cs, mode)
  for name, got in (('acts', o_acts), ('cs', o_cs), ('hs', o_hs)):
    held('%s mode %d' % (name, mode), got, *ref[name])
  _same(o_hpm, ref['hpm'][0], 'hpm is keep * h_prev bitwise')
  _same(hs.cpu(), o_hs, 'returned hs')
  _same(c_last.cpu(), o_cs[-1], 'returned c_T')
  return dict(h_aug=h_aug, x=x, xw=xw, hs=o_hs, cs=o_cs, acts=o_acts, hpm=o_hpm,
              w_fc=w_fc, kernel=kernel)


def delta(call, key='C'):
  before = call.args[4] if key == 'C' else call.kw['colsum']
  return K.d64(call.after[key]) - K.d64(before)


def check_backward(c, inp, d, fw, bwd, mode, loss):
  """Every backward call against the oracle layer on the recorded output of
  the previous one; then each leaf's gradient is the view its call wrote."""
  bf = c['dtype'] == 'bf16'
  gemm = 'gemm_bf16' if bf else 'gemm_f32'
  T, B, A, f_in, c_instr, Kc = (inp[k] for k in ('T', 'B', 'A', 'f_in', 'c_instr', 'K'))
  N = T * B
  state_grad = d['h0'].requires_grad
  want = ['lstm_bwd', gemm, gemm, 'gemm_f32', gemm] + (['colsum_f32_'] if bf else []) + [gemm]
  want += ['gemm_f32'] if state_grad else []
  want += [gemm] if inp['instr'] else []
  assert [x.name for x in bwd] == want, bwd
  it = iter(bwd)
  tol_out = G.TOL[(c['dtype'], bf)]     # outputs stored in the path's dtype
  tol_acc = G.TOL[(c['dtype'], False)]  # fp32 outputs
  w_fc, kernel = fw['w_fc'], fw['kernel']
  w_h = inp['kernel'][f_in:]
  done = inp['done'].to(torch.uint8)
  feats64 = K.d64(inp['feats'])

  rb = next(it)
  assert rb.args[8] == mode and rb.args[7] is bf
  assert (rb.args[6] is None) == (loss == 'hs'), 'dc_last for loss ' + loss
  g_hs = inp['g_hs'] if loss != 'c' else torch.zeros_like(inp['g_hs'])
  g_c = {'both': inp['g_c'], 'c': inp['g_c'], 'hs': None,
         'hs+0c': torch.zeros_like(inp['g_c'])}[loss]
  dg, dc0, dg16 = (t.cpu() for t in rb.out)
  ref = L.backward(g_hs, done, w_h, fw['acts'], fw['cs'], inp['c0'], g_c, dg, mode)
  held('dG mode %d' % mode, dg, *ref['dg'])
  held('dc0 mode %d' % mode, dc0, *ref['dc0'])
  if mode == 2:
    print('CORECHAIN near-tie element share %.3f' % ref['tie_share'])
    assert ref['tie_share'] <= L.MAX_TIE_SHARE
  if bf:
    _same(dg16, dg.to(BF), 'dg16 is RNE bf16 of dG')
  dg2 = K.d64(dg).reshape(N, -1)
  dgx = K.d64(dg16).reshape(N, -1) if bf else dg2  # what the GEMMs read

  call = next(it)
  dh = call.after['C']
  gemm_close('dh', dh, K.dh_layer(dgx, kernel, fw['x'][:, :256]), tol_out)
  assert bool((K.d64(dh) == 0).any()) and bool((K.d64(dh) != 0).any())
  dh64 = K.d64(dh)
  call_f = next(it)
  dfeats = call_f.after['C']
  assert dfeats.dtype == d['feats'].dtype
  gemm_close('dfeats', dfeats, K.dfeats_layer(dh64, w_fc, None if bf else feats64), tol_out)

  call_wh = next(it)
  assert call_wh.after['C'].shape == (256, 1024) and call_wh.kw.get('accumulate') is True
  gemm_close('dW_h', delta(call_wh), K.dw_h_layer(K.d64(fw['hpm']), dg2), G.TOL[('f32', False)])
  call_wx = next(it)
  assert call_wx.after['C'].shape == (Kc, 1024) and call_wx.kw.get('accumulate') is True
  dwx = delta(call_wx)
  ref_wx = K.dw_x_layer(fw['x'], dgx)
  m = min(Kc, f_in)
  gemm_close('dW_x', dwx[:m], ref_wx[:m], tol_acc)
  if inp['instr']:
    if Kc > f_in:
      assert float(dwx[f_in:].abs().max()) == 0, 'pad rows add to dW_h'
    assert float(ref_wx[c_instr:f_in].abs().max()) > 0
  elif Kc > c_instr:
    assert float(dwx[c_instr:].abs().max()) == 0, 'pad rows of W_x got a gradient'
  if bf:
    call_b = next(it)
    x_abs = dg2.abs().sum(0)
    pre = K.d64(call_b.args[1])
    n = 64 + (N + 63) // 64 + 2
    held('db_lstm (colsum_f32_)', K.d64(call_b.after['out']) - pre, K.db_lstm_layer(dg2),
         L.gamma(n) * x_abs + L.gamma(1) * pre.abs())
    db_after = call_b.after['out']
  else:
    gemm_close('db_lstm', delta(call_wx, 'colsum'), K.db_lstm_layer(dg2), tol_acc)
    db_after = call_wx.after['colsum']
  call_fc = next(it)
  assert call_fc.kw.get('accumulate') is True
  gemm_close('dW_fc', delta(call_fc), K.dw_fc_layer(feats64, dh64), tol_acc)
  gemm_close('db_fc', delta(call_fc, 'colsum'), K.db_fc_layer(dh64), tol_acc)

  keep0 = (inp['done'][0] == 0)
  if state_grad:
    call_h0 = next(it)
    raw = call_h0.after['C']
    gemm_close('dh0', raw, K.d64(dg[0]) @ K.d64(w_h).t(), G.TOL[('f32', False)])
    _same(d['h0'].grad, raw * keep0.to(raw.device).float().unsqueeze(-1), 'dh0 = keep0 * product')
    assert bool((~keep0).any())
    assert float(d['h0'].grad.cpu()[~keep0].abs().max()) == 0, 'dh0 of a reset row'
    assert float(d['c0'].grad.cpu()[~keep0].abs().max()) == 0, 'dc0 of a reset row'
    assert float(raw.cpu()[~keep0].abs().max()) > 0  # keep0 did the zeroing
    gemm_close('dh0 (masked)', d['h0'].grad, K.dh0_layer(K.d64(dg[0]), K.d64(w_h), done[0]),
               G.TOL[('f32', False)])
    _same(d['c0'].grad.cpu(), dc0, 'c0.grad is lstm_bwd dc0')
  if inp['instr']:
    call_i = next(it)
    gemm_close('d_instr', call_i.after['C'], K.d_instr_layer(dgx, kernel, c_instr, f_in), tol_acc)
    _same(d['instr_enc'].grad, call_i.after['C'], 'instr_enc.grad')

  # autograd hands every leaf the view its own call wrote
  kg = d['kernel'].grad
  assert kg.shape == d['kernel'].shape and kg.dtype == torch.float32
  _same(kg[f_in:], call_wh.after['C'], 'kernel.grad[f_in:] is the hpm^T dG call result')
  _same(kg[:Kc], call_wx.after['C'], 'kernel.grad[:K]')
  if not inp['instr']:
    assert float(kg[c_instr:f_in].abs().max()) == 0, 'kernel.grad[257 + A : f_in]'
  _same(d['bias'].grad, db_after, 'bias.grad')
  _same(d['w_fc'].grad, call_fc.after['C'], 'w_fc.grad')
  _same(d['b_fc'].grad, call_fc.after['colsum'], 'b_fc.grad')
  _same(d['feats'].grad, dfeats, 'feats.grad')
  return dg


def end_to_end(c, inp, mode, loss, hs, grads, tag=''):
  """hs and every gradient against the exact float64 chain."""
  bf = c['dtype'] == 'bf16'
  g_hs = inp['g_hs'] if loss != 'c' else None
  g_c = inp['g_c'] if loss in ('both', 'c') else None
  ex = K.forward_chain(inp)
  gx = K.backward_chain(ex, g_hs, g_c, mask_feats=not bf)
  rows = [('hs', hs, ex['hs'])] + [(n, grads[n], gx[n]) for n in LEAVES if grads.get(n) is not None]
  if bf:
    em = K.forward_chain(inp, rnd=K.bf16, mode=mode)
    ge = K.backward_chain(em, g_hs, g_c, rnd=K.bf16)
    emul = dict(ge, hs=em['hs'])
  bad = []
  for name, got, ref in rows:
    if float(ref.abs().max()) == 0:  # e.g. dh0 of a loss that cannot reach it
      assert float(K.d64(got).abs().max()) == 0, name
      continue
    e = K.rel_l2(got, ref)
    if bf:
      e_emul = K.rel_l2(emul[name], ref)
      assert e_emul > 0, name
      ratio = e / (2 * e_emul)
      print('CORECHAIN %s%s e2e %-9s e_emul=%.3e e_hip=%.3e  e_hip/(2 e_emul)=%.3f' %
            (K.case_id(c), tag, name, e_emul, e, ratio))
      _note('e2e bf16 e_hip / (2 e_emul)', ratio)
      if not e <= 2 * e_emul:
        bad.append((name, e, e_emul))
    else:
      cos = K.cosine(got, ref)
      print('CORECHAIN %s%s e2e %-9s rel L2=%.3e (<= 1e-4)  1-cos=%.2e' %
            (K.case_id(c), tag, name, e, 1 - cos))
      _note('e2e fp32 rel L2 / 1e-4', e / F32_L2)
      if not (e <= F32_L2 and cos >= F32_COS):
        bad.append((name, e, cos))
  assert not bad, bad


def grads_of(d):
  return {n: (None if d[n] is None or d[n].grad is None else d[n].grad.detach().cpu())
          for n in LEAVES}


def layer_by_layer(monkeypatch, cuda, c, mode, loss='both', allow_gang=None):
  inp = K.draw(c['seed'], c['T'], c['B'], c['A'], c['Fd'], c['instr'])
  d, hs, c_last, fwd, bwd = run(monkeypatch, c, inp, cuda, loss, allow_gang)
  fw = check_forward(c, inp, fwd, mode, hs, c_last)
  check_backward(c, inp, d, fw, bwd, mode, loss)
  end_to_end(c, inp, mode, loss, hs.cpu(), grads_of(d))
  return inp, d, hs, c_last


# --------------------------------------------------------------------- tests

@pytest.mark.parametrize('c', K.CASES, ids=K.case_id)
def test_chain_layer_by_layer(cuda, monkeypatch, c):
  C = _C()
  exact = c['dtype'] == 'f32' or not c['gang']
  assert C.lstm_mode(256, c['B'], c['T'], exact) == c['mode'], 'lstm_mode'
  layer_by_layer(monkeypatch, cuda, c, c['mode'])


@pytest.mark.parametrize('on', [False, True])
def test_fp32_persistent_switch(cuda, monkeypatch, on):
  """fp32, T = 4, B = 32 with lstm_set_persistent both ways: the recurrence
  that runs is the one lstm_mode picks (1 when on: H = 256, B <= 32)."""
  C = _C()
  c = K.F32_WIDE[0]
  prev = C.lstm_get_persistent()
  C.lstm_set_persistent(on)
  try:
    mode = C.lstm_mode(256, c['B'], c['T'], True)
    assert mode == int(on)
    layer_by_layer(monkeypatch, cuda, c, mode)
    from scalable_agent_amd.ops import lstm as lstm_ops
    assert lstm_ops.persistent_error(cuda) == 0
  finally:
    C.lstm_set_persistent(prev)


@pytest.mark.parametrize('c', K.STATE, ids=K.case_id)
@pytest.mark.parametrize('loss', ['c', 'hs'])
def test_loss_on_one_output(cuda, monkeypatch, c, loss):
  """The loss on c_last only (dhs arrives as None) and on hs only (dc_last is
  None: bitwise the run with an explicit all-zero dc_last)."""
  inp, d, hs, c_last = layer_by_layer(monkeypatch, cuda, c, c['mode'], loss=loss)
  if loss == 'hs':
    d0, _, _, fwd, bwd = run(monkeypatch, c, inp, cuda, 'hs+0c')
    assert bwd[0].args[6] is not None and float(bwd[0].args[6].abs().max()) == 0
    for n in LEAVES:
      if d[n] is not None:
        _same(d0[n].grad, d[n].grad, 'explicit zero dc_last: ' + n)


def test_gang_switch_changes_the_mode_only(cuda, monkeypatch):
  """allow_gang=False against True on the bf16 path: both hold the oracle,
  the recorded mode differs."""
  c = K.STATE[0]
  assert c['dtype'] == 'bf16' and c['mode'] == 2
  layer_by_layer(monkeypatch, cuda, c, 0, allow_gang=False)
  layer_by_layer(monkeypatch, cuda, c, 2, allow_gang=True)


@pytest.mark.parametrize('c', K.STATE, ids=K.case_id)
def test_two_chained_chunks(cuda, c):
  """core_lstm on [0, a), state carried with grad into [a, T), a row reset
  exactly at a (the _pipelined_core wiring), against the whole unroll's
  oracle."""
  inp = K.draw(c['seed'], c['T'], c['B'], c['A'], c['Fd'], c['instr'])
  T = c['T']
  a = T // 2
  assert bool(inp['done'][a, 2]) and not bool(inp['done'][a, 3])
  d = device_inputs(c, inp, cuda)
  hs1, (c_mid, h_mid) = call_core(c, d, 0, a)
  c_mid.retain_grad()
  h_mid.retain_grad()
  hs2, (c_last, _) = call_core(c, d, a, T, state=(c_mid, h_mid))
  hs = torch.cat([hs1, hs2], 0)
  loss_of(d, hs, c_last, 'both').backward()
  torch.cuda.synchronize()
  for g in (c_mid.grad, h_mid.grad):
    assert float(g[2].abs().max()) == 0 and float(g[3].abs().max()) > 0
  end_to_end(c, inp, c['mode'], 'both', hs.detach().cpu(), grads_of(d), tag=' chunks')


def make_cache(C, c, d, inp):
  """As Agent.refresh_inference_cache builds it."""
  f_in = inp['f_in']
  dev = d['kernel'].device
  with torch.no_grad():
    w4 = torch.empty(256 * 1024, device=dev)
    C.lstm_pack_fwd(d['kernel'][f_in:], w4)
    w16 = None
    if c['dtype'] == 'bf16':
      k_max = (f_in + 15) // 16 * 16
      w16 = (torch.empty(d['w_fc'].shape, dtype=BF, device=dev),
             torch.empty(k_max, 1024, dtype=BF, device=dev))
      w16[0].copy_(d['w_fc'])
      w16[1].copy_(d['kernel'][:k_max])
  return {'w4': w4, 'w16': w16}


CACHED = [K.SMALL[0], K.SMALL[6], K.GANG[0], K.GANG[1], K.PAST_GANG[0], K.F32_WIDE[0],
          K.STATE[1]]


# the gang takes precedence over the persistent kernels: no such pair
CACHED = [(c, False) for c in CACHED] + [(c, True) for c in CACHED if c['mode'] != 2]


@pytest.mark.parametrize('c,persistent', CACHED,
                         ids=lambda v: K.case_id(v) if isinstance(v, dict) else 'p%d' % v)
def test_inference_cache(cuda, monkeypatch, c, persistent):
  """Under no_grad with the inference cache: outputs are bitwise the uncached
  call's, the forward holds the oracle, modes 0 and 1 receive the packed w4
  and the gang must not."""
  C = _C()
  prev = C.lstm_get_persistent()
  C.lstm_set_persistent(persistent)
  try:
    mode = 1 if (persistent and c['B'] <= 32) else c['mode']
    inp = K.draw(c['seed'], c['T'], c['B'], c['A'], c['Fd'], c['instr'])
    d = device_inputs(c, inp, cuda)
    with torch.no_grad():
      hs0, (c0_, _) = call_core(c, d)
      rec = Recorder(C)
      monkeypatch.setattr(core, 'ext', lambda: rec)
      hs1, (c1_, _) = call_core(c, d, cache=make_cache(C, c, d, inp))
      torch.cuda.synchronize()
      monkeypatch.undo()
    _same(hs1, hs0, 'cached hs')
    _same(c1_, c0_, 'cached c_T')
    check_forward(c, inp, rec.calls, mode, hs1, c1_, w4=mode != 2)
  finally:
    C.lstm_set_persistent(prev)


class _Probe(torch.autograd.Function):
  """Identity in front of the core, standing where the torso stands: its
  backward sees the gradient object the core returns."""
  seen = None

  @staticmethod
  def forward(ctx, x):
    return x.view_as(x)

  @staticmethod
  def backward(ctx, g):
    _Probe.seen = (getattr(g, '_sa_relu_masked', False), g.detach().clone())
    return g


SINKS = [K.SMALL[0], K.SMALL[6], K.SMALL[12], K.SMALL[15]] + K.STATE
PARAMS = ('w_fc', 'b_fc', 'kernel', 'bias')


@pytest.mark.parametrize('c', SINKS, ids=K.case_id)
def test_sinks_and_side_stream(cuda, c):
  """Direct sinks add to a non-zero prefill (autograd gets None); with the
  weight gradients on the side stream the result is bitwise the same; dfeats
  is bitwise equal across the three modes; _sa_relu_masked on fp32 only."""
  inp = K.draw(c['seed'], c['T'], c['B'], c['A'], c['Fd'], c['instr'])

  def once(mode, prefill=None):
    d = device_inputs(c, inp, cuda)
    keep = {k: v.detach().clone() for k, v in d.items() if v is not None}
    leaf = d['feats']
    d['feats'] = _Probe.apply(leaf)
    _Probe.seen = None
    if prefill is not None:
      for n in PARAMS:
        d[n].grad = prefill[n].clone()
    sinks = {n: d[n].grad for n in PARAMS}
    ctxs = {'plain': [], 'direct': [grad_sink.direct_grads()],
            'overlap': [grad_sink.direct_grads(), grad_sink.overlap_weight_grads()]}[mode]
    import contextlib
    with contextlib.ExitStack() as st:
      for cm in ctxs:
        st.enter_context(cm)
      hs, (c_last, _) = call_core(c, d)
      got = torch.autograd.grad(loss_of(d, hs, c_last, 'both'),
                                [d[n] for n in PARAMS] + [leaf], allow_unused=True)
    torch.cuda.synchronize()
    d['feats'] = leaf
    for k, v in keep.items():
      _same(d[k].detach(), v, 'the chain modified its input ' + k)
    masked, dfeats = _Probe.seen
    assert masked is (c['dtype'] == 'f32'), '_sa_relu_masked on the fp32 path only'
    _same(got[-1], dfeats, 'dfeats through the probe')
    if mode == 'plain':
      return {n: g for n, g in zip(PARAMS, got)}, dfeats
    assert all(g is None for g in got[:4]), 'autograd must get None for direct sinks'
    for n in PARAMS:
      assert d[n].grad is sinks[n], n
    return {n: d[n].grad for n in PARAMS}, dfeats

  fresh, df0 = once('plain')
  gen = torch.Generator().manual_seed(c['seed'])
  prefill = {}
  for n in PARAMS:
    scale = float(fresh[n].abs().max())
    assert scale > 0, n
    prefill[n] = (torch.randn(fresh[n].shape, generator=gen) * scale).to(cuda)
    assert bool((prefill[n] != 0).all())
  direct, df1 = once('direct', prefill)
  for n in PARAMS:
    ref = K.d64(fresh[n])
    e = float((K.d64(direct[n]) - K.d64(prefill[n]) - ref).abs().max()) / float(ref.abs().max())
    print('CORECHAIN %s direct sink %-6s minus prefill vs fresh: %.3e' % (K.case_id(c), n, e))
    _note('direct sink / 1e-4', e / SINK_TOL)
    assert e <= SINK_TOL, (n, e)
  over, df2 = once('overlap', prefill)
  assert not grad_sink._PENDING
  for n in PARAMS:
    _same(over[n], direct[n], 'side-stream weight gradients, ' + n)
  _same(df1, df0, 'dfeats, direct sinks')
  _same(df2, df0, 'dfeats, side stream')


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_gemm_aug_out_of_range_actions(cuda, dtype):
  """The GEMM epilogue's core-input columns with aug_num_actions, in the
  poisoned storage of _gemm_oracle: indices outside [0, A) give a zero row
  and every column past the one-hot stays 0; the default (no count) keeps
  treating every column after the reward as a one-hot column."""
  C = _C()
  A = 9
  for c_bf16 in ((False, True) if dtype == 'bf16' else (False,)):
    s = G.spec(dtype, 37, 64, 136, False, False, bias=True, relu=True, naug=16,
               c_bf16=c_bf16)
    c = G.make(s, 'int')
    a = G.view1(c['action'], c['action_at'])
    special = [-1, A, A + 1, 14, 15, 2 ** 32 + 2, -2 ** 32 + 3, 2 ** 31]
    a[1:1 + len(special)] = torch.tensor(special)
    a[0] = A - 1
    ref = G.reference(dict(c, action=torch.zeros_like(c['action'])))
    aug = torch.zeros(37, 16, dtype=torch.float64)
    aug[:, 0] = ref['aug'][:, 0]
    aug[:, 1:1 + A] = K.one_hot(a, A)
    ref['aug'] = aug
    assert float(aug[1:1 + len(special), 1:].abs().max()) == 0 and aug[0, A] == 1

    def launch(**extra):
      dd = {k: c[k].to(cuda) for k in ('A', 'B', 'C', 'bias', 'reward', 'action')}
      fn = C.gemm_f32 if dtype == 'f32' else C.gemm_bf16
      fn(G.view(dd['A'], c['A_at']), G.view(dd['B'], c['B_at']), False, False,
         G.view(dd['C'], c['C_at']), bias=G.view1(dd['bias'], c['bias_at']), relu=True,
         aug_reward=G.view1(dd['reward'], c['reward_at']),
         aug_action=G.view1(dd['action'], c['action_at']), **extra)
      return {'C': dd['C'].cpu()}

    G.check(c, launch(aug_num_actions=A), ref)
    # the default: 15 one-hot columns, so 14 is a valid index there (and the
    # 64-bit comparison still rejects the wrapped ones)
    ref15 = dict(ref, aug=aug.clone())
    ref15['aug'][:, 1:] = K.one_hot(a, 15)
    assert ref15['aug'][4, 15] == 1
    G.check(c, launch(), ref15)
