"""Float64 CPU oracle of the learner's core as a NETWORK (test helper).

_gemm_oracle.py and _lstm_oracle.py hold the single operations.  Here they
are composed into the layers of the core - torso FC, core-input columns,
x-projection, LSTM-256 recurrence, every gradient - and into the whole
chain.  The wiring is read from the model definition (models/agent.py:
core_inputs, core_unroll): x = [relu(feats W_fc + b_fc), clip(r, -1, 1),
one_hot(a), instr | 0], W_x = lstm_kernel[:f_in], W_h = lstm_kernel[f_in:],
f_in = 257 + A + 64; nothing here looks at scalable_agent_amd.ops.core (whose
slices, saved tensors, pads and flags are what test_core_chain_gpu.py
checks).  test_core_chain_oracle.py ties the chain to Agent(backend='torch',
compute_dtype=float64) under autograd to 1e-10.

Every layer function takes the previous layer's tensor and returns float64.
The recurrence goes through _lstm_oracle.forward / backward: those compute
every step from given previous outputs (teacher forcing), so the free-running
recurrence is their fixed point, reached after T sweeps (sweep k makes step
k - 1 final forward, step T - k backward).

Rounding.  `forward_chain` / `backward_chain` take `rnd`, applied where the
bf16 path (_CoreLSTM and its kernels) rounds: w_fc and W_x (one fp32 -> bf16
conversion, round to nearest even), h_aug as stored (torso columns, the
clipped reward, the copied instruction encoding), dG's bf16 copy dg16 (the
operand of the dh, dW_x and d_instr GEMMs), dh as stored, dfeats as stored
(it has the dtype of feats), and with mode 2 the gang's h_{t-1}, W_h and
exchanged partials, exactly as _lstm_oracle's R.  dW_h, db_lstm, dh0 and dc0
read the fp32 dG.  rnd=None is the exact chain; rnd=bf16 the emulated chain
of the GPU test's end-to-end number.
"""

import torch

from tests import _lstm_oracle as L

CORE = 256
INSTR = 64


def bf16(x):
  """Round to bf16 and back (through fp32, round to nearest even, as the
  kernels' fp32 -> bf16 conversion)."""
  return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def d64(x):
  return x.detach().to('cpu', torch.float64)


def _id(x):
  return x


def widths(A, instr):
  """The model's column layout: f_in, c_instr (first instruction column) and
  K, the columns the kernels multiply: everything before the instruction
  block padded to 16 without instructions (that block is zero and drops
  out), f_in padded to 16 with them."""
  f_in = CORE + 1 + A + INSTR
  c_instr = CORE + 1 + A
  K = ((f_in if instr else c_instr) + 15) // 16 * 16
  return dict(f_in=f_in, c_instr=c_instr, K=K)


def special_actions(A, instr):
  """Indices outside [0, A) that must give an all-zero one-hot: -1, A, A + 1,
  the last pad column (K - 258; without instructions and 257 + A a multiple
  of 16 there is none), with instructions the first pad column at f_in too,
  an index inside the instruction block, and one whose low 32 bits are a
  valid action."""
  w = widths(A, instr)
  out = [-1, A, A + 1, 2 ** 32 + min(2, A - 1)]
  if instr:
    out.append(A + 3)  # inside the instruction block
    if w['K'] > w['f_in']:
      out += [w['f_in'] - CORE - 1, w['K'] - CORE - 2]
  elif w['K'] > w['c_instr']:
    out.append(w['K'] - CORE - 2)
  return out


def done_pattern(T, B):
  """Resets at t = 0 (row 0), t = T - 1 (row 1) and an interior step (row 2,
  t = T // 2; T = 2 has no interior step), on different rows; even rows from
  4 on reset at (t + row) % 5 == 0 where that is not t = 0; odd rows from 3
  on never reset, so the initial state reaches the last step."""
  done = torch.zeros(T, B, dtype=torch.bool)
  done[0, 0] = True
  if B > 1:
    done[T - 1, 1] = True
  if B > 2 and T > 2:
    done[T // 2, 2] = True
  for b in range(4, B, 2):
    for t in range(1, T):
      if (t + b) % 5 == 0:
        done[t, b] = True
  return done


def draw(seed, T, B, A, Fd, instr):
  """Inputs on the CPU from a fixed seed, fp32 (feats, w_fc are exact in
  bf16 / fp32 as stated), so oracle and kernels read identical bits.
  feats = relu(pre) with bf16-representable values: the same bits serve the
  bf16 and the fp32 path.  Rewards hold -1, 1 exactly, values below -1 and
  above 1; actions hold every index of special_actions."""
  gen = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=gen)
  N = T * B
  w = widths(A, instr)
  pre = rn(N, Fd).to(torch.bfloat16).float()
  inp = dict(T=T, B=B, A=A, Fd=Fd, instr=bool(instr), seed=seed, **w)
  inp['pre'] = pre
  inp['feats'] = pre.relu()
  inp['w_fc'] = rn(Fd, CORE) * Fd ** -0.5
  inp['b_fc'] = rn(CORE) * 0.1
  inp['kernel'] = rn(w['f_in'] + CORE, 4 * CORE) * 0.05
  inp['bias'] = rn(4 * CORE) * 0.1
  inp['instr_enc'] = (rn(N, INSTR) * 0.5).tanh() if instr else None
  inp['c0'] = rn(B, CORE) * 0.5
  inp['h0'] = rn(B, CORE) * 0.5
  r = rn(N) * 2
  r[0], r[1], r[2], r[3] = -1.0, 1.0, -3.5, 2.25
  inp['rewards'] = r
  a = torch.randint(0, A, (N,), generator=gen)
  sp = special_actions(A, instr)
  assert 2 * len(sp) <= N
  rows = [(2 * i + 1) % N for i in range(len(sp))]
  a[rows] = torch.tensor(sp)
  inp['actions'] = a
  inp['special_rows'] = rows
  inp['done'] = done_pattern(T, B)
  inp['g_hs'] = rn(T, B, CORE)
  inp['g_c'] = rn(B, CORE)
  return inp


def case(dtype, T, B, A, instr, gang=False, Fd=136, seed=None):
  """One case of test_core_chain_gpu.py.  gang: the call allows the bf16 gang
  recurrence; mode is the recurrence that must then run (2 = gang: bf16
  path, B <= 32, T >= 2), the fp32 persistent mode 1 is switched on by its
  own test."""
  mode = 2 if (gang and dtype == 'bf16' and B <= 32 and T >= 2) else 0
  seed = 1000 * T + 10 * B + A + int(instr) * 500 if seed is None else seed
  return dict(dtype=dtype, T=T, B=B, A=A, instr=instr, gang=gang, Fd=Fd,
              seed=seed, mode=mode)


def case_id(c):
  return '%s-T%dB%d-A%d%s%s-Fd%d' % (c['dtype'], c['T'], c['B'], c['A'],
                                     '-instr' if c['instr'] else '',
                                     '-gang' if c['gang'] else '', c['Fd'])


# the smallest shapes at which each branch exists (N = 15: a ragged GEMM
# tile; Fd = 136: a K tail of the FC GEMM; one case at the deep torso's 3456)
SMALL = [case(d, 3, 5, A, False) for d in ('bf16', 'f32') for A in (9, 15, 16, 1, 31, 63)]
SMALL += [case(d, 3, 5, A, True) for d in ('bf16', 'f32') for A in (9, 15, 16)]
SMALL += [case(d, 3, 5, 9, False, Fd=3456) for d in ('bf16', 'f32')]
GANG = [case('bf16', T, B, 9, ins, gang=True) for T, B in ((4, 32), (5, 17))
        for ins in (False, True)]
PAST_GANG = [case('bf16', 2, 33, 9, False, gang=True)]
F32_WIDE = [case('f32', 4, 32, 9, False)]
STATE = [case('bf16', 6, 17, 9, True, gang=True), case('f32', 6, 17, 9, True)]
CASES = SMALL + GANG + PAST_GANG + F32_WIDE + STATE


# ------------------------------------------------------------ forward layers

def one_hot(actions, A):
  """tf.one_hot: an index outside [0, A) gives a zero row."""
  return (actions.reshape(-1, 1).long() == torch.arange(A)).to(torch.float64)


def fc_aug(feats, w_fc, b_fc, rewards, actions, A, instr_enc, rnd=_id):
  """x [N, f_in] = [relu(feats W_fc + b_fc), clip(r, -1, 1), one_hot(a),
  instr or zeros]; rnd: the rounding of the stored values."""
  N = feats.shape[0]
  h = rnd((feats @ w_fc + b_fc).relu())
  r = rnd(rewards.reshape(N, 1).clamp(-1, 1))
  ins = rnd(instr_enc) if instr_enc is not None else torch.zeros(
      N, INSTR, dtype=torch.float64)
  return torch.cat([h, r, one_hot(actions, A), ins], 1)


def xproj(x, kernel, bias):
  """xw = x W_x + b_lstm, W_x = kernel[:f_in]."""
  return x @ kernel[:x.shape[1]] + bias


def w_h_of(kernel, f_in):
  return kernel[f_in:]


def recurrence_fwd(xw, done, c0, h0, w_h, mode):
  """Free-running recurrence: the fixed point of _lstm_oracle.forward.
  Returns {hs, cs, acts, hpm} in float64."""
  T, B, _ = xw.shape
  hs = torch.zeros(T, B, CORE, dtype=torch.float64)
  cs = torch.zeros_like(hs)
  for _ in range(T):
    ref = L.forward(xw, done, c0, h0, w_h, hs, cs, mode)
    hs, cs = ref['hs'][0], ref['cs'][0]
  out = {k: ref[k][0].double() for k in ('hs', 'cs', 'acts', 'hpm')}
  return out


def recurrence_bwd(g_hs, done, w_h, acts, cs, c0, g_c, mode):
  """Free-running backward: the fixed point of _lstm_oracle.backward.
  Returns (dG [T, B, 1024], dc0 [B, 256])."""
  T, B, H4 = acts.shape
  if g_hs is None:
    g_hs = torch.zeros(T, B, CORE, dtype=torch.float64)
  dg = torch.zeros(T, B, H4, dtype=torch.float64)
  for _ in range(T):
    ref = L.backward(g_hs, done, w_h, acts, cs, c0, g_c, dg, mode)
    dg = ref['dg'][0]
  return dg, ref['dc0'][0]


# ----------------------------------------------------------- backward layers

def dh_layer(dg, kernel, h):
  """dh = (dG W_x[:256]^T) * (h > 0)."""
  return (dg @ kernel[:CORE].t()) * (h > 0)


def dfeats_layer(dh, w_fc, feats=None):
  """dfeats = dh W_fc^T; with feats: times (feats > 0), the torso's final
  ReLU gradient, which the fp32 path applies here."""
  out = dh @ w_fc.t()
  return out if feats is None else out * (feats > 0)


def dw_h_layer(hpm, dg):
  return hpm.reshape(-1, CORE).t() @ dg


def dw_x_layer(x, dg):
  """[f_in, 1024]: every row of W_x, the instruction rows included."""
  return x.t() @ dg


def db_lstm_layer(dg):
  return dg.sum(0)


def dw_fc_layer(feats, dh):
  return feats.t() @ dh


def db_fc_layer(dh):
  return dh.sum(0)


def dh0_layer(dg0, w_h, done0):
  """dh0 = keep0 * dG[0] W_h^T."""
  return (done0.reshape(-1, 1) == 0).to(torch.float64) * (dg0 @ w_h.t())


def d_instr_layer(dg, kernel, c_instr, f_in):
  return dg @ kernel[c_instr:f_in].t()


# ----------------------------------------------------------------- the chain

LEAVES = ('feats', 'w_fc', 'b_fc', 'kernel', 'bias', 'instr_enc', 'c0', 'h0')


def forward_chain(inp, rnd=None, mode=0):
  """The whole core forward on draw()'s inputs.  Returns a record with x, xw
  [T, B, 1024], hs, cs, acts, hpm and the weights as used (w_fc, kernel: the
  model's, or with rnd the kernels' operands)."""
  r = rnd or _id
  T, B, f_in = inp['T'], inp['B'], inp['f_in']
  P = {k: (None if inp[k] is None else d64(inp[k])) for k in LEAVES}
  w_fc = r(P['w_fc'])
  kernel = P['kernel'].clone()
  kernel[:f_in] = r(kernel[:f_in])  # W_x; W_h is rounded by the gang alone
  x = fc_aug(P['feats'], w_fc, P['b_fc'], d64(inp['rewards']), inp['actions'],
             inp['A'], P['instr_enc'], r)
  xw = xproj(x, kernel, P['bias']).view(T, B, -1)
  done = inp['done'].to(torch.uint8)
  rec = recurrence_fwd(xw, done, P['c0'], P['h0'], w_h_of(kernel, f_in),
                       mode if rnd is not None else 0)
  rec.update(x=x, xw=xw, P=P, w_fc=w_fc, kernel=kernel, done=done,
             mode=mode if rnd is not None else 0, inp=inp)
  return rec


def backward_chain(rec, g_hs, g_c, rnd=None, mask_feats=False):
  """{leaf name: gradient} of sum(hs * g_hs) + sum(c_last * g_c) (either may
  be None).  mask_feats: dfeats times (feats > 0), the fp32 path's form."""
  r = rnd or _id
  inp, P, kernel = rec['inp'], rec['P'], rec['kernel']
  f_in, c_instr = inp['f_in'], inp['c_instr']
  w_h = w_h_of(kernel, f_in)
  dg, dc0 = recurrence_bwd(None if g_hs is None else d64(g_hs), rec['done'],
                           w_h, rec['acts'], rec['cs'], P['c0'],
                           None if g_c is None else d64(g_c), rec['mode'])
  N = dg.shape[0] * dg.shape[1]
  dg2 = dg.reshape(N, -1)
  dg16 = r(dg2)
  x = rec['x']
  dh = r(dh_layer(dg16, kernel, x[:, :CORE]))
  g = {}
  g['feats'] = r(dfeats_layer(dh, rec['w_fc'], P['feats'] if mask_feats else None))
  g['w_fc'] = dw_fc_layer(P['feats'], dh)
  g['b_fc'] = db_fc_layer(dh)
  g['kernel'] = torch.cat([dw_x_layer(x, dg16), dw_h_layer(rec['hpm'], dg2)], 0)
  g['bias'] = db_lstm_layer(dg2)
  g['instr_enc'] = (d_instr_layer(dg16, kernel, c_instr, f_in)
                    if inp['instr'] else None)
  g['c0'] = dc0
  g['h0'] = dh0_layer(dg[0], w_h, rec['done'][0])
  g['_dg'] = dg
  return g


def autograd_chain(inp, g_hs, g_c):
  """The exact chain under torch autograd (the layer functions above with
  _lstm_oracle.ref_lstm as the recurrence): (hs, c_last, {leaf: gradient},
  gradient of pre).  feats = relu(pre), so pre's gradient is the masked
  dfeats."""
  P = {k: d64(inp[k]).requires_grad_() for k in LEAVES if inp[k] is not None}
  pre = d64(inp['pre']).requires_grad_()
  feats = pre.relu()
  T, B, f_in = inp['T'], inp['B'], inp['f_in']
  x = fc_aug(feats, P['w_fc'], P['b_fc'], d64(inp['rewards']), inp['actions'],
             inp['A'], P.get('instr_enc'))
  xw = xproj(x, P['kernel'], P['bias']).view(T, B, -1)
  hs, cs, _ = L.ref_lstm(xw, inp['done'].to(torch.uint8), P['c0'], P['h0'],
                         w_h_of(P['kernel'], f_in))
  loss = 0.0
  if g_hs is not None:
    loss = loss + (hs * d64(g_hs)).sum()
  if g_c is not None:
    loss = loss + (cs[-1] * d64(g_c)).sum()
  names = [k for k in LEAVES if k in P and k != 'feats']
  got = torch.autograd.grad(loss, [P[k] for k in names] + [feats, pre])
  g = dict(zip(names + ['feats', 'pre'], got))
  g.setdefault('instr_enc', None)
  return hs.detach(), cs[-1].detach(), g


def rel_l2(a, ref):
  a, ref = d64(a), d64(ref)
  return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def cosine(a, ref):
  a, ref = d64(a).flatten(), d64(ref).flatten()
  return float(a @ ref / (a.norm() * ref.norm()).clamp_min(1e-300))
