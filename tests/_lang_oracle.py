"""Float64 one-step oracle of the instruction encoder (test helper).

Kernels under test: lang_lstm_fwd_kernel / lang_lstm_bwd_kernel
(csrc/kernels/lang_lstm.hip): embedding gather, LSTM(64) over the L words of
N instructions, the output at the last valid word, one launch per direction,
fp32 throughout.  As in tests/_lstm_oracle.py every step is checked alone,
fed the KERNEL's own saved tensors, so no bound grows with L:

  forward step t    operand xh[t] = [x_t (20) | h_{t-1} (64)] as the kernel
                    saved it, previous cell state cs[t-1] (0 at t = 0)
  backward step t   the kernel's acts, cs and dgates[t+1]
  dx[t]             the kernel's dgates[t]
  embedding scatter the kernel's dx (of the call without egrad)

Bitwise properties (no bound; compared with torch.equal or as bits):
  xh[t][:, :20] == embed[vid], vid = id if 0 <= id < V else 0;
  xh[0][:, 20:] == 0;  out[n] == xh[len_n][n, 20:] where 0 < len_n < L (the
  same registers stored twice);  out[n] == 0 where len_n == 0;  lengths are
  clamped to [0, L];  dgates[t] == 0 and dx[t] == 0 for t >= len_n (signed
  zeros allowed);  the forget-gate gradient at t = 0 is dc * 0 * ..., exactly
  zero: its bound below is 0 and it belongs to this class;  the fused call's
  dgates are the plain call's bits, its dx is empty, and embedding rows no
  valid word names keep the bits they had.

Bounds, derived, with u = 2^-24 (U, gamma and ACT_ULPS come from
_lstm_oracle):
  * pre = xh[t] @ K + b: the 84-term fp32 MFMA chain (21 steps of
    v_mfma_f32_16x16x4) errs by at most 84 u sum|a||b| in any order, the
    bias addition rounds once more: gamma_2 (|prod| + |b|); the forget gate
    takes one more rounding for its +1: u |pre_f|;
  * sigmoid is 1/4-Lipschitz, tanh 1-Lipschitz; products propagate by the
    float64 magnitudes; c_t = f c_{t-1} + i c~ rounds at most 3 times per
    term (gamma_3), h_t = o tanh(c_t) once more;
  * dh_rec = dgates[t+1] @ K[20:84]^T and dx[t] = dgates[t] @ K[:20]^T are
    256-term chains: 256 u sum|a||b|;  dh = [t == len-1] dout + dh_rec rounds
    once;
  * the carry dc runs as a float64 chain from the last valid step with the
    oracle's own dc_t; its error is the running sum
    e_carry[t] = e_dc[t] f_t + gamma_2 |carry[t]|,
    e_dc[t] = e_carry[t+1] + e_local[t] + u |dc_t|;
    the kernel recomputes tanh(c_t), which gets the activation term;
  * the gate gradients round 4 (i, o), 5 (f) times, and c~'s 1 - c~^2 adds
    gamma_2 |dc i| absolute (the subtraction can cancel), as in _lstm_oracle;
  * the embedding gradient of row v is prefill + count_v atomic additions in
    a free order: (count_v + 1) u (|prefill| + sum|dx|);
  * one term cannot be derived: the intrinsic error of the __expf-based
    sigmoid and of tanhf.  lang_lstm.hip uses the same two functions as
    lstm.hip, so ACT_ULPS measured there (_lstm_oracle.ACT_MEASURED, 2 x
    allowed) applies.  tests/test_lang_lstm_oracle_gpu.py::
    test_activation_constant measures it again on this kernel's L = 1 case
    and holds it to ACT_ULPS; measured there in units of u by gate:
    LANG_ACT_MEASURED below.

The encoder is fp32 throughout: there is no near-tie exclusion, every element
of every compared tensor is held to its bound (verify()).  A NaN counts as
beyond any bound.

CASES is the table both tests/test_lang_oracle.py (an fp32 emulation of the
kernel on the CPU, with planted faults) and the GPU tests walk.
"""

import torch

from tests._lstm_oracle import ACT_ULPS, U, gamma

E, H, G, XH = 20, 64, 256, 84
ROWS = 16  # instructions per workgroup

# |kernel - float64| / u over the gate outputs of ACT_CASE (L = 1) on an
# MI355X (test_activation_constant) by gate: i 1.549, c~ 3.745, f 1.662,
# o 1.654 - within ACT_ULPS = 6.17, which therefore stays as borrowed
LANG_ACT_MEASURED = 3.745

NS = (1, 15, 16, 17, 33, 48)
LS = (1, 2, 5, 16)
LEN_PATTERNS = ('zero', 'full', 'rand', 'beyond', 'block')
ID_PATTERNS = ('rand', 'edge', 'same')


def _cases():
  """Every N meets every length pattern once ('block' needs a second
  workgroup: N >= 17), with L walking LS so that every L meets every pattern
  too; ids alternate between in-range and out-of-range words.  Then: the
  L = 5 block case in the other order, one vocabulary of a single word, every
  word the same id (the heaviest atomic collisions) on a full and a ragged
  length pattern."""
  out = []
  for ip, pat in enumerate(LEN_PATTERNS):
    for i_n, n in enumerate(NS):
      if pat == 'block' and n < 17:
        continue
      out.append(dict(N=n, L=LS[(i_n + ip) % 4], V=1000, lens=pat,
                      ids=ID_PATTERNS[(i_n + ip) % 2]))
  out.append(dict(N=48, L=5, V=1000, lens='block', ids='edge', flip=True))
  out.append(dict(N=17, L=5, V=1, lens='rand', ids='edge'))
  out.append(dict(N=48, L=16, V=1000, lens='full', ids='same'))
  out.append(dict(N=33, L=5, V=1000, lens='rand', ids='same'))
  for k, c in enumerate(out):
    c.setdefault('flip', False)
    c['seed'] = 1000 + k
    c['name'] = 'N%d-L%d-V%d-%s-%s%s' % (c['N'], c['L'], c['V'], c['lens'], c['ids'],
                                        '-flip' if c['flip'] else '')
  return out


CASES = _cases()
ACT_CASE = dict(N=48, L=1, V=1000, lens='full', ids='rand', flip=False, seed=999,
                name='N48-L1-activation')


def draw(case):
  """The inputs of a case on the CPU from its seed.  embed ~ N(0, 1),
  K ~ 0.2 N(0, 1), b ~ 0.5 N(0, 1): pre-activations of standard deviation
  about 1.2, |pre| below 8 like the LSTM oracle's cases (printed by the
  tests)."""
  N, L, V = case['N'], case['L'], case['V']
  gen = torch.Generator().manual_seed(case['seed'])
  rn = lambda *s: torch.randn(*s, generator=gen)
  ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=gen)
  inp = {
      'embed': rn(V, E),
      'kernel': rn(XH, G) * 0.2,
      'bias': rn(G) * 0.5,
      'dout': rn(N, H),
      'prefill': rn(V, E) + 3.0,
  }
  pat = case['lens']
  if pat == 'zero':
    lens = torch.zeros(N, dtype=torch.int64)
  elif pat == 'full':
    lens = torch.full((N,), L, dtype=torch.int64)
  elif pat == 'rand':
    lens = ri(0, L + 1, N)
    if N >= 2:  # both ends present
      lens[N // 2] = 0
      lens[N - 1] = L
  elif pat == 'beyond':
    lens = ri(0, L + 1, N)
    past = torch.tensor([L + 1, -1, 2 * L + 3, -(2 ** 40), 2 ** 40, L, 0])
    lens[::2] = past[torch.arange(lens[::2].numel()) % past.numel()]
  else:  # one whole 16-row block empty next to a full one
    lens = ri(0, L + 1, N)
    lens[:ROWS] = L if case['flip'] else 0
    lens[ROWS:2 * ROWS] = 0 if case['flip'] else L
  inp['lengths'] = lens
  pat = case['ids']
  if pat == 'same':
    ids = torch.full((N, L), 7 % V, dtype=torch.int64)
  else:
    ids = ri(0, V, N, L)
    flat = ids.view(-1)
    where = torch.randperm(N * L, generator=gen)
    vals = [0, V - 1] if pat == 'rand' else [V, -1, 2 ** 40, 0, V - 1, V + 5, -(2 ** 40)]
    for k in range(min(N * L, 2 * len(vals))):
      flat[where[k]] = vals[k % len(vals)]
  inp['ids'] = ids
  return inp


def clamp_lengths(lengths, L):
  return lengths.clamp(0, L)


def valid_ids(ids, V):
  """[N, L] -> the embedding row each word reads: out-of-range ids read row 0."""
  return torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids))


def _prev0(seq):
  return torch.cat([torch.zeros_like(seq[:1]), seq[:-1]])


def invariants(inp, xh):
  """The bitwise forward properties: reference values only.
  x [L, N, 20]: embed rows of the words; lens [N]: clamped lengths;
  out_rows / out_vals: rows with 0 < len < L and the xh[len][n, 20:] their
  out must equal; zero_rows: rows whose out is 0."""
  L, N = xh.shape[0], xh.shape[1]
  V = inp['embed'].shape[0]
  lens = clamp_lengths(inp['lengths'], L)
  x = inp['embed'][valid_ids(inp['ids'], V).t()]
  rows = torch.nonzero((lens > 0) & (lens < L)).view(-1)
  return {
      'x': x,
      'lens': lens,
      'out_rows': rows,
      'out_vals': xh[lens[rows], rows, E:],
      'zero_rows': torch.nonzero(lens == 0).view(-1),
  }


def forward(inp, xh, cs):
  """One-step forward oracle of every step t from the given xh [L, N, 84] and
  cs [L, N, 64].  Returns {name: (float64 reference, bound)} for acts, cs and
  hs (h_t of every step), and 'pre' (reference only)."""
  k, b = inp['kernel'].double(), inp['bias'].double()
  a = xh.double()
  cp = _prev0(cs.double())
  prod = a @ k
  mag = a.abs() @ k.abs()
  fb = torch.zeros(G, dtype=torch.float64)
  fb[2 * H:3 * H] = 1.0
  pre = prod + b + fb
  e_pre = XH * U * mag + gamma(2) * (prod.abs() + b.abs()) + fb * U * pre.abs()
  pi, pg, pf, po = pre.split(H, -1)
  ei, eg, ef, eo = e_pre.split(H, -1)
  act = ACT_ULPS * U
  i, g, f, o = torch.sigmoid(pi), torch.tanh(pg), torch.sigmoid(pf), torch.sigmoid(po)
  ei, eg, ef, eo = ei / 4 + act, eg + act, ef / 4 + act, eo / 4 + act
  c = f * cp + i * g
  e_c = (ef * cp.abs() + ei * g.abs() + eg * i.abs() + ei * eg +
         gamma(3) * ((f * cp).abs() + (i * g).abs()))
  tc = torch.tanh(c)
  e_tc = e_c + act
  h = o * tc
  e_h = eo * tc.abs() + o * e_tc + eo * e_tc + U * h.abs()
  return {
      'acts': (torch.cat([i, g, f, o], -1), torch.cat([ei, eg, ef, eo], -1)),
      'cs': (c, e_c),
      'hs': (h, e_h),
      'pre': (pre, None),
  }


def backward(inp, acts, cs, dgates):
  """One-step backward oracle of every step t: the recurrent term comes from
  the given dgates[t+1], the carry runs in float64 from the last valid step.
  Returns {'dg': (ref, bound), 'dx': (ref, bound), 'valid': [L, N, 1] bool};
  reference and bound are 0 where t >= len."""
  L, N = acts.shape[0], acts.shape[1]
  k = inp['kernel'].double()
  lens = clamp_lengths(inp['lengths'], L).view(1, N, 1)
  t_idx = torch.arange(L).view(L, 1, 1)
  valid = t_idx < lens
  vf = valid.double()
  last = (t_idx == lens - 1).double()
  i, g, f, o = acts.double().split(H, -1)
  cp = _prev0(cs.double())
  d = dgates.double()
  zero = torch.zeros(1, N, H, dtype=torch.float64)
  kr = k[E:]
  rec = torch.cat([d[1:] @ kr.t(), zero])
  e_rec = torch.cat([G * U * (d[1:].abs() @ kr.abs().t()), zero])
  dh = last * inp['dout'].double().view(1, N, H) + rec
  e_dh = e_rec + U * dh.abs()
  tc = torch.tanh(cs.double())
  e_tc = ACT_ULPS * U
  s = 1.0 - tc * tc
  loc = dh * o * s
  e_s = 2.0 * tc.abs() * e_tc + gamma(2)
  e_loc = e_dh * (o * s).abs() + (dh * o).abs() * e_s + gamma(2) * loc.abs()
  fk = f * vf
  dc, e_dc = torch.empty_like(loc), torch.empty_like(loc)
  carry = torch.zeros(N, H, dtype=torch.float64)
  e_carry = torch.zeros(N, H, dtype=torch.float64)
  for t in range(L - 1, -1, -1):
    dc[t] = vf[t] * (carry + loc[t])
    e_dc[t] = vf[t] * (e_carry + e_loc[t] + U * dc[t].abs())
    carry = dc[t] * fk[t]
    e_carry = e_dc[t] * fk[t] + gamma(2) * carry.abs()
  dhv, e_dhv = dh * vf, e_dh * vf
  gi = dc * g * i * (1.0 - i)
  gg = dc * i * (1.0 - g * g)
  gf = dc * cp * f * (1.0 - f)
  go = dhv * tc * o * (1.0 - o)
  e_gi = e_dc * (g * i * (1.0 - i)).abs() + gamma(4) * gi.abs()
  e_gg = (e_dc * (i * (1.0 - g * g)).abs() + gamma(2) * (dc * i).abs() +
          gamma(2) * gg.abs())
  e_gf = e_dc * (cp * f * (1.0 - f)).abs() + gamma(5) * gf.abs()
  e_go = (e_dhv * (tc * o * (1.0 - o)).abs() + (dhv * o * (1.0 - o)).abs() * e_tc +
          gamma(4) * go.abs())
  kx = k[:E]
  return {
      'dg': (torch.cat([gi, gg, gf, go], -1), torch.cat([e_gi, e_gg, e_gf, e_go], -1)),
      'dx': (d @ kx.t(), G * U * (d.abs() @ kx.abs().t())),
      'valid': valid,
  }


def scatter(inp, dx, prefill=None):
  """Embedding gradient from the given dx [L, N, 20]: (reference, bound,
  count [V]); rows with count 0 keep their prefill bitwise."""
  L, N = dx.shape[0], dx.shape[1]
  V = inp['embed'].shape[0]
  pre = (inp['prefill'] if prefill is None else prefill).double()
  lens = clamp_lengths(inp['lengths'], L)
  valid = (torch.arange(L).view(L, 1) < lens.view(1, N)).reshape(-1)
  vid = valid_ids(inp['ids'], V).t().reshape(-1)[valid]
  rows = dx.double().reshape(L * N, E)[valid]
  ref = pre.clone().index_add_(0, vid, rows)
  mag = pre.abs().index_add_(0, vid, rows.abs())
  count = torch.zeros(V, dtype=torch.float64).index_add_(0, vid, torch.ones(vid.numel(), dtype=torch.float64))
  return ref, (count + 1.0).view(V, 1) * U * mag, count


def ref_encoder(inp, dtype=torch.float64):
  """Free-running encoder in `dtype` (autograd-friendly), the recurrence of
  models/agent.py's generic path written out: returns a dict with out and
  the per-step xh, pre (leaves of the graph with retained gradients), acts,
  cs, and x (the gathered embedding rows, gradient retained)."""
  L = inp['ids'].shape[1]
  N = inp['ids'].shape[0]
  emb = inp['embed'].to(dtype).clone().requires_grad_()
  k = inp['kernel'].to(dtype).clone().requires_grad_()
  b = inp['bias'].to(dtype).clone().requires_grad_()
  lens = clamp_lengths(inp['lengths'], L)
  vid = valid_ids(inp['ids'], emb.shape[0])
  c = torch.zeros(N, H, dtype=dtype)
  h = torch.zeros(N, H, dtype=dtype)
  out = torch.zeros(N, H, dtype=dtype)
  xs, xhs, pres, acts, cs = [], [], [], [], []
  for t in range(L):
    x = emb[vid[:, t]]
    x.retain_grad()
    xh = torch.cat([x, h], -1)
    pre = xh @ k + b
    pre.retain_grad()
    i, g, f, o = pre.chunk(4, -1)
    i, g, f, o = torch.sigmoid(i), torch.tanh(g), torch.sigmoid(f + 1.0), torch.sigmoid(o)
    c = g * i + c * f
    h = torch.tanh(c) * o
    out = torch.where((lens - 1 == t).unsqueeze(-1), h, out)
    xs.append(x)
    xhs.append(xh)
    pres.append(pre)
    acts.append(torch.cat([i, g, f, o], -1))
    cs.append(c)
  return {'out': out, 'x': xs, 'xh': xhs, 'pre': pres, 'acts': acts, 'cs': cs,
          'embed': emb, 'kernel': k, 'bias': b}


# ------------------------------------------------------------- fp32 emulation
FAULTS = ('swap_fo', 'no_forget_bias', 'xh_holds_ht', 'out_at_len', 'no_clamp',
          'oor_id_last_row', 'cp_at_t0', 'no_zero_past_len', 'dout_neighbour',
          'egrad_overwrite', 'skip_last_partial_row')


def fault_hits(fault, case, inp):
  """Whether a planted fault must show at this case (the table's cases that
  name it)."""
  N, L, V = case['N'], case['L'], case['V']
  lens = clamp_lengths(inp['lengths'], L)
  some_word = bool((lens > 0).any())
  if fault in ('swap_fo', 'no_forget_bias', 'xh_holds_ht'):
    return True
  if fault in ('out_at_len', 'cp_at_t0', 'egrad_overwrite'):
    return some_word
  if fault == 'no_clamp':
    return bool((inp['lengths'] > L).any())
  if fault == 'oor_id_last_row':
    return V > 1 and bool(((inp['ids'] < 0) | (inp['ids'] >= V)).any())
  if fault == 'no_zero_past_len':
    return bool((lens < L).any())
  if fault == 'dout_neighbour':
    return N > 1 and some_word
  if fault == 'skip_last_partial_row':
    return N % ROWS != 0
  raise KeyError(fault)


def emulate(inp, fault=None):
  """The two kernels' arithmetic in float32 torch on the CPU, step by step in
  the kernels' structure (outputs start as NaN = never written).  Returns the
  dict verify() takes.  fault: one of FAULTS, planted."""
  f32 = torch.float32
  ids, lengths = inp['ids'], inp['lengths']
  N, L = ids.shape
  emb, k, b, dout = inp['embed'], inp['kernel'], inp['bias'], inp['dout']
  V = emb.shape[0]
  nan = lambda *s: torch.full(s, float('nan'), dtype=f32)
  lens = lengths if fault == 'no_clamp' else clamp_lengths(lengths, L)
  inr = (ids >= 0) & (ids < V)
  vid = torch.where(inr, ids, torch.full_like(ids, V - 1 if fault == 'oor_id_last_row' else 0))
  out, acts, cs, xh = nan(N, H), nan(L, N, G), nan(L, N, H), nan(L, N, XH)
  c = torch.zeros(N, H)
  h = torch.zeros(N, H)
  o_at = lens if fault == 'out_at_len' else lens - 1
  for t in range(L):
    x = emb[vid[:, t]]
    row = torch.cat([x, h], -1)
    pre = row @ k + b
    pi, pg, pf, po = pre.split(H, -1)
    if fault == 'swap_fo':
      pf, po = po, pf
    i, g, o = torch.sigmoid(pi), torch.tanh(pg), torch.sigmoid(po)
    f = torch.sigmoid(pf if fault == 'no_forget_bias' else pf + 1.0)
    c = f * c + i * g
    h = o * torch.tanh(c)
    xh[t] = torch.cat([x, h], -1) if fault == 'xh_holds_ht' else row
    acts[t] = torch.cat([i, g, f, o], -1)
    cs[t] = c
    sel = o_at == t
    out[sel] = h[sel]
  out[lens <= 0] = 0.0
  # backward
  dg, dx = nan(L, N, G), nan(L, N, E)
  dcar = torch.zeros(N, H)
  dr = torch.zeros(N, H)
  dsrc = dout.roll(-1, 0) if fault == 'dout_neighbour' else dout
  blens = torch.full_like(lens, L) if fault == 'no_zero_past_len' else lens
  for t in range(L - 1, -1, -1):
    ok = (t < blens).view(N, 1)
    dh = torch.where((blens - 1 == t).view(N, 1), dsrc, torch.zeros(N, H)) + dr
    i, g, f, o = acts[t].split(H, -1)
    ct = cs[t]
    if t > 0:
      cp = cs[t - 1]
    else:
      cp = cs[L - 1] if fault == 'cp_at_t0' else torch.zeros(N, H)
    tc = torch.tanh(ct)
    dc = dcar + dh * o * (1.0 - tc * tc)
    step = torch.cat([dc * g * i * (1.0 - i), dc * i * (1.0 - g * g),
                      dc * cp * f * (1.0 - f), dh * tc * o * (1.0 - o)], -1)
    dg[t] = torch.where(ok, step, torch.zeros(N, G))
    dcar = torch.where(ok, dc * f, torch.zeros(N, H))
    both = dg[t] @ k.t()
    dx[t], dr = both[:, :E], both[:, E:]
  skip = fault == 'skip_last_partial_row' and N % ROWS != 0
  if skip:
    for x in (out, acts, cs, xh, dg, dx):
      x[..., N - 1, :] = float('nan')
  # the fused call: the valid words' dx rows into the prefilled table
  egrad = inp['prefill'].clone()
  word = torch.arange(L).view(L, 1) < lens.view(1, N)
  if skip:
    word[:, N - 1] = False
  if fault == 'egrad_overwrite':
    for t, n in torch.nonzero(word).tolist():
      egrad[vid[n, t]] = dx[t, n]
  else:
    egrad.index_add_(0, vid.t()[word], dx[word])
  return {'out': out, 'acts': acts, 'cs': cs, 'xh': xh, 'dg': dg, 'dx': dx,
          'dg_fused': dg.clone(), 'dx_fused': torch.empty(0), 'egrad': egrad}


# ------------------------------------------------------------------ the check
def bits(x):
  return x.contiguous().view(torch.int32)


def same_bits(a, b):
  return a.shape == b.shape and torch.equal(bits(a), bits(b))


def verify(inp, got):
  """Every check of one case on CPU tensors.  got: out, acts, cs, xh of
  lang_lstm_fwd; dg, dx of lang_lstm_bwd without egrad; dg_fused, dx_fused of
  the call with ids and egrad = prefill, egrad afterwards.  Returns
  (failures: list of str, stats: {name: largest error / bound}, max |pre|)."""
  fails, stats = [], {}
  xh, cs, acts, out = got['xh'], got['cs'], got['acts'], got['out']
  L, N = xh.shape[0], xh.shape[1]

  def held(name, val, ref, bound, mask=None):
    err = (val.double() - ref).abs()
    okay = err <= bound  # a NaN is never within
    if mask is not None:
      okay = okay | ~mask
      err = torch.where(mask, err, torch.zeros_like(err))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.nan_to_num(ratio, nan=float('inf'))
    stats[name] = max(stats.get(name, 0.0), float(ratio.max()) if ratio.numel() else 0.0)
    bad = int((~okay).sum())
    if bad:
      fails.append('%s: %d elements beyond the bound (worst ratio %g)' % (name, bad, stats[name]))

  def exact(name, cond):
    if not cond:
      fails.append(name)

  inv = invariants(inp, xh)
  lens = inv['lens']
  exact('xh[:, :, :20] is the embedding row of the word', same_bits(xh[..., :E], inv['x']))
  exact('xh[0][:, 20:] is zero', torch.equal(xh[0, :, E:], torch.zeros(N, H)))
  exact('out is xh[len][:, 20:] where 0 < len < L',
        same_bits(out[inv['out_rows']], inv['out_vals']))
  exact('out is zero for an empty instruction',
        torch.equal(out[inv['zero_rows']], torch.zeros(inv['zero_rows'].numel(), H)))
  fwd = forward(inp, xh, cs)
  held('acts', acts, *fwd['acts'])
  held('cs', cs, *fwd['cs'])
  h_ref, e_h = fwd['hs']
  if L > 1:
    held('h', xh[1:, :, E:], h_ref[:-1], e_h[:-1])
  rows = torch.nonzero(lens > 0).view(-1)
  held('out', out[rows], h_ref[lens[rows] - 1, rows], e_h[lens[rows] - 1, rows])

  bwd = backward(inp, acts, cs, got['dg'])
  valid = bwd['valid']
  vg, vx = valid.expand(L, N, G), valid.expand(L, N, E)
  held('dgates', got['dg'], *bwd['dg'], mask=vg)
  exact('dgates is zero past the length',
        torch.equal(got['dg'][~vg], torch.zeros(int((~vg).sum()))))
  held('dx', got['dx'], *bwd['dx'])
  exact('dx is zero past the length',
        got['dx'].shape == (L, N, E) and
        torch.equal(got['dx'][~vx], torch.zeros(int((~vx).sum()))))

  exact('fused dgates are the plain call\'s bits', same_bits(got['dg_fused'], got['dg']))
  exact('fused dx comes back empty', got['dx_fused'].numel() == 0)
  ref, bound, count = scatter(inp, got['dx'])
  named = count > 0
  held('egrad', got['egrad'][named], ref[named], bound[named])
  exact('embedding rows no word names keep their bits',
        same_bits(got['egrad'][~named], inp['prefill'][~named]))
  return fails, stats, float(fwd['pre'][0].abs().max())


def bounds_of(inp, got):
  """Every bound of a case, flattened by name, for the oracle's own checks:
  {name: bound tensor restricted to the elements that are not bitwise}."""
  L = got['xh'].shape[0]
  fwd = forward(inp, got['xh'], got['cs'])
  bwd = backward(inp, got['acts'], got['cs'], got['dg'])
  valid = bwd['valid']
  e_dg = bwd['dg'][1]
  gi, gg, gf, go = e_dg.split(H, -1)
  v = valid.expand(gi.shape)
  _, e_sc, count = scatter(inp, got['dx'])
  return {
      'acts': fwd['acts'][1], 'cs': fwd['cs'][1], 'hs': fwd['hs'][1],
      'dg_i': gi[v], 'dg_c': gg[v], 'dg_o': go[v],
      'dg_f': gf[1:][v[1:]] if L > 1 else gf[:0],  # df[0] = dc * 0: bitwise
      'dx': bwd['dx'][1][valid.expand(bwd['dx'][1].shape)],
      'egrad': e_sc[count > 0],
  }
