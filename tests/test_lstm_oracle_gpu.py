"""Float64 one-step oracle tests of the LSTM recurrences at their edges.

Kernels under test, through the raw bindings with an explicit mode:
lstm_fwd_step_kernel / lstm_bwd_step_kernel / lstm_pack_weights_kernel
(lstm.hip, mode 0), lstm_*_persistent_kernel (lstm_persistent.hip, mode 1),
lstm_*_gang_kernel and their wave-specialised variants (lstm_gang.hip, mode 2
with lstm_gang_ws 0 / 1).  Every step is compared with tests/_lstm_oracle.py:
float64 fed the kernel's own previous outputs, with derived bounds (module
docstring there).  Inputs are drawn on the CPU from fixed seeds and copied to
the device, so oracle and kernel read identical bits.  Each check prints
error / bound; the module prints the largest ratio per mode and output when
it finishes (pytest -s).

Case -> branch:

  batch edges, mode 0, H = 256, T = 3
    B = 1, 15, 16, 17, 31      partly filled 16-row workgroups, clamped loads
    B = 32, 48                 full tiles; 48 = three workgroups, half of the
                               second packed 32-row tile uninitialised
    B = 33, 65                 one live row in a fresh packed tile
    B = 76                     the inference board's rows
  H = 64, B = 1, 17, 33        the 32-row kernels
  batch edges, modes 1, 2 (ws 0 / 1), T = 4, B = 1 .. 32: live-row masks
  T = 101, B = 32              every mode, the learner's unroll
  done rows (B = 17, 32)       never / always / t = 0 / T-1 / t = 1 /
                               alternating, side by side in one batch
  two chained chunks           dc_last given against None, state hand-off
  B = 17 in 32, 33 in 64       row independence, bitwise
  lstm_xpack 1, 3, 8           which blocks work; bitwise the default's
  prepacked w4 (T = 1)         the actor step; B = 1, 16, 76, 150
"""

import pytest
import torch

from tests import _lstm_oracle as O

pytestmark = pytest.mark.gpu

# (mode, lstm_gang_ws): per-step, persistent, gang, wave-specialised gang
VARIANTS = [(0, 0), (1, 0), (2, 0), (2, 1)]
WHOLE = VARIANTS[1:]
FWD = ('hs', 'cs', 'acts', 'hpm')
BWD = ('dg', 'dc0', 'dg16')

_WORST = {}
_SHARES = {}


def _C():
  from scalable_agent_amd import ops
  ops.load()
  return ops.ext()


def _err_clear(dev):
  from scalable_agent_amd.ops import lstm as lstm_ops
  assert lstm_ops.persistent_error(dev) == 0


def _bits(x):
  return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def _same(a, b, what):
  assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _fwd(dev, inp, mode, ws=0, w4=None):
  C = _C()
  d = {k: inp[k].to(dev) for k in ('xw', 'done', 'c0', 'h0', 'w_h')}
  prev = C.lstm_gang_ws(ws)
  try:
    args = (d['xw'], d['done'], d['c0'], d['h0'], d['w_h'], mode)
    outs = C.lstm_fwd(*args) if w4 is None else C.lstm_fwd(*args, w4)
  finally:
    C.lstm_gang_ws(prev)
  if mode:
    _err_clear(dev)
  out = dict(zip(FWD, (o.cpu() for o in outs[:4])))
  out['wt'] = outs[4]
  return out


def _bwd(dev, inp, fwd, mode, ws=0, dc_last=True, want_bf16=True, dh=None):
  """Backward on the kernel's own forward outputs (teacher forcing)."""
  C = _C()
  dh = inp['dh'] if dh is None else dh
  dcl = inp['dcl'].to(dev) if dc_last else None
  prev = C.lstm_gang_ws(ws)
  try:
    outs = C.lstm_bwd(dh.to(dev), inp['done'].to(dev), fwd['wt'], fwd['acts'].to(dev),
                      fwd['cs'].to(dev), inp['c0'].to(dev), dcl, want_bf16, mode)
  finally:
    C.lstm_gang_ws(prev)
  if mode:
    _err_clear(dev)
  return dict(zip(BWD, (o.cpu() for o in outs)))


def _held(key, name, got, ref, bound):
  err = (got.double() - ref).abs()
  ratio = float((err / bound.clamp_min(1e-300)).max())
  print('  %-5s mode %d ws %d  max err %.3e  err/bound %.4f' %
        (name, key[0], key[1], float(err.max()), ratio))
  _WORST[key + (name,)] = max(_WORST.get(key + (name,), 0.0), ratio)
  bad = int((err > bound).sum())
  assert bad == 0, '%s: %d elements beyond the bound, worst ratio %g' % (name, bad, ratio)


def _check_fwd(inp, out, mode, ws):
  ref = O.forward(inp['xw'], inp['done'], inp['c0'], inp['h0'], inp['w_h'],
                  out['hs'], out['cs'], mode)
  for name in ('acts', 'cs', 'hs'):
    _held((mode, ws), name, out[name], *ref[name])
  _same(out['hpm'], ref['hpm'][0], 'hpm is keep * h_prev bitwise')
  return ref


def _check_bwd(inp, fwd, out, mode, ws, dc_last=True, case=None):
  ref = O.backward(inp['dh'], inp['done'], inp['w_h'], fwd['acts'], fwd['cs'],
                   inp['c0'], inp['dcl'] if dc_last else None, out['dg'], mode)
  _held((mode, ws), 'dg', out['dg'], *ref['dg'])
  _held((mode, ws), 'dc0', out['dc0'], *ref['dc0'])
  _same(out['dg16'], out['dg'].to(torch.bfloat16), 'dg16 is RNE bf16 of dg')
  assert torch.equal(out['dg16'].double(), O.bf16_rne(out['dg']))
  if mode == 2:
    print('  near-tie element share %.3f' % ref['tie_share'])
    if case is not None:
      _SHARES[(ws,) + case] = ref['tie_share']
    assert ref['tie_share'] <= O.MAX_TIE_SHARE
  return ref


def _full(dev, inp, mode, ws, case=None):
  """Forward and backward against the oracle; want_bf16 off against on."""
  fwd = _fwd(dev, inp, mode, ws)
  _check_fwd(inp, fwd, mode, ws)
  bwd = _bwd(dev, inp, fwd, mode, ws)
  _check_bwd(inp, fwd, bwd, mode, ws, case=case)
  plain = _bwd(dev, inp, fwd, mode, ws, want_bf16=False)
  _same(plain['dg'], bwd['dg'], 'dg with and without the bf16 copy')
  _same(plain['dc0'], bwd['dc0'], 'dc0 with and without the bf16 copy')
  assert plain['dg16'].numel() == 0
  return fwd, bwd


@pytest.fixture(scope='module', autouse=True)
def _report():
  yield
  for key in sorted(_WORST):
    print('\nlargest err/bound  mode %d ws %d  %-5s %.4f' % (key + (_WORST[key],)), end='')
  for key in sorted(_SHARES):
    print('\nnear-tie share  ws %d T %d B %d  %.3f' % (key + (_SHARES[key],)), end='')
  print()


def test_activation_constant(cuda):
  """The measured term of the bounds: |kernel - float64| / 2^-24 over the
  gate outputs of the step-mode T = 1 case stays within the recorded
  measurement's allowance (2 x ACT_MEASURED)."""
  inp = O.draw(100, 1, 32, 256)
  out = _fwd(cuda, inp, 0)
  ref = O.forward(inp['xw'], inp['done'], inp['c0'], inp['h0'], inp['w_h'],
                  out['hs'], out['cs'], 0)
  ulps = (out['acts'].double() - ref['acts'][0]).abs() / O.U
  per_gate = [float(x.max()) for x in ulps.split(256, -1)]
  print('  activation error in 2^-24 units: i %.3f g %.3f f %.3f o %.3f' % tuple(per_gate))
  assert max(per_gate) <= O.ACT_ULPS


@pytest.mark.parametrize('H,B', [(256, b) for b in (1, 15, 16, 17, 31, 32, 33, 48, 65, 76)] +
                         [(64, b) for b in (1, 17, 33)])
def test_batch_edges_step(cuda, H, B):
  _full(cuda, O.draw(200 + B, 3, B, H), 0, 0)


@pytest.mark.parametrize('B', [1, 15, 16, 17, 31, 32])
@pytest.mark.parametrize('mode,ws', WHOLE)
def test_batch_edges_whole_unroll(cuda, mode, ws, B):
  _full(cuda, O.draw(300 + B, 4, B, 256), mode, ws, case=(4, B))


@pytest.mark.parametrize('mode,ws', VARIANTS)
def test_long_unroll(cuda, mode, ws):
  """T = 101: the forward holds the one-step bound at every step; the
  backward holds the bound accumulated along the float64 carry chain, which
  is the one-step bound plus a running sum damped by f keep <= 1."""
  _full(cuda, O.draw(400, 101, 32, 256), mode, ws, case=(101, 32))


def _done_rows(T, B):
  """Row r follows pattern r % 6: never done, always, only t = 0, only
  t = T-1, only t = 1, alternating (even t)."""
  done = torch.zeros(T, B, dtype=torch.bool)
  r = torch.arange(B)
  done[:, r % 6 == 1] = True
  done[0, r % 6 == 2] = True
  done[T - 1, r % 6 == 3] = True
  done[1, r % 6 == 4] = True
  done[0::2, r % 6 == 5] = True
  return done


@pytest.mark.parametrize('B', [17, 32])
@pytest.mark.parametrize('mode,ws', VARIANTS)
def test_done_rows(cuda, mode, ws, B):
  T = 5
  done = _done_rows(T, B)
  inp = O.draw(500 + B, T, B, 256, done=done)
  fwd, bwd = _full(cuda, inp, mode, ws, case=(T, B))
  rows = torch.arange(B)
  # signed zeros allowed: the kernels multiply keep = 0 into h_prev
  assert float(fwd['hpm'][:, rows % 6 == 1].abs().max()) == 0.0
  assert float(bwd['dc0'][done[0]].abs().max()) == 0.0
  assert float(bwd['dc0'][~done[0]].abs().min()) > 0.0
  # a row done at t + 1 takes no recurrent term at t: moving its later
  # dh_out must leave its dG[:t + 1] and dc0 bit for bit
  for t in range(T - 1):
    sel = done[t + 1]
    dh = inp['dh'].clone()
    dh[t + 1:, sel] += 1.0
    moved = _bwd(cuda, inp, fwd, mode, ws, dh=dh)
    assert not torch.equal(moved['dg'][t + 1:, sel], bwd['dg'][t + 1:, sel])
    _same(moved['dg'][:t + 1, sel], bwd['dg'][:t + 1, sel], 'dG[:%d] of done rows' % (t + 1))
    _same(moved['dc0'][sel], bwd['dc0'][sel], 'dc0 of done rows')
    _same(moved['dg'][:, ~sel], bwd['dg'][:, ~sel], 'other rows')


@pytest.mark.parametrize('mode,ws', VARIANTS)
def test_chained_chunks(cuda, mode, ws):
  """Two time chunks: the forward state goes through hs[-1] / cs[-1], the
  second chunk's dc0 is the first's dc_last and its dh0 (host float64) joins
  the first's last dh_out.  The pieces together hold the whole unroll's
  oracle, whose step a - 1 takes its recurrent term from dh_out (cuts)."""
  T, a, B, H = 6, 3, 17, 256
  inp = O.draw(600, T, B, H)
  inp['done'][a, 2] = 1  # a row reset exactly at the chunk boundary
  part = lambda d, lo, hi: dict(d, xw=d['xw'][lo:hi], done=d['done'][lo:hi], dh=d['dh'][lo:hi])
  in1 = part(inp, 0, a)
  f1 = _fwd(cuda, in1, mode, ws)
  in2 = dict(part(inp, a, T), c0=f1['cs'][-1], h0=f1['hs'][-1])
  f2 = _fwd(cuda, in2, mode, ws)
  whole = {k: torch.cat([f1[k], f2[k]]) for k in FWD}
  _check_fwd(inp, whole, mode, ws)
  # the whole unroll carries no final-state gradient: None == zeros, bitwise
  b2 = _bwd(cuda, in2, f2, mode, ws, dc_last=False)
  z2 = _bwd(cuda, dict(in2, dcl=torch.zeros(B, H)), f2, mode, ws)
  for k in BWD:
    _same(b2[k], z2[k], 'dc_last None against zeros: ' + k)
  keep = (inp['done'][a] == 0).double().unsqueeze(-1)
  dh0 = keep * (b2['dg'][0].double() @ inp['w_h'].double().t())
  dh = inp['dh'].clone()
  dh[a - 1] = (dh[a - 1].double() + dh0).float()
  in1 = dict(in1, dh=dh[:a], dcl=b2['dc0'])
  b1 = _bwd(cuda, in1, f1, mode, ws)
  dg = torch.cat([b1['dg'], b2['dg']])
  ref = O.backward(dh, inp['done'], inp['w_h'], whole['acts'], whole['cs'], inp['c0'],
                   None, dg, mode, cuts=(a - 1,))
  _held((mode, ws), 'dg', dg, *ref['dg'])
  _held((mode, ws), 'dc0', b1['dc0'], *ref['dc0'])
  assert ref['tie_share'] <= O.MAX_TIE_SHARE


@pytest.mark.parametrize('mode,ws,B,BB', [(m, w, 17, 32) for m, w in VARIANTS] + [(0, 0, 33, 64)])
def test_row_independence(cuda, mode, ws, B, BB):
  """Rows [0, B) of a B-row run equal the same rows of a BB-row run on the
  same data bit for bit: nothing leaks from the uninitialised padded rows
  of the hand-off buffers or across rows of a packed tile."""
  big = O.draw(700 + B, 4, BB, 256)
  small = {k: (v if k == 'w_h' else (v[:, :B] if v.dim() == 3 or k == 'done' else v[:B]).contiguous())
           for k, v in big.items()}
  outs = []
  for inp in (small, big):
    fwd = _fwd(cuda, inp, mode, ws)
    outs.append((fwd, _bwd(cuda, inp, fwd, mode, ws)))
  (fs, bs), (fb, bb) = outs
  for k in FWD:
    _same(fs[k], fb[k][:, :B], k)
  for k in ('dg', 'dg16'):
    _same(bs[k], bb[k][:, :B], k)
  _same(bs['dc0'], bb['dc0'][:B], 'dc0')


@pytest.mark.parametrize('xpack', [1, 3, 8])
def test_xpack_bitwise(cuda, xpack):
  """lstm_xpack changes which blocks of the step grids work, never what
  they compute."""
  C = _C()
  inp = O.draw(800, 3, 17, 256)
  base_f = _fwd(cuda, inp, 0)
  base_b = _bwd(cuda, inp, base_f, 0)
  prev = C.lstm_xpack(xpack)
  try:
    assert C.lstm_xpack(xpack) == xpack
    fwd = _fwd(cuda, inp, 0)
    bwd = _bwd(cuda, inp, fwd, 0)
  finally:
    C.lstm_xpack(prev)
  assert C.lstm_xpack(prev) == prev
  for k in FWD:
    _same(fwd[k], base_f[k], k)
  for k in BWD:
    _same(bwd[k], base_b[k], k)


@pytest.mark.parametrize('B', [1, 16, 76, 150])
def test_prepacked_weights(cuda, B):
  """The actor step: lstm_pack_fwd once, then lstm_fwd(..., w4) at T = 1 is
  the self-packing call bit for bit, holds the oracle, and returns no wt."""
  C = _C()
  inp = O.draw(900 + B, 1, B, 256)
  inp['done'][0, B // 2] = 1
  w4 = torch.empty(256 * 1024, device=cuda)
  C.lstm_pack_fwd(inp['w_h'].to(cuda), w4)
  own = _fwd(cuda, inp, 0)
  pre = _fwd(cuda, inp, 0, w4=w4)
  for k in FWD:
    _same(pre[k], own[k], k)
  assert pre['wt'].numel() == 0 and own['wt'].numel() == 256 * 1024
  _check_fwd(inp, pre, 0, 0)
  two = O.draw(901, 2, 16, 256)
  with pytest.raises(RuntimeError, match='w4'):
    _fwd(cuda, two, 2, w4=w4)


def test_mode_guards(cuda):
  C = _C()
  from scalable_agent_amd.ops import lstm as lstm_ops
  with pytest.raises(RuntimeError, match='does not cover'):
    _fwd(cuda, O.draw(1, 1, 32, 256), 2)
  with pytest.raises(RuntimeError, match='does not cover'):
    _fwd(cuda, O.draw(2, 2, 33, 256), 2)
  small = O.draw(3, 2, 4, 64)
  with pytest.raises(RuntimeError, match='does not cover'):
    _fwd(cuda, small, 1)
  fwd = _fwd(cuda, small, 0)
  with pytest.raises(RuntimeError, match='does not cover'):
    _bwd(cuda, small, fwd, 1)
  prev_p = lstm_ops.set_persistent(False)
  prev_g = lstm_ops.set_gang(True)
  try:
    assert C.lstm_mode(256, 32, 1, False) == 0
    assert C.lstm_mode(256, 33, 5, False) == 0
    assert C.lstm_mode(256, 32, 5, False) == 2
    for persistent in (False, True):
      lstm_ops.set_persistent(persistent)
      for H in (64, 256):
        for B in (1, 32, 33):
          for T in (1, 2, 101):
            assert C.lstm_mode(H, B, T, True) != 2
  finally:
    lstm_ops.set_gang(prev_g)
    lstm_ops.set_persistent(prev_p)
