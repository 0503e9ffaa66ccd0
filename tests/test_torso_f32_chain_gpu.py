"""The fp32 torsos' autograd chains (ops/conv_f32.py: _ShallowTorsoF32,
_deep_forward, _deep_backward, their index arithmetic, flags, pool pads,
_pad_cin and the cf32_wgrad_defer / cf32_wgrad_flush bracket), call by call
against the float64 oracle of the NETWORK (tests/_torso_f32_chain_oracle.py,
tied to the model definition by tests/test_torso_f32_chain_oracle.py).

Method (that of test_deep_torso_chain_gpu.py).  Every extension call of the
public path (conv_f32.torso_forward_f32 under grad, then .backward(g)) is
recorded by a proxy around the extension (arguments cloned at call time) and
checked TEACHER-FORCED: the oracle's layer function is applied to the chain's
own recorded output of the previous layer, with the tensors and parameters
the MODEL names for that layer (recorded outputs and agent.convnet by name,
never the arguments of the call under check), and compared with the call's
recorded output.  The first layer's oracle input is frames.double() / 255.

Weight and bias gradients.  In the deep backward the slot sums are queued and
written by cf32_wgrad_flush: a view's content is taken when its call receives
it (nothing has written it since the start of the backward: every view is
written by one call) and again when the flush returns, and the difference is
compared with the float64 wgrad of that call's recorded input and dY.  The
sequence relu_mask_, defer(True), the wgrad-producing calls, defer(False),
flush() is asserted.  The shallow backward does not defer: after-minus-before
around the call.  Autograd must hand every parameter, by name, the view its
own layer's call accumulated into (bitwise).

Cases (frames -> maps, images):
  deep     (26, 30, 3) N=3  13x15, 7x8, 4x4: runtime Winograd geometry
           (21, 19, 4) N=3  odd maps, pool pad-before 1, four-channel stage 0
           (72, 96, 3) N=2  compiled geometries, fused Winograd conv+pool
                            heads, stage-0 scatter wgrad
           (84, 84, 4) N=2
  shallow  (20, 26, 3) N=3; (84, 84, 4) N=2 (asymmetric W pad);
           (72, 96, 3) N=2 (_pad_cin, dw_cin = 3)
Frames are buf[1:1+N] of a 0x7f-filled batch, biases are non-zero, g is
N(0, 1).  Switch variants (module attributes of conv_f32, monkeypatched) run
on deep (26, 30, 3) and (72, 96, 3), N=2, each asserting from the recorded
calls that its branch ran: POOL_GATHER_STAGES (0, 1, 2) and (1,),
FUSED_POOL_STAGES (0, 1, 2) (cf32_conv_pool_fwd runs where the Winograd head
declines: at (72, 96, 3) it takes all three heads, so only (26, 30, 3)
reaches the direct kernel), POOL_SCATTER False, U8_DIRECT['deep'], PW_U8, and
U8_DIRECT['shallow'] on the shallow torso.  All variants are reachable
in-process.

Bounds (nothing is fitted to the kernels):
  * conv outputs (y, t, dt, dx): the LARGER of _conv_f32_oracle.bound(M, A)
    and _wino_oracle.bound_fwd(cin, mag) for every call (the strided shallow
    convs: the direct bound alone, they have no Winograd instance).
  * pooled values: within the largest conv bound of the window; every argmax
    code decodes inside the image and equals the float64 first maximal tap
    where _conv_f32_oracle.argmax_clear holds.  cf32_maxpool_fwd is exact
    given the recorded conv output (value and first maximal tap).
  * cf32_relu_mask_ and cf32_maxpool_bwd: exact given the recorded activation
    / code; cf32_maxpool_bwd adds the up to four fp32 gradients of a cell in
    ascending window order, which the reference does in fp32 in that order.
  * gather forms: the same bounds (the + 5 of the direct bound covers the
    three gather additions), magnitudes from the gathered |dP|.
  * dw / db: the larger of bound(N Ho Wo, A) and _wino_oracle.bound_wg, the
    view's content before the call (the prefill) in A.
  * direct sinks: (.grad - prefill) against the fresh-zeros run under the sum
    of the two runs' dw bounds; two runs bitwise equal (tolerance 0).
  * conditions asserted on the calls: relu_out is True on every t (its stored
    ReLU) and, among the convs carrying add=, on the final one only; add= is
    on exactly the second conv of each block and on the backward of the first.

Measured on an MI355X (pytest -s), worst error / bound over all cases and
variants, per call family:
  x / 255 image                         0.198
  pooled (fused heads)                  0.026
  head conv (before cf32_maxpool_fwd)   0.011
  t / y                                 0.013 / 0.014
  dt / dx / dx of the gather dgrad      0.012 / 0.014 / 0.012
  shallow y / dx                        0.014 / 0.004
  dw / db (deep and shallow)            0.141 / 0.076
  direct sink minus prefill             0.057
All are far below 1: the bounds are worst-case sums of magnitudes, while a
wrong operand, flag or index moves a result by O(1), i.e. a ratio of 1e4 or
more.  The 27 tests take 5.6 s together.
"""

import pytest
import torch

from scalable_agent_amd.ops import conv_f32, grad_sink
from tests import _conv_f32_oracle as F32
from tests import _conv_oracle as O
from tests import _torso_chain_oracle as T
from tests import _torso_f32_chain_oracle as TF

pytestmark = pytest.mark.gpu

d64 = O.d64

# binding -> parameter names (with the defaults of the keyword parameters)
SIG = {
    'cf32_frames_f32': ('x',),
    'cf32_conv_fwd': ('x', 'w', 'b', 'stride', 'pt', 'pl', 'Ho', 'Wo', ('relu_in', False),
                      ('add', None), ('relu_out', False)),
    'cf32_wino_conv_pool_fwd': ('x', 'w', 'b', ('stages', -1)),
    'cf32_conv_pool_fwd': ('x', 'w', 'b', 'pbh', 'pbw'),
    'cf32_maxpool_fwd': ('x', 'pbh', 'pbw'),
    'cf32_maxpool_bwd': ('dy', 'arg', 'H', 'W', 'pbh', 'pbw'),
    'cf32_relu_mask_': ('dy', 'ref'),
    'cf32_conv_bwd_fused': ('dy', 'w', 'x', 'relu_x', 'dw', ('db', None), ('add', None),
                            ('mask', True)),
    'cf32_conv_wgrad': ('x', 'dy', 'stride', 'pt', 'pl', 'relu_in', 'dw', ('db', None),
                        ('pool_arg', None), ('pool_pbh', 0), ('pool_pbw', 0)),
    'cf32_conv_dgrad': ('dy', 'w', 'stride', 'pt', 'pl', 'H', 'W', ('mask', None),
                        ('add', None), ('pool_arg', None), ('pool_pbh', 0), ('pool_pbw', 0)),
    'cf32_wgrad_defer': ('on',),
    'cf32_wgrad_flush': (),
}
WGRAD_CALLS = ('cf32_conv_bwd_fused', 'cf32_conv_wgrad')
# forward-only bindings of the inference forms: must never run on this path
FORBIDDEN = ('cf32_head_fwd', 'cf32_res_block_fwd', 'cf32_stage_fwd', 'cf32_stage_tail_fwd',
             'cf32_shallow_fwd')

RATIO = {}


def _clone(v):
  return v.detach().clone() if torch.is_tensor(v) else v


class Call:

  def __init__(self, name, a, ptrs):
    self.name, self.a, self.ptrs = name, a, ptrs
    self.out = None
    self.after = {}  # clones of the views written (dw, db; relu_mask_: dy)

  def __repr__(self):
    return 'Call(%s)' % self.name


class Recorder:
  """Proxy around the extension: logs every torso call (arguments bound to
  their names and cloned before the call, clones of the outputs, clones of
  the tensors written in place).  While cf32_wgrad_defer(True) is in force
  the dw / db views are cloned when cf32_wgrad_flush returns."""

  def __init__(self, real):
    self._real = real
    self.calls = []
    self._defer = False
    self._pending = []

  def __getattr__(self, name):
    attr = getattr(self._real, name)
    assert name not in FORBIDDEN, name
    if name not in SIG:
      return attr

    def wrapped(*args, **kw):
      sig = SIG[name]
      a, live = {}, {}
      for i, p in enumerate(sig):
        pname, default = (p, None) if isinstance(p, str) else p
        if i < len(args):
          v = args[i]
        elif pname in kw:
          v = kw[pname]
        else:
          assert not isinstance(p, str), (name, pname)
          v = default
        live[pname] = v
        a[pname] = _clone(v)
      assert len(args) <= len(sig) and all(k in live for k in kw), (name, kw)
      call = Call(name, a, {k: v.data_ptr() for k, v in live.items() if torch.is_tensor(v)})
      out = attr(*args, **kw)
      call.out = ([_clone(o) for o in out] if isinstance(out, (list, tuple)) else _clone(out))
      if name == 'cf32_relu_mask_':
        call.after['dy'] = live['dy'].detach().clone()
      elif name in WGRAD_CALLS:
        views = {k: live[k] for k in ('dw', 'db')}
        if self._defer:
          self._pending.append((call, views))
        else:
          call.after = {k: v.detach().clone() for k, v in views.items()}
      elif name == 'cf32_wgrad_defer':
        self._defer = bool(live['on'])
      elif name == 'cf32_wgrad_flush':
        for c, views in self._pending:
          c.after = {k: v.detach().clone() for k, v in views.items()}
        self._pending = []
      self.calls.append(call)
      return out
    return wrapped


class Walker:

  def __init__(self, calls):
    self.calls, self.i = calls, 0

  def next(self, name=None):
    assert self.i < len(self.calls), 'the chain ended before %s' % name
    c = self.calls[self.i]
    self.i += 1
    if name is not None:
      assert c.name == name, 'call %d is %s, expected %s' % (self.i - 1, c.name, name)
    return c

  def done(self):
    return self.i == len(self.calls)


def embed_frames(frames, dev):
  return F32.embed(frames, dev)


def named_conv_params(agent):
  return [(n[len('convnet.'):], p) for n, p in agent.named_parameters()
          if n.startswith('convnet.')]


def setup(cuda, torso, frame_shape, N, seed):
  cpu_agent, frames, g = TF.case(torso, frame_shape, N, seed)
  agent = TF.make_agent(torso, frame_shape, seed).to(cuda)
  for (n, p), (m, q) in zip(named_conv_params(agent), named_conv_params(cpu_agent)):
    assert n == m and torch.equal(p.detach().cpu(), q.detach())
  return agent, frames, g, embed_frames(frames, cuda), g.to(cuda)


def run_chain(monkeypatch, agent, frames_d, g_d, grad=True, direct=False):
  """One pass through the public path; returns (features, recorded calls)."""
  rec = Recorder(F32.ext())
  with monkeypatch.context() as m:
    m.setattr(conv_f32, 'ext', lambda: rec)
    if direct:
      with grad_sink.direct_grads():
        feats = conv_f32.torso_forward_f32(agent, frames_d)
        got = torch.autograd.grad(feats, [p for _, p in named_conv_params(agent)], g_d,
                                  allow_unused=True)
      assert all(x is None for x in got), 'autograd must get None for direct sinks'
    elif grad:
      feats = conv_f32.torso_forward_f32(agent, frames_d)
      feats.backward(g_d)
    else:
      with torch.no_grad():
        feats = conv_f32.torso_forward_f32(agent, frames_d)
    torch.cuda.synchronize()
  return feats, rec.calls


def split_calls(calls):
  k = [i for i, c in enumerate(calls) if c.name == 'cf32_relu_mask_']
  assert len(k) == 1, calls
  return calls[:k[0]], calls[k[0]:]


def within(out, ref, bnd, fam, what):
  out = d64(out)
  assert out.shape == ref.shape, (what, out.shape, ref.shape)
  assert bool(torch.isfinite(out).all()), what
  r = float(((out - ref).abs() / bnd.clamp_min(1e-300)).max())
  RATIO[fam] = max(RATIO.get(fam, 0.0), r)
  print('F32CHAIN %-44s %-10s error/bound=%.4f' % (what, fam, r))
  assert r <= 1.0, '%s: error / bound = %.4g' % (what, r)


def exact(out, ref, what):
  out = d64(out)
  assert out.shape == ref.shape, (what, out.shape, ref.shape)
  n = int((out != ref).sum())
  assert n == 0, '%s: %d elements differ' % (what, n)


def report():
  print('F32CHAIN worst error/bound so far: ' +
        ', '.join('%s %.3f' % kv for kv in sorted(RATIO.items())))


def wb_check(call, x, dy, name, views, bounds, K=3, S=1, absdy=None):
  """dw / db of one call: the views' content after (the flush, or the call)
  against content before + the float64 wgrad of (x, dy)."""
  assert set(call.after) == {'dw', 'db'}, '%s: its weight gradient was never written' % name
  dw0, db0 = d64(call.a['dw']), d64(call.a['db'])
  cin = dw0.shape[2]
  if K == 3 and S == 1:
    dw, db = O.wgrad64(x, dy)[:, :, :cin], dy.sum(dim=(0, 1, 2))
    bw, bb = TF.wgrad_bounds(x, dy, dw0, db0, absdy)
  else:
    dw, db = F32.conv_wgrad(x, dy, K, S)
    aw, ab = F32.conv_wgrad(x.abs(), dy.abs(), K, S)
    M = dy.shape[0] * dy.shape[1] * dy.shape[2]
    dw, aw = dw[:, :, :cin], aw[:, :, :cin]
    bw, bb = F32.bound(M, aw + dw0.abs()), F32.bound(M, ab + db0.abs())
  assert bool((dw != 0).any()) and bool((db != 0).any()), name
  within(call.after['dw'], dw0 + dw, bw, 'dw', name + ' dw')
  within(call.after['db'], db0 + db, bb, 'db', name + ' db')
  for sfx, k, b in (('__w', 'dw', bw), ('__b', 'db', bb)):
    assert name + sfx not in views, name
    views[name + sfx] = (call.after[k], call.ptrs[k])
    bounds[name + sfx] = b


# ------------------------------------------------------------------ deep torso

def check_pooled(pooled, arg, y64, B, pads, what):
  val, code, vb, clear = TF.pool_check_terms(y64, B, pads)
  within(pooled, val, vb, 'pooled', what + ' pooled')
  O.tap_positions(arg, y64.shape[1], y64.shape[2], *pads)  # every code inside the image
  left_out = 1.0 - float(clear.double().mean())
  assert left_out <= 0.01, (what, left_out)
  a = arg.to('cpu').long()
  assert torch.equal(a[clear], code[clear]), what + ': argmax is not the first maximal tap'


def check_deep_forward(agent, frames, fwd, sw):
  """Every forward call against the oracle layer applied to the previous
  call's recorded output.  Returns the recorded activations by role."""
  stages = T.stages_of(agent)
  P = T.params64(agent)
  it = Walker(fwd)
  x0 = d64(frames) / 255.0
  rec = dict(heads=[], blocks=[], forms=[], image=False)
  if not sw.get('u8_deep'):
    c = it.next('cf32_frames_f32')
    exact(c.a['x'], d64(frames), 'frames_f32 source')
    img = d64(c.out)
    assert img.shape[3] == 4 and bool((img[..., x0.shape[3]:] == 0).all())
    within(img[..., :x0.shape[3]], x0, F32.bound(0, x0), 'image', 'x / 255 image')
    rec['image'] = True
  x = x0
  nconv2 = 0
  for s, st in enumerate(stages):
    tag = 'stage %d' % s
    w, b = P[st['head']]
    H, W = x.shape[1], x.shape[2]
    y64, B = O.conv64(x, w, b), TF.conv_bound(x, w, b)
    pads = (O.pool_pb(H), O.pool_pb(W))
    c = it.next()
    src_dtype = c.a['x'].dtype
    declined = False
    if c.name == 'cf32_wino_conv_pool_fwd' and len(c.out) == 0:
      declined = True
      c = it.next()
    form = c.name
    if form in ('cf32_wino_conv_pool_fwd', 'cf32_conv_pool_fwd'):
      pooled, arg = c.out
      check_pooled(pooled, arg, y64, B, pads, tag + ' head')
    else:
      assert form == 'cf32_conv_fwd', form
      assert c.a['add'] is None and not c.a['relu_out'] and not c.a['relu_in'], tag
      within(c.out, y64, B, 'head', tag + ' head conv')
      conv_out = d64(c.out)
      c = it.next('cf32_maxpool_fwd')
      pooled, arg = c.out
      val, code = O.pool64(conv_out, *pads)
      exact(pooled, val, tag + ' maxpool_fwd value')
      O.tap_positions(arg, H, W, *pads)
      assert torch.equal(arg.to('cpu').long(), code), tag + ' maxpool_fwd code'
    if s in conv_f32.FUSED_POOL_STAGES and (declined or src_dtype != torch.float32):
      assert form == 'cf32_conv_pool_fwd', (tag, form)
    rec['forms'].append(form)
    rec['heads'].append(dict(x=x, arg=arg.to('cpu').long(), pads=pads, H=H, W=W,
                             src_dtype=src_dtype))
    xa = d64(pooled)
    blocks = []
    for bi, (n1, n2) in enumerate(st['blocks']):
      final = s == len(stages) - 1 and bi == len(st['blocks']) - 1
      btag = '%s block %d' % (tag, bi)
      c = it.next('cf32_conv_fwd')
      assert c.a['add'] is None and c.a['relu_in'] and c.a['relu_out'], btag
      xr = xa.relu()
      t_ref = O.conv64(xr, P[n1][0], P[n1][1]).relu()
      zeros = float((t_ref == 0).double().mean())
      assert 0.2 <= zeros <= 0.8, (btag, zeros)
      within(c.out, t_ref, TF.conv_bound(xr, P[n1][0], P[n1][1]), 't', btag + ' t')
      t64 = d64(c.out)
      c = it.next('cf32_conv_fwd')
      assert c.a['add'] is not None and not c.a['relu_in'], btag
      assert c.a['relu_out'] is final, '%s: relu_out=%r' % (btag, c.a['relu_out'])
      nconv2 += 1
      y_ref = O.conv64(t64, P[n2][0], P[n2][1]) + xa
      assert bool((y_ref < 0).any()), btag  # a wrong final ReLU would show
      if final:
        assert bool((y_ref > 0).any())
        y_ref = y_ref.relu()
      within(c.out, y_ref, TF.conv_bound(t64, P[n2][0], P[n2][1], add=xa), 'y', btag + ' y')
      blocks.append(dict(xa=xa, t=t64, y=d64(c.out)))
      xa = blocks[-1]['y']
    rec['blocks'].append(blocks)
    x = xa
  assert it.done(), fwd[it.i:]
  assert nconv2 == sum(c.name == 'cf32_conv_fwd' and c.a['add'] is not None for c in fwd)
  rec['out'] = x
  assert bool((x == 0).any()) and bool((x > 0).any())
  return rec


def check_deep_backward(agent, frames, g, fw, bwd):
  """Every backward call against the oracle layer applied to the previous
  call's recorded output and the forward tensors the model names.  Returns
  ({parameter name: (final content of its view, its address)}, bounds)."""
  stages = T.stages_of(agent)
  P = T.params64(agent)
  names = [c.name for c in bwd]
  # one defer(True), then defer(False), then one flush, every wgrad between
  assert names[:2] == ['cf32_relu_mask_', 'cf32_wgrad_defer'], names
  assert names[-2:] == ['cf32_wgrad_defer', 'cf32_wgrad_flush'], names
  assert names.count('cf32_wgrad_defer') == 2 and names.count('cf32_wgrad_flush') == 1
  assert bwd[1].a['on'] is True and bwd[-2].a['on'] is False
  assert sum(n in WGRAD_CALLS for n in names) == 15
  it = Walker(bwd)
  views, bounds = {}, {}
  c = it.next('cf32_relu_mask_')
  out = fw['out']
  g64 = d64(g).reshape(out.shape)
  exact(c.a['dy'], g64, 'the mask starts from grad_out')
  exact(c.a['ref'], out, 'the mask reads the features')
  dy = T.final_relu_bwd(g64, out)
  exact(c.after['dy'], dy, 'final ReLU mask')
  assert bool((dy != g64).any())
  dy32 = c.after['dy'].to('cpu')
  it.next('cf32_wgrad_defer')
  for s in reversed(range(len(stages))):
    st = stages[s]
    for bi in reversed(range(len(st['blocks']))):
      n1, n2 = st['blocks'][bi]
      blk = fw['blocks'][s][bi]
      tag = 'stage %d block %d' % (s, bi)
      c = it.next('cf32_conv_bwd_fused')
      assert c.a['add'] is None and c.a['mask'] is True and c.a['relu_x'] is False, tag
      m = (blk['t'] > 0).to(torch.float64)
      w2 = P[n2][0]
      within(c.out, m * O.dgrad64(dy, w2), TF.dgrad_bound(dy, w2, m), 'dt', tag + ' dt')
      wb_check(c, blk['t'], dy, n2, views, bounds)
      dt = d64(c.out)
      c = it.next('cf32_conv_bwd_fused')
      assert c.a['add'] is not None and c.a['mask'] is True and c.a['relu_x'] is True, tag
      m = (blk['xa'] > 0).to(torch.float64)
      w1 = P[n1][0]
      within(c.out, m * O.dgrad64(dt, w1) + dy, TF.dgrad_bound(dt, w1, m, add=dy), 'dx',
             tag + ' dx')
      wb_check(c, blk['xa'].relu(), dt, n1, views, bounds)
      dy, dy32 = d64(c.out), c.out.to('cpu')
    head = fw['heads'][s]
    tag = 'stage %d head' % s
    H, W, pads = head['H'], head['W'], head['pads']
    w = P[st['head']][0]
    c = it.next()
    if c.name == 'cf32_maxpool_bwd':
      ref32 = TF.pool_gather_f32(dy32, head['arg'], H, W, pads)
      exact(c.out, ref32.double(), tag + ' maxpool_bwd')
      dconv = d64(c.out)
      assert bool((dconv != 0).any())
      if s > 0:
        c = it.next('cf32_conv_bwd_fused')
        assert c.a['add'] is None and c.a['mask'] is False and c.a['relu_x'] is False, tag
        within(c.out, O.dgrad64(dconv, w), TF.dgrad_bound(dconv, w), 'dx', tag + ' dx')
      else:
        c = it.next('cf32_conv_wgrad')
        assert c.a['pool_arg'] is None and c.a['relu_in'] is False, tag
      wb_check(c, head['x'], dconv, st['head'], views, bounds)
      fw['heads'][s]['bwd'] = 'maxpool_bwd'
    else:
      assert c.name == 'cf32_conv_wgrad' and c.a['pool_arg'] is not None, (tag, c.name)
      assert c.a['relu_in'] is False
      dY, S, _ = T.head_gather(dy, head['arg'], H, W, pads)
      wb_check(c, head['x'], dY, st['head'], views, bounds, absdy=S)
      fw['heads'][s]['bwd'] = 'gather'
      fw['heads'][s]['wgrad_src'] = c.a['x']
      if s > 0:
        c = it.next('cf32_conv_dgrad')
        assert c.a['pool_arg'] is not None and c.a['mask'] is None and c.a['add'] is None
        within(c.out, O.dgrad64(dY, w), TF.dgrad_bound(dY, w, absdy=S), 'dx_gather',
               tag + ' dx (gather)')
    if s > 0:
      dy, dy32 = d64(c.out), c.out.to('cpu')
  assert it.next('cf32_wgrad_defer').a['on'] is False
  it.next('cf32_wgrad_flush')
  assert it.done()
  return views, bounds


def check_grads(agent, views):
  """Autograd hands every parameter, by name, the view its own layer's call
  accumulated into."""
  named = named_conv_params(agent)
  assert sorted(n for n, _ in named) == sorted(views)
  assert len({ptr for _, ptr in views.values()}) == len(views), 'two calls share a view'
  for n, p in named:
    assert p.grad is not None and p.grad.dtype == torch.float32, n
    O.bits_equal(p.grad, views[n][0], 'autograd gradient of ' + n)


def deep_chain(cuda, monkeypatch, frame_shape, N, seed, sw=None):
  sw = sw or {}
  agent, frames, g, frames_d, g_d = setup(cuda, 'deep', frame_shape, N, seed)
  buf = frames_d._base
  g_keep = g_d.clone()
  feats, calls = run_chain(monkeypatch, agent, frames_d, g_d)
  assert torch.equal(g_d, g_keep), 'backward modified grad_out'
  assert bool((buf[0] == 0x7f).all()) and bool((buf[-1] == 0x7f).all())
  fwd, bwd = split_calls(calls)
  fw = check_deep_forward(agent, frames, fwd, sw)
  exact(feats, fw['out'].reshape(N, -1), 'features are the last call\'s output')
  views, _ = check_deep_backward(agent, frames, g, fw, bwd)
  check_grads(agent, views)
  print('F32CHAIN deep %s calls: %s' % (frame_shape, ' '.join(
      c.name[5:] + ('[]' if c.name == 'cf32_wino_conv_pool_fwd' and not c.out else '')
      for c in calls)))
  report()
  return agent, frames_d, g_d, feats, fw, calls


@pytest.mark.parametrize('frame_shape,N,seed', TF.DEEP_CASES)
def test_deep_chain_call_by_call(cuda, monkeypatch, frame_shape, N, seed):
  agent, frames_d, g_d, feats, fw, calls = deep_chain(cuda, monkeypatch, frame_shape, N, seed)
  names = [c.name for c in calls]
  if frame_shape == (26, 30, 3):
    # 13x15 and 7x8 are odd: the fused Winograd heads decline
    assert fw['forms'][1:] == ['cf32_conv_fwd', 'cf32_conv_fwd']
  if frame_shape == (72, 96, 3):
    assert fw['forms'] == ['cf32_wino_conv_pool_fwd'] * 3
  # defaults: stage 0 in scatter form, stages 1 and 2 through maxpool_bwd
  assert [h['bwd'] for h in fw['heads']] == ['gather', 'maxpool_bwd', 'maxpool_bwd']
  assert names.count('cf32_maxpool_bwd') == 2
  # features under no_grad (torso_blocks='ops') are bitwise the under-grad ones
  assert agent.torso_blocks == 'ops'
  feats_i, calls_i = run_chain(monkeypatch, agent, frames_d, g_d, grad=False)
  assert [c.name for c in calls_i] == [c.name for c in split_calls(calls)[0]]
  O.bits_equal(feats_i, feats.detach(), 'no_grad features vs under-grad features')


# name -> (conv_f32 attributes, U8_DIRECT items)
DEEP_VARIANTS = {
    'gather_all': (dict(POOL_GATHER_STAGES=(0, 1, 2), POOL_GATHER=True), {}),
    'gather_1': (dict(POOL_GATHER_STAGES=(1,), POOL_GATHER=True), {}),
    'fused_pool': (dict(FUSED_POOL_STAGES=(0, 1, 2)), {}),
    'no_scatter': (dict(POOL_SCATTER=False), {}),
    'u8_deep': ({}, dict(deep=True)),
    'pw_u8': (dict(PW_U8=True), {}),
}
VARIANT_SHAPES = [TF.DEEP_CASES[0][0], TF.DEEP_CASES[2][0]]


@pytest.mark.parametrize('frame_shape', VARIANT_SHAPES)
@pytest.mark.parametrize('variant', sorted(DEEP_VARIANTS))
def test_deep_switch_variants(cuda, monkeypatch, variant, frame_shape):
  attrs, u8 = DEEP_VARIANTS[variant]
  for k, v in attrs.items():
    assert hasattr(conv_f32, k)
    monkeypatch.setattr(conv_f32, k, v)
  for k, v in u8.items():
    monkeypatch.setitem(conv_f32.U8_DIRECT, k, v)
  seed = [c[2] for c in TF.DEEP_CASES if c[0] == frame_shape][0]
  _, frames_d, _, _, fw, calls = deep_chain(cuda, monkeypatch, frame_shape, 2, seed,
                                            sw={'u8_deep': variant == 'u8_deep'})
  names = [c.name for c in calls]
  heads = fw['heads']
  bwd_forms = [h['bwd'] for h in heads]
  if variant == 'gather_all':
    assert bwd_forms == ['gather'] * 3 and 'cf32_maxpool_bwd' not in names
    assert names.count('cf32_conv_dgrad') == 2
    assert sum(c.name == 'cf32_conv_wgrad' and c.a['pool_arg'] is not None
               for c in calls) == 3
  elif variant == 'gather_1':
    assert bwd_forms == ['gather', 'gather', 'maxpool_bwd']
    assert names.count('cf32_conv_dgrad') == 1 and names.count('cf32_maxpool_bwd') == 1
  elif variant == 'fused_pool':
    if frame_shape == (26, 30, 3):
      assert fw['forms'][1:] == ['cf32_conv_pool_fwd'] * 2
    declined = sum(c.name == 'cf32_wino_conv_pool_fwd' and not c.out for c in calls)
    assert names.count('cf32_conv_pool_fwd') == declined
    assert 'cf32_maxpool_fwd' not in names
  elif variant == 'no_scatter':
    assert bwd_forms == ['maxpool_bwd'] * 3 and names.count('cf32_maxpool_bwd') == 3
    assert all(c.a['pool_arg'] is None for c in calls if c.name == 'cf32_conv_wgrad')
  elif variant == 'u8_deep':
    # no image; the Winograd head takes fp32 only, so stage 0 runs the direct
    # conv+pool on the bytes (stage 0 is in the default FUSED_POOL_STAGES)
    assert 'cf32_frames_f32' not in names and names[0] != 'cf32_wino_conv_pool_fwd'
    assert heads[0]['src_dtype'] == torch.uint8
    assert fw['forms'][0] == ('cf32_conv_pool_fwd' if 0 in conv_f32.FUSED_POOL_STAGES
                              else 'cf32_conv_fwd')
    assert heads[0]['wgrad_src'].dtype == torch.uint8
  elif variant == 'pw_u8':
    # the forward reads the fp32 image, the saved stage-0 input is the frames
    assert fw['image'] and heads[0]['src_dtype'] == torch.float32
    src = heads[0]['wgrad_src']
    assert src.dtype == torch.uint8 and torch.equal(src, frames_d)


# -------------------------------------------------------------- shallow torso

def check_shallow(agent, frames, g, calls, u8):
  layers = TF.shallow_layers(agent)
  P = TF.shallow_params64(agent)
  fwd, bwd = split_calls(calls)
  it = Walker(fwd)
  x0 = d64(frames) / 255.0
  if not u8:
    c = it.next('cf32_frames_f32')
    img = d64(c.out)
    assert img.shape[3] == 4 and bool((img[..., x0.shape[3]:] == 0).all())
    within(img[..., :x0.shape[3]], x0, F32.bound(0, x0), 'image', 'x / 255 image')
  acts = [x0]
  for i, (n, K, S) in enumerate(layers):
    c = it.next('cf32_conv_fwd')
    assert c.a['relu_out'] is True and not c.a['relu_in'] and c.a['add'] is None
    if i == 0:
      assert c.a['x'].dtype == (torch.uint8 if u8 else torch.float32)
    x = acts[-1]
    ref, A = TF.sh_fwd(x, P[n][0], P[n][1], S)
    zeros = float((ref == 0).double().mean())
    assert 0.2 <= zeros <= 0.8, (n, zeros)
    M = K * K * (max(x.shape[3], 4) if i == 0 else x.shape[3])
    within(c.out, ref, F32.bound(M, A), 'shallow_y', 'shallow layer %d y' % i)
    acts.append(d64(c.out))
  assert it.done()
  out = acts[-1]
  assert bool((out == 0).any()) and bool((out > 0).any())
  names = [c.name for c in bwd]
  assert names == ['cf32_relu_mask_', 'cf32_conv_wgrad', 'cf32_conv_dgrad', 'cf32_conv_wgrad',
                   'cf32_conv_dgrad', 'cf32_conv_wgrad'], names
  it = Walker(bwd)
  c = it.next()
  g64 = d64(g).reshape(out.shape)
  exact(c.a['dy'], g64, 'the mask starts from grad_out')
  dy = T.final_relu_bwd(g64, out)
  exact(c.after['dy'], dy, 'final ReLU mask')
  assert bool((dy != g64).any())
  views, bounds = {}, {}
  for i in reversed(range(3)):
    n, K, S = layers[i]
    c = it.next('cf32_conv_wgrad')
    assert c.a['pool_arg'] is None and c.a['relu_in'] is False
    wb_check(c, acts[i], dy, n, views, bounds, K=K, S=S)
    if i > 0:
      c = it.next('cf32_conv_dgrad')
      assert c.a['mask'] is not None and c.a['add'] is None and c.a['pool_arg'] is None
      ref, A = TF.sh_dgrad(dy, P[n][0], S, acts[i])
      within(c.out, ref, F32.bound(K * K * dy.shape[3], A), 'shallow_dx',
             'shallow layer %d dx' % i)
      dy = d64(c.out)
  assert it.done()
  return out, views, bounds


def shallow_chain(cuda, monkeypatch, frame_shape, N, seed, u8=False):
  agent, frames, g, frames_d, g_d = setup(cuda, 'shallow', frame_shape, N, seed)
  buf = frames_d._base
  g_keep = g_d.clone()
  feats, calls = run_chain(monkeypatch, agent, frames_d, g_d)
  assert torch.equal(g_d, g_keep), 'backward modified grad_out'
  assert bool((buf[0] == 0x7f).all()) and bool((buf[-1] == 0x7f).all())
  out, views, _ = check_shallow(agent, frames, g, calls, u8)
  exact(feats, out.reshape(N, -1), 'features are the last call\'s output')
  check_grads(agent, views)
  print('F32CHAIN shallow %s calls: %s' % (frame_shape, ' '.join(c.name[5:] for c in calls)))
  report()
  return agent, frames_d, g_d, feats, calls


@pytest.mark.parametrize('frame_shape,N,seed', TF.SHALLOW_CASES)
def test_shallow_chain_call_by_call(cuda, monkeypatch, frame_shape, N, seed):
  agent, frames_d, g_d, feats, calls = shallow_chain(cuda, monkeypatch, frame_shape, N, seed)
  w0 = [c for c in calls if c.name == 'cf32_conv_fwd'][0].a['w']
  assert w0.shape[2] == 4  # _pad_cin on RGB frames: the image's pad channel
  if frame_shape[2] == 3:
    assert bool((w0[:, :, 3] == 0).all())
    wg0 = [c for c in calls if c.name == 'cf32_conv_wgrad'][-1]
    assert wg0.a['dw'].shape[2] == 3 and wg0.a['x'].shape[3] == 4  # dw_cin = 3
  assert agent.torso_blocks == 'ops'
  feats_i, calls_i = run_chain(monkeypatch, agent, frames_d, g_d, grad=False)
  assert [c.name for c in calls_i] == [c.name for c in split_calls(calls)[0]]
  O.bits_equal(feats_i, feats.detach(), 'no_grad features vs under-grad features')


@pytest.mark.parametrize('frame_shape,N,seed', [TF.SHALLOW_CASES[0], TF.SHALLOW_CASES[2]])
def test_shallow_u8_direct_variant(cuda, monkeypatch, frame_shape, N, seed):
  monkeypatch.setitem(conv_f32.U8_DIRECT, 'shallow', True)
  _, _, _, _, calls = shallow_chain(cuda, monkeypatch, frame_shape, N, seed, u8=True)
  assert all(c.name != 'cf32_frames_f32' for c in calls)
  first = [c for c in calls if c.name == 'cf32_conv_fwd'][0]
  assert first.a['x'].dtype == torch.uint8 and first.a['w'].shape[2] == frame_shape[2]
  wg0 = [c for c in calls if c.name == 'cf32_conv_wgrad'][-1]
  assert wg0.a['x'].dtype == torch.uint8


# ---------------------------------------------------------- whole-chain checks

SMALL = ([('deep',) + c for c in TF.DEEP_CASES[:2]] +
         [('shallow',) + c for c in TF.SHALLOW_CASES[:1]])


def fresh_grads(agent, frames_d, g_d):
  for _, p in named_conv_params(agent):
    p.grad = None
  feats = conv_f32.torso_forward_f32(agent, frames_d)
  feats.backward(g_d)
  torch.cuda.synchronize()
  return feats.detach(), {n: p.grad.clone() for n, p in named_conv_params(agent)}


def checked_bounds(agent, frames, g, calls, torso):
  if torso == 'shallow':
    return check_shallow(agent, frames, g, calls, False)[1:]
  fwd, bwd = split_calls(calls)
  fw = check_deep_forward(agent, frames, fwd, {})
  return check_deep_backward(agent, frames, g, fw, bwd)


@pytest.mark.parametrize('torso,frame_shape,N,seed', SMALL)
def test_direct_sink_adds_to_the_prefill(cuda, monkeypatch, torso, frame_shape, N, seed):
  agent, frames, g, frames_d, g_d = setup(cuda, torso, frame_shape, N, seed)
  named = named_conv_params(agent)
  _, calls0 = run_chain(monkeypatch, agent, frames_d, g_d)
  fresh = {n: p.grad.clone() for n, p in named}
  _, bounds0 = checked_bounds(agent, frames, g, calls0, torso)
  gen = torch.Generator().manual_seed(seed)
  prefill = {}
  for n, p in named:
    scale = float(fresh[n].abs().max())
    assert scale > 0, n
    prefill[n] = (torch.randn(p.shape, generator=gen) * scale).to(cuda)
    assert bool((prefill[n] != 0).all())
    p.grad = prefill[n].clone()
  sinks = {n: p.grad for n, p in named}
  g_keep = g_d.clone()
  _, calls = run_chain(monkeypatch, agent, frames_d, g_d, direct=True)
  assert torch.equal(g_d, g_keep), 'backward modified grad_out'
  # the same per-call checks, the prefill in every magnitude
  views, bounds = checked_bounds(agent, frames, g, calls, torso)
  # every dw / db view the kernels wrote is a parameter's own .grad
  for n, p in named:
    assert p.grad is sinks[n], n
    assert views[n][1] == p.grad.data_ptr(), n
    O.bits_equal(p.grad, views[n][0], 'direct sink ' + n)
    within(d64(p.grad) - d64(prefill[n]), d64(fresh[n]), bounds[n] + bounds0[n], 'sink',
           'direct sink minus prefill ' + n)
  report()


@pytest.mark.parametrize('torso,frame_shape,N,seed', SMALL)
def test_two_runs_are_bitwise_equal(cuda, torso, frame_shape, N, seed):
  agent, frames, g, frames_d, g_d = setup(cuda, torso, frame_shape, N, seed)
  f1, g1 = fresh_grads(agent, frames_d, g_d)
  f2, g2 = fresh_grads(agent, frames_d, g_d)
  O.bits_equal(f1, f2, 'features, two runs')
  for n in g1:
    O.bits_equal(g1[n], g2[n], 'gradient of ' + n)
    assert bool((g1[n] != 0).any()), n
