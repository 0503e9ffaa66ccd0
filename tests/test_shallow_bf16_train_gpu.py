"""The shallow torso's bf16 training kernels (csrc/kernels/
conv_shallow_bf16_train.hip) against a plain float64 conv chain on the CPU:
the forward with its saved maps, the data gradient layer by layer, the weight
and bias gradients, and the public path Agent(torso_dtype='bf16').

Frames 72x96x3, 84x84x4, 72x128x3 and 72x96x1; N = 1, and N = 5 under a grid
cap of 2 (every workgroup walks 2-3 images, two slots are reduced).

Error model of the bounds: bf16 x bf16 products are exact in fp32, so an
element's error is that of its fp32 additions, each at most 2^-24 of the sum
of absolute products S.  A forward / data-gradient element takes one
accumulator rounding per MFMA K step (8 / 16 / 18 per layer) plus the
additions inside an MFMA and the bias (and division) roundings, for which 8
more are allowed: K = steps + 8.  The gradient bounds use the number of
reduced terms, the plain worst case.
"""

import pytest
import torch
import torch.nn.functional as F

from scalable_agent_amd.models import Agent

from . import _shallow_bf16_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = O.FRAMES
CASES = [(1, 0), (5, 2)]  # (images, grid cap)
STRIDES = (4, 2, 2)
KSTEPS = (8, 16, 18)
EPS = 2.0 ** -24


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _conv64(x, w, s):
  """NHWC float64 x, HWIO float64 w -> NHWC, TF-SAME pads written out."""
  _, pt, pb = O.pads(x.shape[1], w.shape[0], s)
  _, pl, pr = O.pads(x.shape[2], w.shape[1], s)
  y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)),
               w.permute(3, 2, 0, 1), stride=s)
  return y.permute(0, 2, 3, 1)


def _grads64(x, w, s, dout):
  """-> (dx, dw, db) of sum(conv(x, w) * dout)."""
  x = x.clone().requires_grad_()
  w = w.clone().requires_grad_()
  dx, dw = torch.autograd.grad(_conv64(x, w, s), (x, w), dout)
  return dx, dw, dout.sum(dim=(0, 1, 2))


def _bf(t):
  return t.to(torch.bfloat16).double()


def _run(C, dev, frames, ws, bs, dfeats, cap):
  """Every tensor of one forward + backward of the raw ops (CPU float64)."""
  assert C.conv_tune('shallow_bf16_grid', cap) >= 0
  try:
    fr = frames.to(dev)
    w = [x.to(dev).contiguous() for x in ws]
    b = [x.to(dev) for x in bs]
    w1p, w2p, w3p, wd2, wd3 = C.shallow_bf16_train_pack(*w)
    feats, a1, a2 = C.shallow_bf16_train_fwd(fr, w1p, b[0], w2p, b[1], w3p, b[2])
    infer = C.shallow_bf16_fwd(fr, *[t for p, q in zip(C.shallow_bf16_pack(*w), b)
                                     for t in (p, q)])
    dy3, da2, da1 = C.shallow_bf16_bwd_data(fr, dfeats.to(dev), feats, a2, a1, wd3, wd2)
    g = [torch.zeros_like(t) for pair in zip(w, b) for t in pair]
    C.shallow_bf16_wgrad(fr, a1, a2, dy3, da2, da1, *g)
    info = [C.conv_launch_info('shallow_bf16_' + f)
            for f in ('train_fwd', 'bwd_data', 'wgrad')]
    torch.cuda.synchronize()
  finally:
    C.conv_tune('shallow_bf16_grid', 0)
  n = frames.shape[0]
  for i in info:
    assert i['grid'] == (min(n, cap) if cap else n) and i['ntiles'] == n, i
  out = dict(feats=feats, a1=a1, a2=a2, dy3=dy3, da2=da2, da1=da1, infer=infer)
  out = {k: v.cpu() for k, v in out.items()}
  out.update(dw=[t.double().cpu() for t in g[0::2]], db=[t.double().cpu() for t in g[1::2]])
  return out


def _random_inputs(shape, n):
  g = torch.Generator().manual_seed(100 * shape[0] + 10 * shape[2] + n)
  frames = torch.randint(0, 256, (n,) + tuple(shape), generator=g, dtype=torch.uint8)
  ws, bs, cin = [], [], shape[2]
  for k, _, cout in O.LAYERS:
    ws.append(torch.randn(k, k, cin, cout, generator=g) / (k * k * cin) ** 0.5)
    bs.append(0.1 * torch.randn(cout, generator=g))
    cin = cout
  dfeats = torch.randn((n,) + O.out_shape(shape), generator=g)
  return frames, ws, bs, dfeats


_RANDOM = {}


def _random_case(cuda, shape, n, cap):
  key = (shape, n, cap)
  if key not in _RANDOM:
    inp = _random_inputs(shape, n)
    _RANDOM[key] = inp + (_run(_C(), cuda, *inp, cap),)
  return _RANDOM[key]


@pytest.mark.parametrize('n,cap', CASES)
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_and_saved_maps(cuda, shape, n, cap):
  """feats rounds to the inference kernel's bits; each saved map is what a
  float64 conv of the previous SAVED map rounds to, wherever the float64
  value is further than (steps + 8) 2^-24 S from a bf16 rounding boundary or
  from 0 (one ulp elsewhere; at most 2 % of the elements may be that close)."""
  frames, ws, bs, _, k = _random_case(cuda, shape, n, cap)
  assert torch.equal(k['feats'].to(torch.bfloat16), k['infer'])
  x = frames.double()
  for l, name in enumerate(('a1', 'a2', 'feats')):
    wb = _bf(ws[l])
    scale = 255.0 if l == 0 else 1.0
    v = _conv64(x, wb, STRIDES[l]) / scale + bs[l].double()
    tol = (KSTEPS[l] + 8) * EPS * (_conv64(x, wb.abs(), STRIDES[l]) / scale +
                                   bs[l].double().abs())
    got = k[name].double()
    if name == 'feats':  # fp32, not rounded
      assert bool(((got - v.clamp(min=0)).abs() <= tol).all())
      break
    lo, hi = _bf((v - tol).clamp(min=0)), _bf((v + tol).clamp(min=0))
    share = (lo != hi).double().mean().item()
    print(shape, n, name, 'share near a boundary %.4f' % share)
    assert share <= 0.02
    assert bool(((lo <= got) & (got <= hi)).all())
    x = got  # the next layer reads the kernel's own map


@pytest.mark.parametrize('n,cap', CASES)
@pytest.mark.parametrize('shape', SHAPES)
def test_backward_layer_by_layer(cuda, shape, n, cap):
  """Each gradient against float64 fed the kernel's own bf16 tensors.  dA:
  2^-8 |ref| (one RNE to bf16) + (K + 8) 2^-24 sum|w||dOut| with K the reduced
  terms (taps of a phase x cout); dW, db: (P + 8) 2^-24 sum|in||dOut| with P
  the reduced pixels x images, layer 1 plus one division rounding.

  The rounding term is 2^-8, not 2^-9: bf16 keeps 8 significant bits, so the
  spacing in [2^e, 2^(e+1)) is 2^(e-7) and RNE errs by up to half of it,
  2^(e-8) <= 2^-8 |x|.  With 2^-9 a correctly rounded 0.58203 for 0.58066
  (error 1.37e-3, half a spacing is 1.95e-3) counted as wrong."""
  frames, ws, _, dfeats, k = _random_case(cuda, shape, n, cap)
  assert torch.equal(k['dy3'], torch.where(k['feats'] > 0, dfeats, torch.zeros(()))
                     .to(torch.bfloat16))
  ins = [frames.double(), k['a1'].double(), k['a2'].double()]
  douts = [k['da1'].double(), k['da2'].double(), k['dy3'].double()]
  for l in (2, 1, 0):
    wb, s = _bf(ws[l]), STRIDES[l]
    dx, dw, db = _grads64(ins[l], wb, s, douts[l])
    ax, aw, ab = _grads64(ins[l].abs(), wb.abs(), s, douts[l].abs())
    P = douts[l][..., 0].numel()
    scale = 255.0 if l == 0 else 1.0
    tw = (P + 8) * EPS * aw / scale + (EPS * dw.abs() / scale if l == 0 else 0)
    assert bool(((k['dw'][l] - dw / scale).abs() <= tw).all()), l
    assert bool(((k['db'][l] - db).abs() <= (P + 8) * EPS * ab).all()), l
    if l > 0:
      K = 4 * wb.shape[3]
      ref = dx * (ins[l] > 0)
      got = (k['da1'], k['da2'])[l - 1].double()
      assert bool(((got - ref).abs() <= 2.0 ** -8 * ref.abs() + (K + 8) * EPS * ax).all()), l


@pytest.mark.parametrize('n,cap', CASES)
@pytest.mark.parametrize('shape', SHAPES)
def test_exact_integers(cuda, shape, n, cap):
  """Bytes in {0, 255}, sparse +-1 weights, integer biases, dfeats in
  {-1, 0, 1}: every rounded value is an integer <= 256 and every gradient sum
  stays below 2^24 (asserted on the float64 chain first), so bf16 and fp32 are
  exact and every tensor EQUALS float64 - masks at pre-activations of exactly
  0 and the asymmetric pads included."""
  ws, bs = O.integer_weights(shape[2], 1)
  frames = O.binary_frames(shape, n, seed=9)
  g = torch.Generator().manual_seed(3)
  dfeats = torch.randint(-1, 2, (n,) + O.out_shape(shape), generator=g).float()
  acts, x, zeros = [], frames.double() / 255.0, 0
  for l in range(3):
    pre = _conv64(x, ws[l].double(), STRIDES[l]) + bs[l].double()
    zeros += int((pre == 0).sum())
    x = pre.clamp(min=0)
    acts.append(x)
  dy3 = dfeats.double() * (acts[2] > 0)
  da2, dw3, db3 = _grads64(acts[1], ws[2].double(), 2, dy3)
  da2 = da2 * (acts[1] > 0)
  da1, dw2, db2 = _grads64(acts[0], ws[1].double(), 2, da2)
  da1 = da1 * (acts[0] > 0)
  _, dw1, db1 = _grads64(frames.double() / 255.0, ws[0].double(), 4, da1)
  assert zeros > 0
  for t in acts + [da2, da1]:
    assert torch.equal(t, t.round()) and t.abs().max().item() <= 256
  for a, l, d in ((frames.double(), 0, da1), (acts[0], 1, da2), (acts[1], 2, dy3)):
    # inputs >= 0: the weight gradient of |dOut| is the sum of absolute products
    assert _grads64(a, ws[l].double(), STRIDES[l], d.abs())[1].max().item() < 2 ** 24
    assert d.abs().sum(dim=(0, 1, 2)).max().item() < 2 ** 24
  k = _run(_C(), cuda, frames, ws, bs, dfeats, cap)
  want = dict(feats=acts[2], a1=acts[0], a2=acts[1], dy3=dy3, da2=da2, da1=da1)
  for name, ref in want.items():
    assert torch.equal(k[name].double(), ref), name
  for l, (dw, db) in enumerate(((dw1, db1), (dw2, db2), (dw3, db3))):
    assert torch.equal(k['dw'][l], dw), l
    assert torch.equal(k['db'][l], db), l


@pytest.mark.parametrize('shape', [(72, 96, 3), (84, 84, 4)])
def test_public_path_and_determinism(cuda, shape):
  """Agent(torso_dtype='bf16') under autograd on a [T + 1 = 3, B = 2] batch
  with direct gradient sinks: the three families run, the conv gradients in
  the flat buffer are bitwise the raw op chain's, twice the same bits;
  torso_dtype='auto' runs none of them."""
  from scalable_agent_amd import optim
  from scalable_agent_amd.ops import grad_sink
  C = _C()
  g = torch.Generator().manual_seed(17)
  frames = torch.randint(0, 256, (3, 2) + tuple(shape), generator=g,
                         dtype=torch.uint8).to(cuda)
  fams = ['shallow_bf16_' + f for f in ('train_fwd', 'bwd_data', 'wgrad')]

  def step(torso_dtype):
    agent = Agent(9, torso='shallow', frame_shape=shape, seed=5, backend='hip',
                  torso_dtype=torso_dtype).to(cuda)
    flat = optim.FlatParams(agent)
    seen = []
    with grad_sink.direct_grads():
      feats = agent.conv_features(frames.reshape((6,) + tuple(shape)))
      feats.register_hook(seen.append)
      agent.torso_fc(feats).square().sum().backward()
    return agent, flat, feats.detach(), seen[0]

  _run(C, cuda, *_random_inputs(shape, 1), 0)  # the records now say one image
  auto = step('auto')
  assert [C.conv_launch_info(f)['ntiles'] for f in fams] == [1, 1, 1]
  agent, flat, feats, dfeats = step('bf16')
  assert [C.conv_launch_info(f)['ntiles'] for f in fams] == [6, 6, 6]
  assert feats.dtype == torch.float32 and not torch.equal(feats, auto[2])
  again = step('bf16')
  assert torch.equal(flat.grads, again[1].grads)
  ws = [agent._conv_params(sp['name'])[0].detach().cpu() for sp in agent.specs]
  bs = [agent._conv_params(sp['name'])[1].detach().cpu() for sp in agent.specs]
  k = _run(C, cuda, frames.reshape((6,) + tuple(shape)).cpu(), ws, bs,
           dfeats.reshape((6,) + O.out_shape(shape)).cpu(), 0)
  assert torch.equal(k['feats'].reshape(6, -1), feats.cpu())
  for l, sp in enumerate(agent.specs):
    for kind, ref in (('__w', k['dw'][l]), ('__b', k['db'][l])):
      got = flat.view_of(flat.grads, 'convnet.' + sp['name'] + kind)
      assert torch.equal(got.double().cpu(), ref), (l, kind)
