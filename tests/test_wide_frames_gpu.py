"""Wide frames (5..16 channels) on the fp32 torsos (csrc/kernels/conv_wide.hip and
the Cp instances of the direct kernels) against float64.  Forward bound: (M + 5)
2^-24 sum |x||w| (tests/_conv_f32_oracle.bound); scatter gradient: (tiles + 10)
2^-24 sum |dP||x|.  Random forward seeds have every pool window's maximum clear
of the runner-up by more than twice the conv bound (checked on the CPU)."""

import pytest
import torch

from tests import _conv_f32_oracle as O
from tests import _discontinuity

pytestmark = pytest.mark.gpu

WIDE_C = [5, 8, 12, 13, 16]
MAPS = [(7, 9), (10, 12)]
N = 5


def _cp(c):
  return (c + 3) // 4 * 4


def _capped(C, cap, fn, *a, **kw):
  prev = C.cf32_grid_cap(cap)
  try:
    return fn(*a, **kw)
  finally:
    C.cf32_grid_cap(prev)


def _pad_c(t, cp):
  return torch.cat([t, t.new_zeros(t.shape[:-1] + (cp - t.shape[-1],))], -1)


@pytest.mark.parametrize('W', [1, 5, 7])
@pytest.mark.parametrize('c', [5, 8, 13, 16])
def test_wide_frame_conversion(cuda, c, W):
  C = O.ext()
  g = O.gen(100 * c + W)
  n = max(2, -(-256 // (3 * W * c)))  # frames of 3 x W: enough for every byte value
  x = torch.randint(0, 256, (n, 3, W, c), generator=g, dtype=torch.uint8)
  flat = x.view(-1)
  flat[torch.randperm(flat.numel(), generator=g)[:256]] = torch.arange(256, dtype=torch.uint8)
  assert len(torch.unique(x)) == 256
  buf = torch.full((n + 2, 3, W, c), 127, dtype=torch.uint8, device=cuda)
  buf[1:1 + n] = x.to(cuda)
  y = C.cf32_frames_f32(buf[1:1 + n])
  assert C.cf32_launch_info(True)['family'] == 'frames_wide'
  ref = _pad_c((x.double() / 255).float(), _cp(c))
  assert torch.equal(y.cpu(), ref)
  assert bool((buf[0] == 127).all()) and bool((buf[-1] == 127).all())
  assert torch.equal(buf[1:1 + n].cpu(), x)


def _fwd_case(c, H, W, exact, seed):
  g = O.gen(seed)
  # the 96-wide map (several bands per image: the band seams) on two frames
  fr = O.frames(g, (2 if W == 96 else N, H, W, c), exact)
  w = O.weights(g, (3, 3, c, 16), exact)
  b = O.weights(g, (16,), exact)
  x64 = fr.double() / 255.0
  pre = O.conv(x64, w.double(), b.double(), 1)
  A = O.conv(x64.abs(), w.double().abs(), b.double().abs(), 1)
  return fr, w, b, pre, O.bound(9 * _cp(c), A)


def _clear_seed(c, H, W):
  """First seed whose pool windows are all clear of fp32 rounding (CPU)."""
  for seed in range(1000 * c, 1000 * c + 50):
    fr, w, b, pre, bnd = _fwd_case(c, H, W, False, seed)
    win, _, _ = O.pool_windows(pre)
    bwin, _, _ = O.pool_windows(bnd)
    if bool(O.argmax_clear(win, bwin.clamp(min=0)).all()):
      return seed
  raise AssertionError('no pool-tie-free seed')


@pytest.mark.parametrize('cap', [0, 3])
@pytest.mark.parametrize('H,W', MAPS + [(10, 96)])
@pytest.mark.parametrize('c', WIDE_C)
def test_wide_stage0_forward(cuda, c, H, W, cap):
  C = O.ext()
  cp = _cp(c)
  pbh, pbw = O.same_pads(H, 3, 2)[0], O.same_pads(W, 3, 2)[0]
  for exact in (True, False):
    fr, w, b, pre, bnd = _fwd_case(c, H, W, exact, 7 if exact else _clear_seed(c, H, W))
    ref, code = O.maxpool(pre)
    x = C.cf32_frames_f32(fr.to(cuda))
    wp = _pad_c(w.permute(0, 1, 3, 2), cp).permute(0, 1, 3, 2).contiguous().to(cuda)
    y, arg = _capped(C, cap, C.cf32_conv_pool_fwd, x, wp, b.to(cuda), pbh, pbw)
    info = C.cf32_launch_info(True)
    assert info['family'] == 'wide_conv_pool', info
    if cap:
      assert info['grid_x'] == cap and info['ntiles'] > cap
    if W == 96:
      assert info['tiles_per_img'] > 1
    assert torch.equal(arg.cpu().long(), code)
    if exact:
      assert torch.equal(O.d64(y), ref)
    else:
      pb = O.pool_windows(bnd)[0].gather(-1, code.unsqueeze(-1)).squeeze(-1)  # at the argmax
      r = O.ratio(y, ref, pb)
      assert r <= 1.0
    # the dense chain on the same image, where its conv runs the direct kernel
    conv = C.cf32_conv_fwd(x, wp, b.to(cuda), 1, 1, 1, H, W)
    if C.cf32_launch_info(True)['family'] == 'conv_fwd':
      yd, ad = C.cf32_maxpool_fwd(conv, pbh, pbw)
      assert torch.equal(y, yd) and torch.equal(arg, ad)


@pytest.mark.parametrize('cap', [0, 3])
@pytest.mark.parametrize('c', WIDE_C)
def test_wide_stage0_scatter_wgrad(cuda, c, cap):
  C = O.ext()
  H, W = 10, 12
  pbh, pbw = O.same_pads(H, 3, 2)[0], O.same_pads(W, 3, 2)[0]
  Hp, Wp = O.same_out(H, 2), O.same_out(W, 2)
  for exact in (True, False):
    g = O.gen(31 * c + exact)
    fr = O.frames(g, (N, H, W, c), exact)
    dP = O.acts(g, (N, Hp, Wp, 16), exact)
    # codes of a real pool, so no argmax lies in the pool's padding
    _, code = O.maxpool(torch.randn((N, H, W, 16), generator=g).double())
    x64 = fr.double() / 255.0
    dconv = O.pool_gather(dP.double(), code, H, W)
    dw_ref, db_ref = O.conv_wgrad(x64, dconv, 3, 1)
    mag, _ = O.conv_wgrad(x64.abs(), dconv.abs(), 3, 1)
    x = C.cf32_frames_f32(fr.to(cuda))
    outs = []
    for _ in range(2):
      dw = torch.zeros(3, 3, c, 16, device=cuda)
      db = torch.zeros(16, device=cuda)
      _capped(C, cap, C.cf32_conv_wgrad, x, dP.to(cuda), 1, 1, 1, False, dw, db,
              pool_arg=code.to(torch.uint8).to(cuda), pool_pbh=pbh, pool_pbw=pbw)
      info = C.cf32_launch_info(True)
      assert info['family'] == 'wide_pool_wgrad', info
      if cap:
        assert info['grid_x'] == cap and info['ntiles'] > 2 * cap
      outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dw, db = outs[0]
    assert tuple(dw.shape) == (3, 3, c, 16)
    if exact:
      assert O.exact_ok(mag)
      assert torch.equal(O.d64(dw), dw_ref) and torch.equal(O.d64(db), db_ref)
    else:
      tiles = N * -(-Hp // 2)
      r = O.ratio(dw, dw_ref, (tiles + 10) * O.U * mag)
      rb = O.ratio(db, db_ref, (tiles + 10) * O.U * dconv.abs().sum((0, 1, 2)))
      assert r <= 1.0 and rb <= 1.0


@pytest.mark.parametrize('c', [5, 12, 16])
def test_wide_shallow_layer1(cuda, c):
  """The 8x8/4 layer (Cp -> 32): forward and C-channel wgrad, direct-conv bound."""
  C = O.ext()
  n, H, W = 3, 16, 20
  g = O.gen(77 + c)
  fr = O.frames(g, (n, H, W, c), False)
  w, b = O.weights(g, (8, 8, c, 32), False), O.weights(g, (32,), False)
  x64 = fr.double() / 255.0
  (pt, _), (pl, _) = O.same_pads(H, 8, 4), O.same_pads(W, 8, 4)
  Ho, Wo = O.same_out(H, 4), O.same_out(W, 4)
  x = C.cf32_frames_f32(fr.to(cuda))
  wp = _pad_c(w.permute(0, 1, 3, 2), _cp(c)).permute(0, 1, 3, 2).contiguous().to(cuda)
  y = C.cf32_conv_fwd(x, wp, b.to(cuda), 4, pt, pl, Ho, Wo)
  A = O.conv(x64, w.double().abs(), b.double().abs(), 4)
  r = O.ratio(y, O.conv(x64, w.double(), b.double(), 4), O.bound(64 * _cp(c), A))
  dy = O.acts(g, (n, Ho, Wo, 32), False)
  dw, db = torch.zeros(8, 8, c, 32, device=cuda), torch.zeros(32, device=cuda)
  C.cf32_conv_wgrad(x, dy.to(cuda), 4, pt, pl, False, dw, db)
  dw_ref, db_ref = O.conv_wgrad(x64, dy.double(), 8, 4)
  mag, magb = O.conv_wgrad(x64, dy.double().abs(), 8, 4)
  rw = O.ratio(dw, dw_ref, O.bound(n * Ho * Wo, mag))
  rb = O.ratio(db, db_ref, O.bound(n * Ho * Wo, magb))
  assert max(r, rw, rb) <= 1.0


def _walk64(agent, frames):
  """Float64 torso from agent's parameters: features, their magnitude sums (sum
  |x||w| + |b| of the last conv, + |skip|), the first conv's output (a leaf: its
  grad is that conv's float64 dY) and K = the sum over the convs of M + 5, M =
  k k max(Cin, Cout) (a conv's forward and its data gradient).  A worst case
  passed on through |w| of every layer exceeds the values themselves, so the
  per-layer constants are summed and applied to the last magnitude sums."""
  from scalable_agent_amd.models import layers
  P = {k: v.detach().double().cpu() for k, v in agent.convnet.items()}
  x = frames.double() / 255.0
  st = {'A': None, 'K': 0, 'first': None}

  def conv(x, name, s):
    w, b = P[name + '__w'], P[name + '__b']
    m = w.shape[0] ** 2 * max(_cp(w.shape[2]), w.shape[3]) + 5
    st['K'] += m
    st['A'] = layers.conv2d_same_nhwc(x.detach().abs(), w.abs(), b.abs(), s)
    y = layers.conv2d_same_nhwc(x, w, b, s)
    if st['first'] is None:
      st['first'] = y.requires_grad_()
    return y

  for sp in agent.specs:
    if sp['kind'] == 'conv':
      x = conv(x, sp['name'], sp['s'])
      x = x.clamp(min=0) if sp['relu_out'] else x
    elif sp['kind'] == 'pool':
      x = layers.maxpool_same_nhwc(x, 3, 2)
    else:
      xin = x
      for sub in ('conv_2d', 'conv_2d_1'):
        x = conv(x.clamp(min=0), sp['name'] + '__' + sub, 1)
      x, st['A'] = x + xin, st['A'] + xin.detach().abs()
  return x.clamp(min=0).flatten(1), st['A'].flatten(1), st['first'], st['K']


@pytest.mark.parametrize('torso', ['deep', 'shallow'])
def test_wide_agent(cuda, torso):
  """Features inside K 2^-24 of their magnitude sums; the first conv's dW / db
  inside (K + kw) 2^-24 sum |x||dY|, kw the gradient kernel's own term (scatter:
  tiles + 10; dense: terms + 5); torso_blocks='whole' bitwise the same."""
  from scalable_agent_amd.models import Agent
  shape = (16, 20, 12)
  agent = Agent(9, torso=torso, frame_shape=shape, backend='hip', seed=3).to(cuda)
  for seed in range(50):
    frames = torch.randint(0, 256, (4,) + shape, generator=O.gen(seed), dtype=torch.uint8)
    if _discontinuity.count(agent, frames) == 0:
      break
  else:
    raise AssertionError('no discontinuity-free frames')
  ref, mag, first, K = _walk64(agent, frames)
  feats = agent.conv_features(frames.to(cuda))
  assert O.ratio(feats, ref.detach(), K * O.U * mag) <= 1.0
  cot = torch.randn(ref.shape, generator=O.gen(5), dtype=torch.float64)
  w0, b0 = agent._conv_params('conv_2d')
  gw, gb = torch.autograd.grad(feats, (w0, b0), cot.float().to(cuda))
  dy, = torch.autograd.grad(ref, first, cot)
  k, s = w0.shape[0], 1 if torso == 'deep' else 4
  x64 = frames.double() / 255.0
  rw, rb = O.conv_wgrad(x64, dy, k, s)
  mw, mb = O.conv_wgrad(x64, dy.abs(), k, s)
  kw = 4 * 4 + 10 if torso == 'deep' else 4 * dy.shape[1] * dy.shape[2] + 5
  assert tuple(gw.shape) == (k, k, 12, w0.shape[3])
  r = (O.ratio(gw, rw, (K + kw) * O.U * mw), O.ratio(gb, rb, (K + kw) * O.U * mb))
  assert max(r) <= 1.0
  whole = Agent(9, torso=torso, frame_shape=shape, backend='hip', seed=3,
                torso_blocks='whole').to(cuda)
  whole.load_state_dict(agent.state_dict())
  with torch.no_grad():
    assert torch.equal(whole.conv_features(frames.to(cuda)), feats.detach())
