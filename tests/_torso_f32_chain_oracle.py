"""Float64 CPU oracle of the two fp32 torsos as NETWORKS (test helper of
test_torso_f32_chain_oracle.py on the CPU and test_torso_f32_chain_gpu.py on
the GPU).

Deep torso: the layer functions and the chain of _torso_chain_oracle.py with
rnd=None (exact float64, x = frames / 255, the model's weights).  Shallow
torso (added here): three convs 8x8/4, 4x4/2, 3x3/2, each bias + ReLU, TF-SAME
pads including the asymmetric one, from the plain tap loops of
_conv_f32_oracle.py.  The wiring is read from agent.specs and every parameter
is fetched by name from agent.convnet; nothing here looks at
scalable_agent_amd.ops.conv_f32 (whose parameter lists, index arithmetic,
saved tensors and flags are what the GPU test checks).

Bounds.  Nothing is fitted: for every conv output (y, t, dt, dx) the bound is
the LARGER of the direct kernels' bound _conv_f32_oracle.bound(M, A) and the
Winograd kernels' bound _wino_oracle.bound_fwd(cin, mag), elementwise, so it
holds whichever family the launcher picks; the same for dw / db with
bound(N Ho Wo, A) and _wino_oracle.bound_wg.  The strided shallow convs have
no Winograd instance: the direct bound alone.  The channel count of the first
layer is the staged one (4: the fp32 image's pad channel is a k-step of the
chain like the others), as in the per-kernel oracles' f32-image cases.
"""

import functools

import torch

from tests import _conv_f32_oracle as F32
from tests import _conv_oracle as O
from tests import _torso_chain_oracle as T
from tests import _wino_oracle as WO

# frame shape, images, seed.  The seeds are the first tried (3.. in order); no
# seed had to be skipped for the conditions of test_torso_f32_chain_oracle.py.
DEEP_CASES = [((26, 30, 3), 3, 3), ((21, 19, 4), 3, 4), ((72, 96, 3), 2, 5),
              ((84, 84, 4), 2, 6)]
SHALLOW_CASES = [((20, 26, 3), 3, 7), ((84, 84, 4), 2, 8), ((72, 96, 3), 2, 9)]


def make_agent(torso, frame_shape, seed):
  """fp32 HIP agent with seed-fixed init and non-zero biases."""
  from scalable_agent_amd.models import Agent
  agent = Agent(9, torso=torso, frame_shape=frame_shape, seed=seed,
                backend='hip', compute_dtype=torch.float32)
  g = torch.Generator().manual_seed(seed + 1000003)
  with torch.no_grad():
    for name, p in agent.convnet.items():
      if name.endswith('__b'):
        p.copy_(torch.randn(p.shape, generator=g) * 0.1)
  return agent


def make_inputs(frame_shape, N, seed, flat):
  """(uint8 frames [N, H, W, C], fp32 N(0, 1) feature gradient [N, flat])."""
  g = torch.Generator().manual_seed(seed + 77)
  frames = torch.randint(0, 256, (N,) + tuple(frame_shape), generator=g,
                         dtype=torch.uint8)
  return frames, torch.randn(N, flat, generator=g)


@functools.lru_cache(maxsize=None)
def case(torso, frame_shape, N, seed):
  """(agent on the CPU, frames, g): built once per process, never modified."""
  agent = make_agent(torso, frame_shape, seed)
  frames, g = make_inputs(frame_shape, N, seed, agent.flat_size)
  return agent, frames, g


# ------------------------------------------------------------- shallow torso

def shallow_layers(agent):
  """[(conv name, K, S)] in the order of agent.specs."""
  out = []
  for sp in agent.specs:
    assert sp['kind'] == 'conv' and sp['relu_out'], sp
    out.append((sp['name'], sp['k'], sp['s']))
  assert [(k, s) for _, k, s in out] == [(8, 4), (4, 2), (3, 2)]
  return out


def shallow_params64(agent):
  return {n: (O.d64(agent.convnet[n + '__w']), O.d64(agent.convnet[n + '__b']))
          for n, _, _ in shallow_layers(agent)}


def sh_fwd(x, w, b, S):
  """relu(conv(x) + b): (ref, A)."""
  return F32.conv(x, w, b, S).relu(), F32.conv(x.abs(), w.abs(), b.abs(), S)


def sh_dgrad(dy, w, S, x):
  """Gradient at the PRE-activation of the layer that produced x = relu(.):
  (dx, A) of conv(x, w, S), masked by x > 0."""
  H, W = x.shape[1], x.shape[2]
  return (F32.conv_dgrad(dy, w, S, H, W, mask=x),
          F32.conv_dgrad(dy.abs(), w.abs(), S, H, W, mask=x))


def shallow_forward_chain(agent, frames, P=None):
  """acts[0] = frames / 255, acts[i + 1] = relu(conv_i(acts[i]) + b_i)."""
  P = P or shallow_params64(agent)
  layers = shallow_layers(agent)
  acts = [O.d64(frames) / 255.0]
  for n, _, S in layers:
    acts.append(sh_fwd(acts[-1], P[n][0], P[n][1], S)[0])
  out = acts[-1]
  return dict(layers=layers, P=P, acts=acts, out=out,
              feats=out.reshape(out.shape[0], -1))


def shallow_backward_chain(rec, g):
  """{param name: gradient} of sum(feats * g)."""
  layers, P, acts = rec['layers'], rec['P'], rec['acts']
  out = rec['out']
  dy = T.final_relu_bwd(O.d64(g).reshape(out.shape), out)
  grads = {}
  for i in reversed(range(len(layers))):
    n, K, S = layers[i]
    grads[n + '__w'], grads[n + '__b'] = F32.conv_wgrad(acts[i], dy, K, S)
    if i > 0:
      dy = sh_dgrad(dy, P[n][0], S, acts[i])[0]
  return grads


# -------------------------------------------------------------------- bounds

def _staged(c):
  return max(c, 4)


def _emax(a, b):
  return torch.maximum(a, b)


def conv_bound(x, w, b, add=None):
  """3x3 / 1 forward: bias + optional residual add in the magnitude."""
  c = _staged(x.shape[3])
  extra = b.abs() if add is None else b.abs() + add.abs()
  A = O.conv64(x.abs(), w.abs()) + extra
  Aw = WO.mag_fwd(x, w) + extra
  return _emax(F32.bound(9 * c, A), WO.bound_fwd(c, Aw))


def dgrad_bound(dy, w, m=None, add=None, absdy=None):
  """3x3 / 1 data gradient [* m] [+ add].  absdy: the magnitude of a dY that
  is itself a sum (the pool-gradient gather)."""
  c = dy.shape[3]
  a = dy.abs() if absdy is None else absdy
  A = O.dgrad64(a, w.abs())
  Aw = WO.mag_fwd(a, WO.flip_t(w))
  if m is not None:
    A, Aw = m * A, m * Aw
  if add is not None:
    A, Aw = A + add.abs(), Aw + add.abs()
  return _emax(F32.bound(9 * c, A), WO.bound_fwd(c, Aw))


def wgrad_bounds(x, dy, dw0, db0, absdy=None):
  """(dw bound, db bound) of a 3x3 / 1 conv's accumulated weight gradients;
  dw0 / db0: the views' content before (part of the magnitude)."""
  N, H, W, _ = x.shape
  a = dy.abs() if absdy is None else absdy
  cin = dw0.shape[2]
  TY, TX = WO.tiles_of(H, W)
  A = O.wgrad64(x.abs(), a)[:, :, :cin] + dw0.abs()
  Aw = WO.mag_wgrad(x, a)[:, :, :cin] + dw0.abs()
  Ab = a.sum(dim=(0, 1, 2)) + db0.abs()
  return (_emax(F32.bound(N * H * W, A), WO.bound_wg(N * TY * TX, Aw)),
          _emax(F32.bound(N * H * W, Ab), WO.bound_wg(N * H * W, Ab)))


def pool_check_terms(y, B, pads):
  """For a head conv y with elementwise bound B: (window max, first maximal
  tap, the largest bound in each window, the windows whose argmax is clear)."""
  win = O.pool_taps(y, *pads)
  wb = O.pool_taps(B, *pads, fill=0.0)
  val, code = O.pool64(y, *pads)
  return val, code, wb.max(dim=-1).values, F32.argmax_clear(win, wb)


def pool_gather_f32(dP32, code, H, W, pads):
  """maxpool_bwd in fp32 as the kernels add: the (at most four) windows that
  chose a cell are added one by one in ascending (py, px) order, i.e. in
  descending tap order, starting from zero."""
  assert dP32.dtype == torch.float32
  N, Hp, Wp, C = dP32.shape
  dxp = torch.zeros(N, 2 * Hp + 1, 2 * Wp + 1, C, dtype=torch.float32)
  zero = torch.zeros_like(dP32)
  for dy in (2, 1, 0):
    for dx in (2, 1, 0):
      F32._taps(dxp, dy, dx, Hp, Wp, 2).add_(torch.where(code == dy * 3 + dx, dP32, zero))
  return dxp[:, pads[0]:pads[0] + H, pads[1]:pads[1] + W].clone()
