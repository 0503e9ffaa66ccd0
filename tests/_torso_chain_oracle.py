"""Float64 CPU oracle of the deep torso as a NETWORK (test helper).

_conv_oracle.py holds the single operations (conv64, dgrad64, wgrad64,
pool64, scatter64).  Here they are composed into the layers of the deep
ResNet torso, forward and backward, and into the whole chain.  The wiring is
read from the model definition: `stages_of` walks agent.specs and every
parameter is fetched by its name from agent.convnet; nothing here looks at
scalable_agent_amd.ops.conv (whose parameter order, saved tensors and flags
are what test_deep_torso_chain_gpu.py checks).  test_torso_chain_oracle.py
ties the chain to Agent(backend='torch', compute_dtype=float64) under
autograd to 1e-10.

Every layer function returns float64 NHWC tensors; the forward and dgrad
functions return (ref, A) with A the same layer applied to magnitudes, the
scale of _conv_oracle.check_bound's accumulation term.

Rounding.  `forward_chain` / `backward_chain` take `rnd`, applied where the
bf16 kernels round: the head conv before its pool (the kernels pool bf16
values, first maximal tap wins), t, y, the masked upstream gradient, dt, dx
and the gathered dY of a stage head.  rnd=None is the exact chain; rnd=bf16
is the emulated chain of the GPU test's end-to-end number.  `kernel_weights`
gives the weights as the kernels see them.
"""

import torch

from tests import _conv_oracle as O


def bf16(x):
  """Round to bf16 and back (torch converts through fp32, round to nearest
  even, which is what the kernels' fp32 -> bf16 conversion does)."""
  return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def stages_of(agent):
  """[{head, cin, cout, blocks: [(conv_2d name, conv_2d_1 name), ...]}] in
  the order of agent.specs (deep torso: conv, pool, residual blocks)."""
  stages = []
  for sp in agent.specs:
    if sp['kind'] == 'conv':
      assert sp['k'] == 3 and sp['s'] == 1 and not sp['relu_out'], sp
      stages.append(dict(head=sp['name'], cin=sp['cin'], cout=sp['cout'],
                         pool=False, blocks=[]))
    elif sp['kind'] == 'pool':
      assert not stages[-1]['blocks']
      stages[-1]['pool'] = True
    else:
      assert sp['kind'] == 'res' and sp['ch'] == stages[-1]['cout'], sp
      stages[-1]['blocks'].append((sp['name'] + '__conv_2d',
                                   sp['name'] + '__conv_2d_1'))
  assert all(st['pool'] for st in stages)
  return stages


def conv_names(agent):
  """Names of all conv layers in model order."""
  out = []
  for st in stages_of(agent):
    out.append(st['head'])
    for pair in st['blocks']:
      out += list(pair)
  return out


def params64(agent):
  """{conv name: (w, b)} in float64, looked up by name."""
  return {n: (O.d64(agent.convnet[n + '__w']), O.d64(agent.convnet[n + '__b']))
          for n in conv_names(agent)}


def kernel_weights(agent):
  """{conv name: w} as the bf16 kernels use them.  Every kernel converts its
  fp32 master weights with one fp32 -> bf16 conversion, round to nearest even
  (conv_common.h f2bf / load_weights4).  The first layer folds x / 255 into
  the weight first: bf16(fl32(w * fl32(1 / 255))), applied to the raw uint8
  frame (exact in bf16)."""
  stages = stages_of(agent)
  out = {}
  for n in conv_names(agent):
    w = agent.convnet[n + '__w'].detach().to('cpu', torch.float32)
    if n == stages[0]['head']:
      w = w * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    out[n] = w.to(torch.bfloat16).to(torch.float64)
  return out


# ------------------------------------------------------------ forward layers

def head_conv(x, w, b):
  """Stage head before its pool: conv(x) + b."""
  return O.conv64(x, w, b), O.conv64(x.abs(), w.abs(), b.abs())


def head_pool(y):
  """3x3 / 2 SAME max-pool: (pooled, code, (pb_h, pb_w))."""
  pads = (O.pool_pb(y.shape[1]), O.pool_pb(y.shape[2]))
  pooled, code = O.pool64(y, *pads)
  return pooled, code, pads


def res_t(xa, w1, b1):
  """First conv of a residual block, stored ReLU'd:
  t = relu(conv(relu(xa)) + b1)."""
  xr = xa.relu()
  return O.conv64(xr, w1, b1).relu(), O.conv64(xr, w1.abs(), b1.abs())


def res_y(t, w2, b2, xa):
  """Second conv plus the skip: y = conv(t) + b2 + xa (t is already
  relu(conv1))."""
  return (O.conv64(t, w2, b2) + xa,
          O.conv64(t.abs(), w2.abs(), b2.abs()) + xa.abs())


def final_relu(y):
  return y.relu()


# ----------------------------------------------------------- backward layers

def final_relu_bwd(g, out):
  return g * (out > 0)


def res_y_bwd(dy, t, w2):
  """Backward of y = conv(t) + b2 + xa to t's pre-activation:
  (dt, A, dw2, db2); the skip's share of dy is added by res_t_bwd."""
  m = (t > 0).to(torch.float64)
  return (m * O.dgrad64(dy, w2), m * O.dgrad64(dy.abs(), w2.abs()),
          O.wgrad64(t.relu(), dy), dy.sum(dim=(0, 1, 2)))


def res_t_bwd(dt, xa, w1, dy):
  """Backward of t = relu(conv(relu(xa)) + b1), plus the skip gradient dy:
  (dx, A, dw1, db1)."""
  m = (xa > 0).to(torch.float64)
  return (m * O.dgrad64(dt, w1) + dy,
          m * O.dgrad64(dt.abs(), w1.abs()) + dy.abs(),
          O.wgrad64(xa.relu(), dt), dt.sum(dim=(0, 1, 2)))


def head_gather(dP, code, H, W, pads):
  """dY of the head conv: every pooled gradient at its argmax tap.  Returns
  (dY, S, cnt): S the same sum over magnitudes, cnt the number of windows
  that landed on each cell."""
  dY = O.scatter64(dP, code, H, W, *pads)
  S = O.scatter64(dP.abs(), code, H, W, *pads)
  cnt = O.scatter64(torch.ones_like(dP), code, H, W, *pads)
  return dY, S, cnt


def head_bwd(dY, x, w, need_dx=True):
  """Backward of the head conv: (dx, A, dw, db); dx / A None for conv1."""
  dx = A = None
  if need_dx:
    dx, A = O.dgrad64(dY, w), O.dgrad64(dY.abs(), w.abs())
  return dx, A, O.wgrad64(x, dY), dY.sum(dim=(0, 1, 2))


# ----------------------------------------------------------------- the chain

def _id(x):
  return x


def pool_fragile(y, a, pads):
  """Windows of the bf16 pool whose winner could change if every tap moved
  by up to its accumulation bound a before the rounding: with k the first
  maximal tap of bf16(y), some other tap j has bf16(y_j + a_j) above
  bf16(y_k - a_k), or equal to it with j < k (the first maximal tap wins)."""
  mid = O.pool_taps(bf16(y), *pads)
  lo = O.pool_taps(bf16(y - a), *pads)
  hi = O.pool_taps(bf16(y + a), *pads)
  _, k = O.pool64(bf16(y), *pads)
  assert torch.equal(mid.gather(-1, k.unsqueeze(-1)).squeeze(-1), mid.max(dim=-1).values)
  lo_k = lo.gather(-1, k.unsqueeze(-1))
  j = torch.arange(9).view(1, 1, 1, 1, 9)
  kk = k.unsqueeze(-1)
  frag = (j != kk) & ((hi > lo_k) | ((j < kk) & (hi == lo_k)))
  return int(frag.any(dim=-1).sum())


def relu_fragile(z, a):
  """Pre-activations within their accumulation bound of zero."""
  return int((z.abs() <= a).sum())


def forward_chain(agent, frames, rnd=None, P=None):
  """The whole torso on uint8 frames.  Returns a record:
    heads[s]  = {x, y, pooled, code, pads}
    blocks[s] = [{xa, t, y}, {xa, t, y}]
    pre       = last block's y, out = relu(pre), feats = out flattened.
  rnd=None: exact float64 (x = frames / 255, the model's weights).  With
  rnd: the kernels' operands (raw frames and kernel_weights) and roundings."""
  rnd_ = rnd or _id
  stages = stages_of(agent)
  P = P or params64(agent)
  if rnd is None:
    Wt = {n: P[n][0] for n in P}
    x = O.d64(frames) / 255.0
  else:
    Wt = kernel_weights(agent)
    x = O.d64(frames)
  rec = dict(stages=stages, P=P, W=Wt, heads=[], blocks=[],
             x0=O.d64(frames) / 255.0)
  fragile = 0
  for si, st in enumerate(stages):
    K = st['cin']
    y, A = head_conv(x, Wt[st['head']], P[st['head']][1])
    if rnd is not None:
      a = 9 * K * O.ACC * A
      pads = (O.pool_pb(y.shape[1]), O.pool_pb(y.shape[2]))
      fragile += pool_fragile(y, a, pads)
      # the pooled value's sign is block 0's ReLU mask
      fragile += relu_fragile(O.pool64(y, *pads)[0],
                              O.pool_taps(a, *pads, fill=0.0).max(dim=-1).values)
    y = rnd_(y)
    pooled, code, pads = head_pool(y)
    rec['heads'].append(dict(x=x, y=y, pooled=pooled, code=code, pads=pads))
    xa = pooled
    blocks = []
    K = st['cout']
    for bi, (n1, n2) in enumerate(st['blocks']):
      final = si == len(stages) - 1 and bi == len(st['blocks']) - 1
      t, tA = res_t(xa, Wt[n1], P[n1][1])
      if rnd is not None:
        fragile += relu_fragile(O.conv64(xa.relu(), Wt[n1], P[n1][1]),
                                9 * K * O.ACC * tA)
      t = rnd_(t)
      y, yA = res_y(t, Wt[n2], P[n2][1], xa)
      # y's sign is a ReLU mask in the next block and in the final ReLU; a
      # stage's last y feeds the next head conv without one
      if rnd is not None and (final or bi < len(st['blocks']) - 1):
        fragile += relu_fragile(y, 9 * K * O.ACC * yA)
      if final:
        rec['pre'] = y  # the kernel applies the final ReLU before rounding
        y = final_relu(y)
      y = rnd_(y)
      blocks.append(dict(xa=xa, t=t, y=y))
      xa = y
    rec['blocks'].append(blocks)
    x = xa
  rec['fragile'] = fragile
  rec['out'] = x
  rec['feats'] = x.reshape(x.shape[0], -1)
  return rec


def backward_chain(rec, g, rnd=None):
  """{param name: gradient} of sum(feats * g), names as in agent.convnet
  ('<conv>__w', '<conv>__b'), plus '_dy' = [(tag, tensor)] of every
  activation gradient in the order it is formed."""
  rnd_ = rnd or _id
  stages, P, Wt = rec['stages'], rec['P'], rec['W']
  out = rec['out']
  grads, trace = {}, []
  dy = final_relu_bwd(rnd_(O.d64(g).reshape(out.shape)), out)
  trace.append(('mask', dy))
  for si in reversed(range(len(stages))):
    st = stages[si]
    for bi in reversed(range(len(st['blocks']))):
      n1, n2 = st['blocks'][bi]
      blk = rec['blocks'][si][bi]
      dt, _, dw2, db2 = res_y_bwd(dy, blk['t'], Wt[n2])
      dt = rnd_(dt)
      grads[n2 + '__w'], grads[n2 + '__b'] = dw2, db2
      dx, _, dw1, db1 = res_t_bwd(dt, blk['xa'], Wt[n1], dy)
      dy = rnd_(dx)
      grads[n1 + '__w'], grads[n1 + '__b'] = dw1, db1
      trace += [('dt %d.%d' % (si, bi), dt), ('dx %d.%d' % (si, bi), dy)]
    head = rec['heads'][si]
    H, W = head['y'].shape[1], head['y'].shape[2]
    dY = rnd_(head_gather(dy, head['code'], H, W, head['pads'])[0])
    # the weight gradient is taken against x / 255 whatever form the forward
    # used (conv1_pool_bwd scales by 1 / 255 in fp32 at its flush)
    x = rec['x0'] if si == 0 else head['x']
    dx, _, dw, db = head_bwd(dY, x, Wt[st['head']], need_dx=si > 0)
    grads[st['head'] + '__w'], grads[st['head'] + '__b'] = dw, db
    if si > 0:
      dy = rnd_(dx)
      trace.append(('dx head %d' % si, dy))
  grads['_dy'] = trace
  return grads


def rel_l2(a, ref):
  a, ref = O.d64(a), O.d64(ref)
  return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


# -------------------------------------------------------------------- inputs

def make_agent(frame_shape, seed, round_weights=True):
  """Deep HIP bf16 agent with seed-fixed init, conv weights rounded in place
  to bf16-representable values (unless round_weights=False) and non-zero
  biases."""
  from scalable_agent_amd.models import Agent
  agent = Agent(9, torso='deep', frame_shape=frame_shape, seed=seed,
                backend='hip', compute_dtype=torch.bfloat16)
  g = torch.Generator().manual_seed(seed + 1000003)
  with torch.no_grad():
    for name, p in agent.convnet.items():
      if name.endswith('__w'):
        if round_weights:
          p.copy_(p.to(torch.bfloat16).float())
      else:
        p.copy_(torch.randn(p.shape, generator=g) * 0.1)
  return agent


def make_inputs(frame_shape, N, seed, flat):
  """(uint8 frames [N, H, W, C], bf16 feature gradient [N, flat])."""
  g = torch.Generator().manual_seed(seed + 77)
  frames = torch.randint(0, 256, (N,) + tuple(frame_shape), generator=g,
                         dtype=torch.uint8)
  grad = torch.randn(N, flat, generator=g).to(torch.bfloat16)
  return frames, grad
