#!/usr/bin/env python3
"""Per-layer timing of the exact-fp32 conv kernels at learner-batch size.

Deep-ResNet layers at N = (T+1) * B = 3232 frames (72x96x3 input): forward,
data gradient and weight gradient of every distinct layer shape, with the
achieved TFLOP/s against the 157 TF fp32 MFMA peak.  Usage:
  python tools/conv_f32_bench.py [N] [reps]
"""
import sys
import torch

sys.path.insert(0, '.')
from scalable_agent_amd import ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 3232
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ONLY = sys.argv[3] if len(sys.argv) > 3 else ''  # substring filter on layer names
C = ops.ext()
dev = torch.device('cuda')
# name, H, W, Cin, Cout, K, S, pt, pl, uint8 source, relu_in, resid
LAYERS = [
    ('deep conv1 3->16 72x96', 72, 96, 3, 16, 3, 1, 1, 1, True),
    ('deep res16 36x48', 36, 48, 16, 16, 3, 1, 1, 1, False),
    ('deep conv2 16->32 36x48', 36, 48, 16, 32, 3, 1, 1, 1, False),
    ('deep res32 18x24', 18, 24, 32, 32, 3, 1, 1, 1, False),
    ('deep res32 9x12', 9, 12, 32, 32, 3, 1, 1, 1, False),
    ('shallow1 8x8/4', 72, 96, 3, 32, 8, 4, 2, 2, True),
    ('shallow2 4x4/2', 18, 24, 32, 64, 4, 2, 1, 1, False),
    ('shallow3 3x3/2', 9, 12, 64, 128, 3, 2, 1, 0, False),
]


def timeit(fn):
  fn()
  torch.cuda.synchronize()
  s, e = torch.cuda.Event(True), torch.cuda.Event(True)
  s.record()
  for _ in range(REPS):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) / REPS * 1e3


for name, H, W, Ci, Co, K, S, pt, pl, u8 in LAYERS:
  if ONLY and ONLY not in name:
    continue
  Ho, Wo = -(-H // S), -(-W // S)
  x = (torch.randint(0, 256, (N, H, W, Ci), dtype=torch.uint8, device=dev) if u8
       else torch.randn(N, H, W, Ci, device=dev))
  w = torch.randn(K, K, Ci, Co, device=dev) * 0.1
  b = torch.randn(Co, device=dev)
  dy = torch.randn(N, Ho, Wo, Co, device=dev)
  dw = torch.zeros_like(w)
  db = torch.zeros_like(b)
  flop = 2.0 * N * Ho * Wo * K * K * Ci * Co
  tf = timeit(lambda: C.cf32_conv_fwd(x, w, b, S, pt, pl, Ho, Wo))
  tw = timeit(lambda: C.cf32_conv_wgrad(x, dy, S, pt, pl, False, dw, db))
  line = '%-26s fwd %8.1f us %6.1f TF | wgrad %8.1f us %6.1f TF' % (
      name, tf, flop / tf / 1e6, tw, flop / tw / 1e6)
  if not u8:
    td = timeit(lambda: C.cf32_conv_dgrad(dy, w, S, pt, pl, H, W))
    line += ' | dgrad %8.1f us %6.1f TF' % (td, flop / td / 1e6)
  print(line, flush=True)
# residual-conv backward: fused (one pass) vs separate wgrad + masked dgrad
# (stage heads: 16 -> 32 and 32 -> 32 without mask / skip, relu_x off)
for name, H, W, Cc, Cy, res in [('res16 36x48', 36, 48, 16, 16, True),
                                ('res32 18x24', 18, 24, 32, 32, True),
                                ('res32 9x12', 9, 12, 32, 32, True),
                                ('head conv2 16->32 36x48', 36, 48, 16, 32, False),
                                ('head conv3 32->32 18x24', 18, 24, 32, 32, False)]:
  if ONLY and ONLY not in name and ONLY not in ('bwd', 'deep'):
    continue
  x = torch.randn(N, H, W, Cc, device=dev)
  w = torch.randn(3, 3, Cc, Cy, device=dev) * 0.1
  dy = torch.randn(N, H, W, Cy, device=dev)
  add = torch.randn(N, H, W, Cc, device=dev) if res else None
  dw = torch.zeros_like(w)
  db = torch.zeros(Cy, device=dev)
  tf = timeit(lambda: C.cf32_conv_bwd_fused(dy, w, x, res, dw, db, add=add, mask=res))

  def sep():
    C.cf32_conv_wgrad(x, dy, 1, 1, 1, res, dw, db)
    C.cf32_conv_dgrad(dy, w, 1, 1, 1, H, W, mask=x if res else None, add=add)
  ts = timeit(sep)
  bflop = 2 * 2.0 * N * H * W * 9 * Cc * Cy  # dgrad + wgrad, direct-conv FLOPs
  print('%-26s bwd fused %8.1f us %6.1f TF | separate wgrad+dgrad %8.1f us %6.1f TF' % (
      name, tf, bflop / tf / 1e6, ts, bflop / ts / 1e6), flush=True)
# stage-1 head forward: conv + maxpool_fwd vs the pool fused into the
# Winograd epilogue (wino_conv_pool_kernel)
if not ONLY or ONLY in 'head conv2 pool deep':
  x = torch.randn(N, 36, 48, 16, device=dev)
  w = torch.randn(3, 3, 16, 32, device=dev) * 0.1
  b = torch.randn(32, device=dev)
  tc = timeit(lambda: C.cf32_maxpool_fwd(C.cf32_conv_fwd(x, w, b, 1, 1, 1, 36, 48), 0, 0))
  tfp = timeit(lambda: C.cf32_wino_conv_pool_fwd(x, w, b))
  flop = 2.0 * N * 36 * 48 * 9 * 16 * 32
  print('%-26s fwd+pool: conv + maxpool %8.1f us | fused %8.1f us %6.1f TF' % (
      'head conv2 16->32 36x48', tc, tfp, flop / tfp / 1e6), flush=True)


def timeit_graph(fn, inner=20):
  """us per call of fn inside a captured graph of `inner` back-to-back calls
  (actor inference replays graphs: no host launch cost between kernels)."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
      for _ in range(inner):
        fn()
    g.replay()
    side.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record(side)
    for _ in range(REPS):
      g.replay()
    e.record(side)
    side.synchronize()
  return s.elapsed_time(e) / (REPS * inner) * 1e3


# residual block forward at an actor-inference batch (N <= 512, e.g. 76 or
# 150): the two Winograd convs vs the one-launch block (wino_res_block_kernel),
# eager and inside a captured graph
if (not ONLY or ONLY in 'block') and N <= 512:
  for name, H, W, Cc in [('res16 36x48', 36, 48, 16), ('res32 18x24', 18, 24, 32),
                         ('res32 9x12', 9, 12, 32)]:
    x = torch.randn(N, H, W, Cc, device=dev)
    w1 = torch.randn(3, 3, Cc, Cc, device=dev) * 0.1
    w2 = torch.randn(3, 3, Cc, Cc, device=dev) * 0.1
    b1 = torch.randn(Cc, device=dev)
    b2 = torch.randn(Cc, device=dev)
    conv1 = lambda: C.cf32_conv_fwd(x, w1, b1, 1, 1, 1, H, W, relu_in=True, relu_out=True)
    t = conv1()
    conv2 = lambda: C.cf32_conv_fwd(t, w2, b2, 1, 1, 1, H, W, add=x)
    block = lambda: C.cf32_res_block_fwd(x, w1, b1, w2, b2, False)
    assert block(), 'the fused block declined %s' % name
    for label, tm in (('eager', timeit), ('graph', timeit_graph)):
      t1, t2, tb = tm(conv1), tm(conv2), tm(block)
      print('%-14s N=%-4d %s block fwd: conv1 %6.1f + conv2 %6.1f = %6.1f us | fused '
            '%6.1f us (band %d rows)' % (name, N, label, t1, t2, t1 + t2, tb,
                                        C.cf32_res_block_band(Cc, W)), flush=True)
# the whole last stage at an actor-inference batch in the three forms of
# --torso_blocks: ops (head + 4 convs), fused (head + 2 block launches), stage
# (one launch where cf32_stage_fwd takes the input, else head + one launch
# for both blocks); filter 'stage'
if (not ONLY or ONLY in 'stage') and N <= 512:
  for name, H, W in [('18x24 -> 9x12', 18, 24), ('21x21 -> 11x11', 21, 21),
                     ('18x32 -> 9x16', 18, 32)]:
    h, w_ = (H + 1) // 2, (W + 1) // 2
    x = torch.randn(N, H, W, 32, device=dev)
    wh = torch.randn(3, 3, 32, 32, device=dev) * 0.1
    bh = torch.randn(32, device=dev)
    tail = []
    for _ in range(4):
      tail += [torch.randn(3, 3, 32, 32, device=dev) * 0.1, torch.randn(32, device=dev)]

    def head():
      out = C.cf32_wino_conv_pool_fwd(x, wh, bh)
      if out:
        return out[0]
      pb = (0 if H % 2 == 0 else 1, 0 if W % 2 == 0 else 1)
      return C.cf32_maxpool_fwd(C.cf32_conv_fwd(x, wh, bh, 1, 1, 1, H, W), *pb)[0]

    def f_ops():
      xa = head()
      for k in range(2):
        w1, b1, w2, b2 = tail[4 * k:4 * k + 4]
        t = C.cf32_conv_fwd(xa, w1, b1, 1, 1, 1, h, w_, relu_in=True, relu_out=True)
        xa = C.cf32_conv_fwd(t, w2, b2, 1, 1, 1, h, w_, add=xa, relu_out=k == 1)
      return xa

    def f_fused():
      xa = head()
      for k in range(2):
        xa = C.cf32_res_block_fwd(xa, *tail[4 * k:4 * k + 4], k == 1)[0]
      return xa

    def f_stage():
      out = C.cf32_stage_fwd(x, wh, bh, *tail, True)
      return out[0] if out else C.cf32_stage_tail_fwd(head(), *tail, True)[0]

    form = {2: 'one launch', 1: 'head + one launch', 0: 'declined'}[
        C.cf32_stage_form(N, H, W, 32)]
    assert form != 'declined' and torch.equal(f_stage(), f_ops()), name
    for label, tm in (('eager', timeit), ('graph', timeit_graph)):
      print('last stage %-15s N=%-4d %s: ops %6.1f us | fused %6.1f us | stage %6.1f us (%s)' % (
          name, N, label, tm(f_ops), tm(f_fused), tm(f_stage), form), flush=True)
if ONLY:
  sys.exit(0)
xp =torch.randn(N, 72, 96, 16, device=dev)
tp = timeit(lambda: C.cf32_maxpool_fwd(xp, 0, 0))
y, arg = C.cf32_maxpool_fwd(xp, 0, 0)
tb = timeit(lambda: C.cf32_maxpool_bwd(y, arg, 72, 96, 0, 0))
print('maxpool 72x96x16 fwd %.1f us bwd %.1f us' % (tp, tb))
