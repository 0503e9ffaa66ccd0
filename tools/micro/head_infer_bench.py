#!/usr/bin/env python3
"""The one-launch inference stage heads (cf32_head_fwd) against the launches
they replace, at actor-inference batches.

  stage 0: cf32_frames_f32 + cf32_wino_conv_pool_fwd (conv + pool, fix-up)
  stage 1: cf32_wino_conv_pool_fwd (conv + pool, fix-up; the 42-wide map runs
           cf32_conv_fwd + cf32_maxpool_fwd, as the torso does)

Each form is captured in a graph of REPS back-to-back repetitions (allocator
and launch overhead out of the picture), the two graphs are replayed
alternately for ROUNDS rounds in one process, and the median and the minimum
per repetition are printed.  The inputs stay the same across repetitions, so
they are cache-resident, as a board's freshly copied frames are.
Usage: python tools/micro/head_infer_bench.py [rounds] [reps]
"""
import statistics
import sys

import torch

sys.path.insert(0, '.')
from scalable_agent_amd import ops  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
C = ops.ext()
dev = torch.device('cuda')


def graph_of(fn):
  side = torch.cuda.Stream(dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side), torch.no_grad():
    fn()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
      for _ in range(REPS):
        out = fn()
  torch.cuda.current_stream(dev).wait_stream(side)
  return g, out


def replay_us(g):
  s, e = torch.cuda.Event(True), torch.cuda.Event(True)
  s.record()
  g.replay()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) / REPS * 1e3


def compare(name, old, new):
  g_old, y_old = graph_of(old)
  g_new, y_new = graph_of(new)
  for g in (g_old, g_new):
    g.replay()
  torch.cuda.synchronize()
  assert torch.equal(y_old, y_new), name
  t_old, t_new = [], []
  for _ in range(ROUNDS):
    t_old.append(replay_us(g_old))
    t_new.append(replay_us(g_new))
  print('%-34s replaced launches %6.1f us (min %6.1f) | head %6.1f us (min %6.1f)' % (
      name, statistics.median(t_old), min(t_old), statistics.median(t_new),
      min(t_new)), flush=True)


for N in (76, 150):
  for H, W, c in [(72, 96, 3), (84, 84, 4), (72, 128, 3)]:
    frames = torch.randint(0, 256, (N, H, W, c), dtype=torch.uint8, device=dev)
    w0 = torch.randn(3, 3, c, 16, device=dev) * 0.1
    w0p = torch.cat([w0, torch.zeros(3, 3, 4 - c, 16, device=dev)], 2) if c < 4 else w0
    b0 = torch.randn(16, device=dev)
    old0 = lambda: C.cf32_wino_conv_pool_fwd(C.cf32_frames_f32(frames), w0p, b0)[0]
    new0 = lambda: C.cf32_head_fwd(frames, w0p, b0)[0]
    compare('N=%-3d stage 0 %dx%dx%d (band %d)' % (N, H, W, c, C.cf32_head_band(H, W, c)),
            old0, new0)
    h, w_ = H // 2, W // 2
    x = torch.randn(N, h, w_, 16, device=dev)
    w1 = torch.randn(3, 3, 16, 32, device=dev) * 0.1
    b1 = torch.randn(32, device=dev)

    def old1():
      out = C.cf32_wino_conv_pool_fwd(x, w1, b1)
      if out:
        return out[0]
      return C.cf32_maxpool_fwd(C.cf32_conv_fwd(x, w1, b1, 1, 1, 1, h, w_), 0, 0)[0]

    new1 = lambda: C.cf32_head_fwd(x, w1, b1)[0]
    compare('N=%-3d stage 1 %dx%dx16 (band %d)' % (N, h, w_, C.cf32_head_band(h, w_, 16)),
            old1, new1)
