#!/usr/bin/env python3
"""Times the 12 fp32 inference Winograd instances (conv_wino_infer.hip) at 76
rows of the three frame ladders.  Each binding is captured in a graph of REPS
back-to-back launches and replayed ROUNDS times; prints one JSON line with the
median / min us per launch and a checksum of each output's bits.  To compare
two builds, run it once per build (SA_EXT_PATH names another extension),
alternating.  Usage: python tools/micro/infer_wino_bench.py [label]"""
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
from scalable_agent_amd import ops  # noqa: E402

ROUNDS, REPS, N = 15, 20, 76
C = ops.ext()
dev = torch.device('cuda')
torch.manual_seed(0)


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


def wb(ci, co):
  return torch.randn(3, 3, ci, co, device=dev) * 0.1, torch.randn(co, device=dev)


cases = []
for H, W, c in [(72, 96, 3), (84, 84, 4), (72, 128, 3)]:
  tag = '%dx%dx%d' % (H, W, c)
  frames = torch.randint(0, 256, (N, H, W, c), dtype=torch.uint8, device=dev)
  w0, b0 = wb(c, 16)
  cases.append(('head0 ' + tag, lambda f=frames, w=w0, b=b0: C.cf32_head_fwd(f, w, b)))
  h1, w1_ = H // 2, W // 2
  x16 = torch.randn(N, h1, w1_, 16, device=dev)
  (wa, ba), (wc, bc) = wb(16, 16), wb(16, 16)
  cases.append(('res16 ' + tag, lambda x=x16, a=wa, b=ba, c_=wc, d=bc:
                C.cf32_res_block_fwd(x, a, b, c_, d, False)))
  wh1, bh1 = wb(16, 32)
  cases.append(('head1 ' + tag, lambda x=x16, w=wh1, b=bh1: C.cf32_head_fwd(x, w, b)))
  h2, w2_ = h1 // 2, w1_ // 2
  x32 = torch.randn(N, h2, w2_, 32, device=dev)
  ws = [wb(32, 32) for _ in range(5)]
  cases.append(('res32 ' + tag, lambda x=x32, s=ws:
                C.cf32_res_block_fwd(x, s[0][0], s[0][1], s[1][0], s[1][1], True)))
  flat = [t for p in ws[1:] for t in p]
  if C.cf32_stage_form(N, h2, w2_, 32) == 2:
    cases.append(('stage+head ' + tag, lambda x=x32, s=ws, f=flat:
                  C.cf32_stage_fwd(x, s[0][0], s[0][1], *f, True)))
  h3, w3_ = (h2 + 1) // 2, (w2_ + 1) // 2
  x3 = torch.randn(N, h3, w3_, 32, device=dev)
  cases.append(('stage_tail ' + tag, lambda x=x3, f=flat: C.cf32_stage_tail_fwd(x, *f, True)))

res = {}
for name, fn in cases:
  out = fn()
  assert out, name + ': declined'
  g, y = graph_of(lambda: fn()[0])
  for _ in range(3):
    g.replay()
  torch.cuda.synchronize()
  ts = [replay_us(g) for _ in range(ROUNDS)]
  res[name] = {'med_us': round(statistics.median(ts), 2), 'min_us': round(min(ts), 2),
               'bits': int(y.contiguous().view(torch.int32).to(torch.int64).sum().item())}
print(json.dumps({'label': sys.argv[1] if len(sys.argv) > 1 else '', 'results': res}), flush=True)
