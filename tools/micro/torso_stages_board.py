#!/usr/bin/env python3
"""Model step of a bf16 deep inference board launch with --torso_stages=ops
and fused (the method of profiles/shallow_bf16_board.txt): per arm 10 warm-up
steps, 100 timed eager steps (wall), then 30 steps under torch.profiler.
Prints kernels per step, kernel time per step, the summed time of the conv
torso's kernels and each kernel's mean duration.

usage: torso_stages_board.py [--rows 76,150] [--frames 72x96x3,84x84x4]
                             [--stages ops,fused] [--tag this]
An extension without the stage kernel (SA_EXT_PATH=<the parent's build>) runs
the ops arm only: pass --stages ops."""

import argparse
import collections
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))

from scalable_agent_amd import inference  # noqa: E402
from scalable_agent_amd.models import Agent  # noqa: E402

TORSO = ('conv1_pool_fwd', 'conv_pool_fwd', 'res_block_fwd', 'res_conv_fwd',
         'stage_fwd')


def arm(tag, rows, shape, stages, core):
  dev = torch.device('cuda', 0)
  agent = Agent(9, torso='deep', frame_shape=shape, seed=1, backend='hip',
                compute_dtype=torch.bfloat16, torso_stages=stages,
                actor_core=core)
  model = inference.InferenceModel(agent, dev, use_instruction=False, seed=3)
  g = torch.Generator().manual_seed(4)
  ins = [torch.randint(0, 9, (rows,), generator=g),
         torch.randn(rows, generator=g), torch.zeros(rows, dtype=torch.bool),
         torch.randint(0, 256, (rows,) + shape, generator=g, dtype=torch.uint8),
         torch.zeros(rows, 16, dtype=torch.int64),
         torch.zeros(rows, dtype=torch.int64),
         torch.randn(rows, 256, generator=g), torch.randn(rows, 256, generator=g)]
  ins = [t.to(dev) for t in ins]

  def steps(n):
    with model._lock, torch.cuda.stream(model.stream):
      for _ in range(n):
        model.step_device(*ins, has_instr=False)
      model.stream.synchronize()

  steps(10)
  t0 = time.perf_counter()
  steps(100)
  wall = (time.perf_counter() - t0) / 100 * 1e6
  n = 30
  with torch.profiler.profile(
      activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
    steps(n)
  dur = collections.defaultdict(float)
  cnt = collections.Counter()
  for ev in prof.events():
    if ev.device_type == torch.autograd.DeviceType.CUDA:
      dur[ev.name] += ev.self_device_time_total
      cnt[ev.name] += 1
  total = sum(dur.values()) / n
  torso = sum(v for k, v in dur.items() if any(t in k for t in TORSO)) / n
  ntorso = sum(v for k, v in cnt.items() if any(t in k for t in TORSO)) / n
  print('%s rows=%d frame=%s actor_core=%s torso_stages=%s(%s): %.1f kernels/step, '
        '%.1f us kernel time/step, torso %.1f kernels %.1f us, %.1f us eager '
        'wall/step' % (tag, rows, 'x'.join(map(str, shape)), core, stages,
                       model.torso_stages, sum(cnt.values()) / n, total, ntorso,
                       torso, wall), flush=True)
  for k in sorted(dur, key=lambda k: -dur[k]):
    print('    %7.2f us x %4.1f/step  %s' % (dur[k] / cnt[k], cnt[k] / n, k[:110]),
          flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rows', default='76,150')
  ap.add_argument('--frames', default='72x96x3,84x84x4')
  ap.add_argument('--stages', default='ops,fused')
  ap.add_argument('--actor_core', default='ops')
  ap.add_argument('--tag', default='this')
  args = ap.parse_args()
  for frame in args.frames.split(','):
    shape = tuple(int(d) for d in frame.split('x'))
    for rows in args.rows.split(','):
      for stages in args.stages.split(','):
        arm(args.tag, int(rows), shape, stages, args.actor_core)


if __name__ == '__main__':
  main()
