#!/usr/bin/env python3
"""Shallow learner step with --torso_dtype=auto against --torso_dtype=bf16
(bench.py cannot pass the flag).  One learner per form on the same device-
resident synthetic batch (no host-to-device prefetch: both forms skip it
alike), one captured graph each, `--rounds` interleaved rounds of `--steps`
replays after `--warmup`; prints one JSON line with every round's ms per step.

  python tools/shallow_torso_dtype_bench.py [--rounds 5 --steps 30 --warmup 10]
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scalable_agent_amd import flags as flags_lib  # noqa: E402
from scalable_agent_amd.envs.synthetic import make_synthetic_batch  # noqa: E402
from scalable_agent_amd.learner import FlatStaging, Learner  # noqa: E402
from scalable_agent_amd.models import Agent  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch_size', type=int, default=32)
  ap.add_argument('--unroll_length', type=int, default=100)
  ap.add_argument('--height', type=int, default=72)
  ap.add_argument('--width', type=int, default=96)
  ap.add_argument('--channels', type=int, default=3)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--steps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--graph', type=int, default=1)
  args = ap.parse_args()
  device = torch.device('cuda', 0)
  shape = (args.height, args.width, args.channels)
  batch = make_synthetic_batch(args.batch_size, args.unroll_length, shape, 9,
                               seed=1000, pin_memory=False)
  slot = FlatStaging(batch, device).load(batch).views
  runs = {}
  for form in ('auto', 'bf16'):
    flags = flags_lib.default_flags(
        batch_size=args.batch_size, unroll_length=args.unroll_length,
        torso='shallow', height=args.height, width=args.width,
        torso_dtype=form)
    agent = Agent(9, torso='shallow', frame_shape=shape, seed=flags.seed,
                  backend='hip', torso_dtype=form)
    learner = Learner(agent, flags, device)
    if args.graph:
      learner.capture(slot, clone=False)
      step = learner.graph_step
    else:
      step = lambda learner=learner: learner.step(slot)  # noqa: E731
    for _ in range(args.warmup):
      loss = step()
    torch.cuda.synchronize(device)
    assert bool(torch.isfinite(loss).item()), form
    runs[form] = (step, [])
  for _ in range(args.rounds):
    for form, (step, ms) in runs.items():
      torch.cuda.synchronize(device)
      t0 = time.perf_counter()
      for _ in range(args.steps):
        step()
      torch.cuda.synchronize(device)
      ms.append(round(1000 * (time.perf_counter() - t0) / args.steps, 4))
  print(json.dumps({'frame': shape, 'B': args.batch_size,
                    'T': args.unroll_length, 'graph': bool(args.graph),
                    'ms_per_step': {f: ms for f, (_, ms) in runs.items()}}))


if __name__ == '__main__':
  main()
