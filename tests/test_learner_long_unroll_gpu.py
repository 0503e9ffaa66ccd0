"""The HIP learner's fused loss past the whole-column head kernel's limits.

compute_loss(use_fused=True) on a HIP-backend agent (shallow torso, fp32,
frames 72 x 96 x 3, B = 2) against the torch-backend agent of the same seed
on the same batch, with the tolerance of the fp32 learner parity tests
(tests/test_learner_parity_gpu.py: per-parameter gradient cosine >= 0.999999
and relative L2 error <= 1e-4, loss within 1e-4 max(|loss|, 1)):

  A = 31, T = learner_head_max_unroll(31) + 1   one step past the LDS bound
  A = 40, T = 8                                 more than 31 actions

Both must run the time-tiled head kernel (the op's launch counter).
"""

import pytest
import torch

from scalable_agent_amd import flags as flags_lib
from scalable_agent_amd.envs.synthetic import make_synthetic_batch
from scalable_agent_amd.learner import Learner, batch_to_device, compute_loss
from scalable_agent_amd.models import Agent

pytestmark = pytest.mark.gpu

_SHAPE = (72, 96, 3)


def _loss_and_grads(backend, A, T, batch, cuda):
  flags = flags_lib.default_flags(batch_size=2, unroll_length=T, torso='shallow')
  agent = Agent(A, torso='shallow', frame_shape=_SHAPE, seed=3, backend=backend,
                compute_dtype=torch.float32)
  lrn = Learner(agent, flags, cuda)
  lrn.flat.zero_grad()
  loss = compute_loss(agent, batch, flags, use_fused=backend == 'hip')
  loss.backward()
  torch.cuda.synchronize()
  return float(loss), lrn.flat.grads.clone(), lrn.flat


def _compare(A, T, cuda):
  from scalable_agent_amd import ops
  from scalable_agent_amd.ops import heads as heads_mod
  ops.load()
  batch = batch_to_device(make_synthetic_batch(2, T, _SHAPE, A, seed=2), cuda)
  ref_loss, ref_g, ref_flat = _loss_and_grads('torch', A, T, batch, cuda)
  before = dict(heads_mod.head_kernel_calls)
  hip_loss, hip_g, hip_flat = _loss_and_grads('hip', A, T, batch, cuda)
  after = heads_mod.head_kernel_calls
  assert after['tiled'] == before['tiled'] + 1
  assert after['untiled'] == before['untiled']
  print('loss hip %.6f torch %.6f' % (hip_loss, ref_loss))
  assert abs(hip_loss - ref_loss) <= 1e-4 * max(abs(ref_loss), 1.0)
  worst = []
  for name, _ in ref_flat.named:
    gr = ref_flat.view_of(ref_g, name).double()
    gh = hip_flat.view_of(hip_g, name).double()
    if gr.abs().max() == 0:
      assert gh.abs().max() == 0, name
      continue
    cos = torch.nn.functional.cosine_similarity(gr.reshape(1, -1),
                                                gh.reshape(1, -1)).item()
    rel = ((gh - gr).norm() / gr.norm()).item()
    print('%-40s rel %.3g  1 - cos %.3g' % (name, rel, 1.0 - cos))
    worst.append((rel, cos, name))
  for rel, cos, name in worst:
    assert cos >= 0.999999, (name, cos)
    assert rel <= 1e-4, (name, rel)


def test_unroll_past_the_head_lds_bound(cuda):
  from scalable_agent_amd import ops
  ops.load()
  A = 31
  _compare(A, ops.learner_head_max_unroll(A) + 1, cuda)


def test_forty_actions_stay_on_the_fused_path(cuda):
  _compare(40, 8, cuda)
