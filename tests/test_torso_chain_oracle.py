"""The float64 torso-chain oracle (tests/_torso_chain_oracle.py) against the
model definition: Agent(torso='deep', backend='torch',
compute_dtype=float64) under autograd.

The oracle's layer functions are chained with no rounding; the features and
every conv weight and bias gradient must equal the torch agent's to 1e-10
(max error relative to the tensor's largest magnitude).  That makes the
oracle's wiring - which activation masks which gradient, where the skip is
added, which parameter a gradient belongs to - the model's wiring; the GPU
test then holds the HIP chain to the oracle layer by layer.  No GPU.
"""

import pytest
import torch

from scalable_agent_amd.models import Agent
from tests import _torso_chain_oracle as T

TOL = 1e-10

# frame shape, images (the shapes of test_deep_torso_chain_gpu.py)
CASES = [((20, 26, 3), 3), ((21, 19, 4), 3), ((72, 96, 3), 2), ((84, 84, 4), 2)]


def _close(a, ref, what):
  err = float((a - ref).abs().max())
  scale = float(ref.abs().max())
  assert scale > 0, what
  assert err <= TOL * scale, '%s: max err %.3g vs scale %.3g' % (what, err, scale)


@pytest.mark.parametrize('frame_shape,N', CASES)
def test_chain_equals_torch_float64_agent(frame_shape, N):
  seed = 11
  agent = Agent(9, torso='deep', frame_shape=frame_shape, seed=seed,
                backend='torch', compute_dtype=torch.float64)
  g = torch.Generator().manual_seed(5)
  with torch.no_grad():
    for name, p in agent.convnet.items():
      if name.endswith('__b'):
        p.copy_(torch.randn(p.shape, generator=g) * 0.1)
  # float64 master copies too: autograd hands a gradient back in its
  # parameter's dtype, and fp32 would round it at 6e-8
  agent.double()
  frames, grad = T.make_inputs(frame_shape, N, seed, agent.flat_size)
  grad = grad.to(torch.float64)

  feats = agent.conv_features(frames)
  assert feats.dtype == torch.float64
  names = [n for n, _ in agent.convnet.named_parameters()]
  want = torch.autograd.grad(feats, [agent.convnet[n] for n in names], grad)

  rec = T.forward_chain(agent, frames)
  grads = T.backward_chain(rec, grad)
  assert rec['feats'].shape == feats.shape
  _close(rec['feats'], feats.detach(), 'features')
  # every conv parameter of the model has exactly one oracle gradient
  assert sorted(names) == sorted(k for k in grads if k != '_dy')
  for n, gw in zip(names, want):
    assert grads[n].shape == gw.shape, n
    _close(grads[n], gw.to(torch.float64), n)


def test_stage_table_follows_the_specs():
  agent = Agent(9, torso='deep', frame_shape=(20, 26, 3), seed=1)
  stages = T.stages_of(agent)
  assert [(s['cin'], s['cout'], len(s['blocks'])) for s in stages] == \
      [(3, 16, 2), (16, 32, 2), (32, 32, 2)]
  names = T.conv_names(agent)
  assert len(names) == 15 and len(set(names)) == 15
  assert {n + s for n in names for s in ('__w', '__b')} == set(agent.convnet.keys())


def test_kernel_weights_round_to_nearest_even():
  """The bf16 grid near 1 has spacing 2^-7: 1 + 2^-8 is a tie and goes to the
  even neighbour 1, 1 + 3 * 2^-8 to 1 + 2^-6 (truncation would give 1 and
  1 + 2^-7)."""
  agent = Agent(9, torso='deep', frame_shape=(20, 26, 3), seed=1)
  name = T.stages_of(agent)[1]['head']
  with torch.no_grad():
    w = agent.convnet[name + '__w']
    w.view(-1)[0] = 1.0 + 2.0 ** -8
    w.view(-1)[1] = 1.0 + 3 * 2.0 ** -8
  kw = T.kernel_weights(agent)[name].view(-1)
  assert float(kw[0]) == 1.0 and float(kw[1]) == 1.0 + 2.0 ** -6
  # the first layer folds 1 / 255 in before the one rounding
  head = T.stages_of(agent)[0]['head']
  w0 = agent.convnet[head + '__w'].detach()
  want = (w0 * torch.tensor(1 / 255.0)).to(torch.bfloat16).double()
  assert torch.equal(T.kernel_weights(agent)[head], want)
