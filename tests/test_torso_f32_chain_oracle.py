"""The float64 chain oracle of the fp32 torsos (tests/_torso_f32_chain_oracle.py)
against the model definition, and the conditions the GPU test
(test_torso_f32_chain_gpu.py) relies on, from float64 alone.  No GPU.

  * both torsos at every GPU case shape: the oracle's features and every conv
    weight and bias gradient equal Agent(backend='torch',
    compute_dtype=float64).conv_features under torch.autograd (assert_close,
    1e-10 of the tensor's largest magnitude);
  * per deep head, at most 1 % of the pool windows are left out of the
    argmax comparison by _conv_f32_oracle.argmax_clear;
  * no dead or saturated ReLU: between 20 % and 80 % of every deep t and of
    every shallow activation is zero, every non-final deep y has negative
    entries, the final output has zeros and positives.

The conditions on the recorded calls (relu_out on the final conv only, add= on
the second conv of each block and on the first conv's backward) need the
calls: the GPU test asserts them.  The seeds are the first tried; none had to
be skipped.
"""

import pytest
import torch

from scalable_agent_amd.models import Agent
from tests import _conv_oracle as O
from tests import _torso_chain_oracle as T
from tests import _torso_f32_chain_oracle as TF

TOL = 1e-10

CASES = ([('deep',) + c for c in TF.DEEP_CASES] +
         [('shallow',) + c for c in TF.SHALLOW_CASES])


def _close(a, ref, what):
  scale = float(ref.abs().max())
  assert scale > 0, what
  torch.testing.assert_close(a, ref, rtol=0, atol=TOL * scale, msg=lambda m: what + ': ' + m)


@pytest.mark.parametrize('torso,frame_shape,N,seed', CASES)
def test_chain_equals_torch_float64_agent(torso, frame_shape, N, seed):
  src, frames, g = TF.case(torso, frame_shape, N, seed)
  agent = Agent(9, torso=torso, frame_shape=frame_shape, seed=seed,
                backend='torch', compute_dtype=torch.float64)
  agent.convnet.load_state_dict(src.convnet.state_dict())
  # float64 master copies too: autograd hands a gradient back in its
  # parameter's dtype, and fp32 would round it at 6e-8
  agent.double()
  g = g.to(torch.float64)
  feats = agent.conv_features(frames)
  assert feats.dtype == torch.float64
  names = [n for n, _ in agent.convnet.named_parameters()]
  want = torch.autograd.grad(feats, [agent.convnet[n] for n in names], g)
  if torso == 'deep':
    rec = T.forward_chain(agent, frames)
    grads = T.backward_chain(rec, g)
    grads.pop('_dy')
  else:
    rec = TF.shallow_forward_chain(agent, frames)
    grads = TF.shallow_backward_chain(rec, g)
  assert torch.equal(rec['x0'] if torso == 'deep' else rec['acts'][0],
                     frames.double() / 255)
  assert rec['feats'].shape == feats.shape
  _close(rec['feats'], feats.detach(), 'features')
  assert sorted(names) == sorted(grads)
  for n, gw in zip(names, want):
    assert grads[n].shape == gw.shape, n
    _close(grads[n], gw, n)


@pytest.mark.parametrize('frame_shape,N,seed', TF.DEEP_CASES)
def test_deep_conditions(frame_shape, N, seed):
  agent, frames, _ = TF.case('deep', frame_shape, N, seed)
  rec = T.forward_chain(agent, frames)
  stages, P = rec['stages'], rec['P']
  for s, st in enumerate(stages):
    head = rec['heads'][s]
    w, b = P[st['head']]
    B = TF.conv_bound(head['x'], w, b)
    _, _, _, clear = TF.pool_check_terms(head['y'], B, head['pads'])
    left_out = 1.0 - float(clear.double().mean())
    print('F32CHAIN %s stage %d windows left out %.5f' % (frame_shape, s, left_out))
    assert left_out <= 0.01, (s, left_out)
    for bi, blk in enumerate(rec['blocks'][s]):
      final = s == len(stages) - 1 and bi == len(st['blocks']) - 1
      zeros = float((blk['t'] == 0).double().mean())
      assert 0.2 <= zeros <= 0.8, (s, bi, zeros)
      if not final:
        assert bool((blk['y'] < 0).any()), (s, bi)
  assert bool((rec['pre'] < 0).any())
  assert bool((rec['out'] == 0).any()) and bool((rec['out'] > 0).any())


@pytest.mark.parametrize('frame_shape,N,seed', TF.SHALLOW_CASES)
def test_shallow_conditions(frame_shape, N, seed):
  agent, frames, _ = TF.case('shallow', frame_shape, N, seed)
  rec = TF.shallow_forward_chain(agent, frames)
  for i, a in enumerate(rec['acts'][1:]):
    zeros = float((a == 0).double().mean())
    print('F32CHAIN %s layer %d zeros %.3f' % (frame_shape, i, zeros))
    assert 0.2 <= zeros <= 0.8, (i, zeros)
  assert bool((rec['out'] == 0).any()) and bool((rec['out'] > 0).any())


def test_tables_follow_the_specs():
  agent, _, _ = TF.case('shallow', *TF.SHALLOW_CASES[0])
  names = [n for n, _, _ in TF.shallow_layers(agent)]
  assert {n + s for n in names for s in ('__w', '__b')} == set(agent.convnet.keys())
  # the asymmetric pad of the 3x3 / 2 conv over a 12-wide map
  from tests import _conv_f32_oracle as F32
  assert F32.same_pads(12, 3, 2) == (0, 1) and F32.same_pads(11, 3, 2) == (1, 1)


def test_pool_gather_f32_is_the_float64_gather_in_fp32():
  """Integer gradients: no addition rounds, the ordered fp32 sums equal the
  float64 scatter; pad-before 0 and 1."""
  g = torch.Generator().manual_seed(1)
  for H, W in ((6, 8), (7, 5)):
    y = torch.randint(-3, 4, (2, H, W, 4), generator=g).double()
    pads = (O.pool_pb(H), O.pool_pb(W))
    _, code = O.pool64(y, *pads)
    dP = torch.randint(-3, 4, tuple(code.shape), generator=g).float()
    got = TF.pool_gather_f32(dP, code, H, W, pads)
    assert torch.equal(got.double(), O.scatter64(dP, code, H, W, *pads))
