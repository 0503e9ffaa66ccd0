"""The one-launch bf16 torso stages (stage_fwd_kernel: stage_bf16_fwd and
stage_tail_bf16_fwd) against the launches they replace.

The oracle is conv_pool_fwd followed by two res_block_fwd (covered by the
float64 tests of test_conv_gpu.py / test_conv_persistent_gpu.py).  Both paths
round to bf16 at the same points (the pooled map, t and y) and conv_tile_fwd
fixes every pixel's MFMA order whatever the tiling, so the requirement is
BITWISE equality: torch.equal, no tolerance.

Shapes: the smallest that reach each path - runtime-geometry inputs, odd maps
(odd pooled size, pad_before 1), every compiled geometry, one and several
images, and five images on two workgroups so a workgroup walks three.  The
weights are scaled so that about half of t is positive (asserted on the
oracle's t): a dead ReLU would hide conv2."""

import pytest
import torch

from scalable_agent_amd.models import layers

pytestmark = pytest.mark.gpu

# (H, W, CIN) of a stage's input (COUT = 32), compiled geometry or not
STAGES = [(12, 16, 16, False), (6, 8, 32, False), (10, 14, 16, False),
          (5, 7, 32, False), (36, 48, 16, True), (42, 42, 16, True),
          (18, 24, 32, True), (21, 21, 32, True), (18, 32, 32, True)]
# (H, W) of a pooled 16-channel map
TAILS = [(12, 16, False), (36, 48, True), (42, 42, True)]


def _C():
  from scalable_agent_amd import ops
  return ops.ext()


def _seed(*key):
  return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def _conv(g, cin, cout, cuda):
  w = torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5
  b = torch.randn(cout, generator=g) * 0.1
  return w.to(cuda), b.to(cuda)


def _blocks(g, c, cuda):
  out = []
  for _ in range(4):
    out += list(_conv(g, c, c, cuda))
  return out


def _pads(h, w):
  return layers.same_pads(h, 3, 2)[0], layers.same_pads(w, 3, 2)[0]


def _oracle_blocks(C, p, blocks, last):
  t1, y1 = C.res_block_fwd(p, *blocks[:4], False)
  t2, y2 = C.res_block_fwd(y1, *blocks[4:], last)
  for name, t in (('t1', t1), ('t2', t2)):
    zeros = (t == 0).float().mean().item()
    print('%s zeros: %.3f' % (name, zeros))
    assert 0.2 <= zeros <= 0.8, (name, zeros)
  return y2


def _check_record(C, n, cap, compiled):
  rec = C.conv_launch_info('')
  assert rec['family'] == 'stage_bf16', rec
  assert rec == C.conv_launch_info('stage_bf16')
  assert rec['ntiles'] == n and rec['grid'] == min(n, cap), rec
  assert rec['specialized'] == compiled, rec


def _run_stage(C, cuda, H, W, cin, n, last, compiled, cap=None):
  g = torch.Generator().manual_seed(_seed(1, H, W, cin, n, last))
  x = torch.randn(n, H, W, cin, generator=g).to(torch.bfloat16).to(cuda)
  w, b = _conv(g, cin, 32, cuda)
  blocks = _blocks(g, 32, cuda)
  pb_h, pb_w = _pads(H, W)
  assert (pb_h, pb_w) == (H % 2, W % 2)
  p = C.conv_pool_fwd(x, w, b, pb_h, pb_w)[0]
  want = _oracle_blocks(C, p, blocks, last)
  assert C.stage_bf16_form(n, H, W, cin, 32) == 1
  got = C.stage_bf16_fwd(x, w, b, *blocks, pb_h, pb_w, last)
  _check_record(C, n, cap or C.conv_launch_info('stage_bf16')['grid_max'], compiled)
  assert got.shape == want.shape == (n, (H + 1) // 2, (W + 1) // 2, 32)
  assert got.dtype == torch.bfloat16
  assert (want < 0).any().item() != last
  assert torch.equal(got, want)


def _run_tail(C, cuda, H, W, n, last, compiled, cap=None):
  g = torch.Generator().manual_seed(_seed(2, H, W, n, last))
  x = (torch.randn(n, H, W, 16, generator=g) + 0.5).to(torch.bfloat16).to(cuda)
  blocks = _blocks(g, 16, cuda)
  want = _oracle_blocks(C, x, blocks, last)
  assert C.stage_bf16_form(n, H, W, 16, 16) == 2
  got = C.stage_tail_bf16_fwd(x, *blocks, last)
  _check_record(C, n, cap or C.conv_launch_info('stage_bf16')['grid_max'], compiled)
  assert got.shape == x.shape and got.dtype == torch.bfloat16
  assert (want < 0).any().item() != last
  assert torch.equal(got, want)


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('H,W,cin,compiled', STAGES)
def test_stage_is_bitwise_the_launches(cuda, H, W, cin, compiled, n, last):
  _run_stage(_C(), cuda, H, W, cin, n, last, compiled)


@pytest.mark.parametrize('last', [False, True])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('H,W,compiled', TAILS)
def test_tail_is_bitwise_the_launches(cuda, H, W, compiled, n, last):
  _run_tail(_C(), cuda, H, W, n, last, compiled)


def test_a_workgroup_walks_several_images(cuda):
  """Five images on two workgroups (conv_tune('stage_bf16_grid', 2))."""
  C = _C()
  old = C.conv_tune('stage_bf16_grid', 2)
  try:
    assert C.conv_tune('stage_bf16_grid') == 2
    _run_stage(C, cuda, 12, 16, 16, 5, True, False, cap=2)
    _run_stage(C, cuda, 18, 24, 32, 5, False, True, cap=2)
    _run_tail(C, cuda, 36, 48, 5, False, True, cap=2)
  finally:
    C.conv_tune('stage_bf16_grid', old)
  assert C.conv_tune('stage_bf16_grid') == old == 0


def test_runtime_geometry_kernel_equals_the_compiled_one(cuda):
  C = _C()
  old = C.conv_tune('specialize', 0)
  try:
    _run_stage(C, cuda, 18, 24, 32, 3, True, False)
    _run_tail(C, cuda, 36, 48, 3, False, False)
  finally:
    C.conv_tune('specialize', old)


def test_bindings_decline_and_raise(cuda):
  C = _C()
  assert C.stage_bf16_form(3, 36, 64, 16, 16) == 0  # two maps exceed the LDS
  assert C.stage_bf16_form(0, 36, 48, 16, 16) == 0
  assert C.stage_bf16_form(513, 36, 48, 16, 16) == 0
  assert C.stage_bf16_form(0, 36, 48, 16, 32) == 0
  assert C.stage_bf16_form(513, 18, 24, 32, 32) == 0
  assert C.stage_bf16_form(512, 36, 48, 16, 16) == 2
  g = torch.Generator().manual_seed(3)
  b16, b32 = _blocks(g, 16, cuda), _blocks(g, 32, cuda)
  w, b = _conv(g, 16, 32, cuda)
  bf = dict(device=cuda, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match='no one-launch form'):
    C.stage_tail_bf16_fwd(torch.zeros(3, 36, 64, 16, **bf), *b16, False)
  with pytest.raises(RuntimeError, match='no one-launch form'):
    C.stage_tail_bf16_fwd(torch.zeros(0, 36, 48, 16, **bf), *b16, False)
  with pytest.raises(RuntimeError, match='no one-launch form'):
    C.stage_tail_bf16_fwd(torch.zeros(513, 12, 16, 16, **bf), *b16, False)
  with pytest.raises(RuntimeError, match='no one-launch form'):
    C.stage_bf16_fwd(torch.zeros(513, 6, 8, 16, **bf), w, b, *b32, 0, 0, False)
  with pytest.raises(RuntimeError, match='bfloat16'):
    C.stage_tail_bf16_fwd(torch.zeros(3, 12, 16, 16, device=cuda), *b16, False)
  with pytest.raises(RuntimeError, match='bfloat16'):
    C.stage_bf16_fwd(torch.zeros(3, 12, 16, 16, device=cuda), w, b, *b32, 0, 0,
                     False)
  with pytest.raises(RuntimeError):  # block weights of the wrong width
    C.stage_bf16_fwd(torch.zeros(3, 12, 16, 16, **bf), w, b, *b16, 0, 0, False)
  with pytest.raises(RuntimeError):  # an odd width needs pad_before 1
    C.stage_bf16_fwd(torch.zeros(3, 10, 15, 16, **bf), w, b, *b32, 0, 0, False)
  torch.cuda.synchronize()
