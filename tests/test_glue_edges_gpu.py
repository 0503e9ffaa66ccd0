"""colsum_f32_ and relu_mask_bf16_ (csrc/kernels/learner_io.hip) at their
edges: the learner's live glue (the b_lstm gradient in ops/core.py, the
torso's final ReLU backward in ops/conv.py).

colsum_f32_(x, out): out[c] += sum_r x[r, c].  colsum_f32_kernel gives every
64-row chunk (blockIdx.y) and 256-column block (blockIdx.x) one slot of
partial sums, loading 16 rows at a time with rows past N read as 0;
rows_reduce_kernel adds the S = ceil(N / 64) slots of a column in four
interleaved chains (slots 4j, 4j+1, 4j+2, 4j+3, the S % 4 tail slots on the
first chain), joins them as (a0 + a1) + (a2 + a3) and adds that into out.

  * integer inputs: every partial and total is an integer below 2^24, exact
    in fp32 in any order, so the result is compared with torch.equal against
    the float64 sum; x is a contiguous row range of a NaN-filled buffer, so a
    read outside its N rows turns a column into NaN, a dropped row or column
    block changes an integer; N = 1 .. 512 gives S = 1, 2, 3, 5, 8 slots (the
    unrolled loop not entered, its tail alone, one round, one round + tail,
    two rounds) and row counts on both sides of the 16-row batch and the
    64-row chunk; C = 1 .. 1024 gives one to four column blocks with a
    partial last one;
  * random inputs: an element of x passes through at most 63 additions of
    its chunk's chain, at most S additions of its slot chain, 2 of the join
    and 1 of the final += (n = 64 + S + 2 roundings; padded zeros add none);
    the prefill passes through the last one only:
        |out - ref| <= gamma_n sum_r |x[r, c]| + gamma_1 |prefill[c]|,
    gamma_n = n u / (1 - n u), u = 2^-24, against float64.

relu_mask_bf16_(dx, x): dx = x > 0 ? dx : +0 in place, 8 bf16 per thread,
decided from x's bits (sign clear and not zero).  x walks all bf16 bit
patterns except NaNs (+0, -0, subnormals, infinities, every finite value);
the result is compared as bits.  NaN is not a specified input of the op: the
kernel keeps dx for a NaN with a clear sign bit and zeroes it for one with
the sign bit set, where IEEE `x > 0` is false for both.
"""

import pytest
import torch

from tests._lstm_oracle import U, gamma

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 63, 64, 65, 129, 257, 512)
CS = (1, 255, 256, 257, 1000, 1024)
PAD = 3  # NaN rows before and after x


def _C():
  from scalable_agent_amd import ops
  ops.load()
  return ops.ext()


def _slots(n):
  return (n + 63) // 64


def _embedded(x, dev):
  """x as a contiguous row range of a NaN-filled device buffer."""
  rows = x.reshape(-1, x.shape[-1])
  buf = torch.full((rows.shape[0] + 2 * PAD, rows.shape[1]), float('nan'), device=dev)
  buf[PAD:PAD + rows.shape[0]] = rows.to(dev)
  view = buf[PAD:PAD + rows.shape[0]].view(x.shape)
  assert view.is_contiguous() and view.data_ptr() != buf.data_ptr()
  return buf, view


def _ints(seed, *shape):
  gen = torch.Generator().manual_seed(seed)
  return torch.randint(-8, 9, shape, generator=gen).float()


def _prefill_ints(seed, C):
  gen = torch.Generator().manual_seed(seed)
  p = torch.randint(1, 6, (C,), generator=gen) * (2 * torch.randint(0, 2, (C,), generator=gen) - 1)
  return p.float()


assert [_slots(n) for n in NS] == [1, 1, 1, 1, 1, 1, 2, 3, 5, 8]


@pytest.mark.parametrize('C', CS)
@pytest.mark.parametrize('N', NS)
def test_colsum_integers_exact(cuda, N, C):
  x = _ints(N * 2000 + C, N, C)
  pre = _prefill_ints(N + C, C)
  buf, view = _embedded(x, cuda)
  out = pre.clone().to(cuda)
  _C().colsum_f32_(view, out)
  ref = (pre.double() + x.double().sum(0)).float()
  assert bool((pre != 0).all()) and float(ref.abs().max()) < 2 ** 24
  assert torch.equal(out.cpu(), ref)
  # the op read x only: the buffer still holds x between its NaN rows
  assert torch.equal(buf[PAD:PAD + N].cpu(), x)
  assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + N:]).all())


def test_colsum_integers_3d(cuda):
  """[T, B, C]: every leading dimension is a row (N = T * B = 65, two
  slots; C = 257, two column blocks)."""
  T, B, C = 5, 13, 257
  x = _ints(77, T, B, C)
  pre = _prefill_ints(78, C)
  _, view = _embedded(x, cuda)
  assert view.shape == (T, B, C)
  out = pre.clone().to(cuda)
  _C().colsum_f32_(view, out)
  assert torch.equal(out.cpu(), (pre.double() + x.double().sum((0, 1))).float())


@pytest.mark.parametrize('N,C', [(1, 257), (17, 256), (63, 1), (65, 257), (129, 1000),
                                 (257, 255), (512, 1024), (300, 1024)])
def test_colsum_random_bound(cuda, N, C):
  gen = torch.Generator().manual_seed(N * 3000 + C)
  x = torch.randn(N, C, generator=gen) * torch.exp2(
      torch.randint(-6, 7, (N, C), generator=gen).float())
  pre = torch.randn(C, generator=gen) * 10
  _, view = _embedded(x, cuda)
  out = pre.clone().to(cuda)
  _C().colsum_f32_(view, out)
  ref = pre.double() + x.double().sum(0)
  bound = gamma(64 + _slots(N) + 2) * x.double().abs().sum(0) + gamma(1) * pre.double().abs()
  err = (out.cpu().double() - ref).abs()
  print('  N %d C %d S %d  max err %.3e  err/bound %.4f' %
        (N, C, _slots(N), float(err.max()), float((err / bound).max())))
  assert U < float(bound.min()) and bool(torch.isfinite(bound).all())
  assert bool((err <= bound).all())


def _from_bits(bits):
  """int tensor of 16-bit patterns -> bf16 tensor with those bits."""
  return (bits.to(torch.int32) & 0xffff).to(torch.int16).view(torch.bfloat16)


def _as_bits(x):
  return x.contiguous().view(torch.int16)


def _all_patterns():
  p = torch.arange(1 << 16, dtype=torch.int32)
  nan = ((p & 0x7f80) == 0x7f80) & ((p & 0x007f) != 0)
  p = p[~nan]
  assert p.numel() == 65536 - 254
  # pad to a multiple of 8 with +0 / -0
  tail = torch.tensor([0x0000, 0x8000] * 4, dtype=torch.int32)[:(-p.numel()) % 8]
  return torch.cat([p, tail])


@pytest.mark.parametrize('dx_kind', ['mixed', '+inf', '-inf', 'ones'])
def test_relu_mask_all_bit_patterns(cuda, dx_kind):
  xb = _all_patterns()
  n = xb.numel()
  assert n % 8 == 0 and n // 8 > 256 * 31  # 32 workgroups, the last partial
  if dx_kind == 'mixed':  # every pattern again, NaNs and infinities included, decorrelated
    db = (torch.arange(n, dtype=torch.int64) * 40503 + 0x7f80) & 0xffff
  else:
    db = torch.full((n,), {'+inf': 0x7f80, '-inf': 0xff80, 'ones': 0xffff}[dx_kind])
  x, dx = _from_bits(xb), _from_bits(db)
  pos = x.float() > 0
  # the specials the mask turns on: +0, -0, smallest subnormals, infinities
  spec = {0x0000: False, 0x8000: False, 0x0001: True, 0x8001: False, 0x007f: True,
          0x0080: True, 0x7f7f: True, 0x7f80: True, 0xff80: False, 0xff7f: False}
  for pat, want in spec.items():
    assert bool(pos[xb == pat].all()) == want and bool((xb == pat).any())
  want = torch.where(pos, _as_bits(dx), torch.zeros(n, dtype=torch.int16))
  d = dx.to(cuda)
  xd = x.to(cuda)
  _C().relu_mask_bf16_(d, xd)
  assert torch.equal(_as_bits(d.cpu()), want)
  assert torch.equal(_as_bits(xd.cpu()), _as_bits(x))


@pytest.mark.parametrize('numel', [8, 8 * 255, 8 * 256, 8 * 257])
def test_relu_mask_sizes_and_sentinels(cuda, numel):
  """One thread, one thread short of a workgroup, exactly one, one thread
  into a second: nothing past numel is read into the result or written."""
  gen = torch.Generator().manual_seed(numel)
  tail = 64
  xs = torch.randn(numel + tail, generator=gen)
  xs[torch.rand(numel + tail, generator=gen) < 0.1] = 0.0
  xs[numel:] = 1.0  # positive past the end: a masked write there would show
  xs[numel - 1] = -1.0
  ds = torch.randn(numel + tail, generator=gen).bfloat16()
  ds[numel:] = -7.0
  xbuf, dbuf = xs.bfloat16().to(cuda), ds.to(cuda)
  _C().relu_mask_bf16_(dbuf[:numel], xbuf[:numel])
  want = torch.where(xs.bfloat16()[:numel].float() > 0, _as_bits(ds[:numel]),
                     torch.zeros(numel, dtype=torch.int16))
  got = dbuf.cpu()
  assert torch.equal(_as_bits(got[:numel]), want)
  assert torch.equal(_as_bits(got[numel:]), _as_bits(ds[numel:]))
  assert torch.equal(_as_bits(xbuf.cpu()), _as_bits(xs.bfloat16()))


@pytest.mark.parametrize('numel', [1, 7, 9, 8 * 256 + 4])
def test_relu_mask_refuses_ragged_sizes(cuda, numel):
  d = torch.ones(numel, device=cuda, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match='size'):
    _C().relu_mask_bf16_(d, d.clone())
  with pytest.raises(RuntimeError, match='size'):
    _C().relu_mask_bf16_(torch.ones(16, device=cuda, dtype=torch.bfloat16),
                         torch.ones(8, device=cuda, dtype=torch.bfloat16))
  torch.cuda.synchronize()
  assert torch.equal(d.cpu(), torch.ones(numel, dtype=torch.bfloat16))
