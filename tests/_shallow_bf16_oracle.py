"""Shared constructions for the bf16 shallow torso tests: TF-SAME pads, a
float64 conv chain with explicit pads, and the exact-integer case whose every
stored value is an integer <= 256 (exact in bf16)."""

import torch
import torch.nn.functional as F

FRAMES = [(72, 96, 3), (84, 84, 4), (72, 128, 3), (72, 96, 1)]
LAYERS = ((8, 4, 32), (4, 2, 64), (3, 2, 128))  # (kernel, stride, cout)
NNZ = (3, 6, 9)    # non-zero taps per output channel
BMAX = (1, 2, 8)   # biases are integers in [0, bmax]
BOUNDS = (4, 26, 242)


def pads(n, k, s):
  """TF SAME: (output size, pad before, pad after)."""
  out = -(-n // s)
  total = max((out - 1) * s + k - n, 0)
  return out, total // 2, total - total // 2


def out_shape(shape):
  h, w = shape[0], shape[1]
  for k, s, _ in LAYERS:
    h, w = pads(h, k, s)[0], pads(w, k, s)[0]
  return h, w, 128


def chain64(frames, ws, bs):
  """uint8 NHWC frames, HWIO weights, biases (any float dtype, CPU) ->
  float64 NHWC features: x / 255, then conv + bias + ReLU per layer with the
  TF-SAME pads written out."""
  x = (frames.double() / 255.0).permute(0, 3, 1, 2)
  for (k, s, _), w, b in zip(LAYERS, ws, bs):
    _, pt, pb = pads(x.shape[2], k, s)
    _, pl, pr = pads(x.shape[3], k, s)
    x = F.relu(F.conv2d(F.pad(x, (pl, pr, pt, pb)),
                        w.double().permute(3, 2, 0, 1), b.double(), stride=s))
  return x.permute(0, 2, 3, 1).contiguous()


def integer_weights(c, phase, seed=31):
  """-> (ws, bs): layer l has NNZ[l] taps of +-1 (+1 with probability 3/4)
  per output channel o, the j-th at flat tap index
  (phase * cout * nnz + o * nnz + j) mod K, K = kh * kw * cin; integer biases
  in [0, BMAX[l]]."""
  g = torch.Generator().manual_seed(seed + phase)
  ws, bs = [], []
  cin = c
  for (k, _, cout), nnz, bmax in zip(LAYERS, NNZ, BMAX):
    K = k * k * cin
    w = torch.zeros(K, cout)
    o = torch.arange(cout).repeat_interleave(nnz)
    j = torch.arange(nnz).repeat(cout)
    idx = (phase * cout * nnz + o * nnz + j) % K
    val = torch.where(torch.rand(cout * nnz, generator=g) < 0.75, 1.0, -1.0)
    w[idx, o] = val
    assert int((w != 0).sum()) == cout * nnz  # no two taps of a channel collide
    ws.append(w.reshape(k, k, cin, cout))
    bs.append(torch.randint(0, bmax + 1, (cout,), generator=g).float())
    cin = cout
  return ws, bs


def running_bounds(ws, bs):
  """max |value| after each layer for inputs in [0, 1]."""
  bound, out = 1.0, []
  for w, b in zip(ws, bs):
    bound = (w.abs().sum(dim=(0, 1, 2)).max().item() * bound +
             b.abs().max().item())
    out.append(bound)
  return out


def binary_frames(shape, n=3, seed=7):
  g = torch.Generator().manual_seed(seed)
  return (torch.randint(0, 2, (n,) + tuple(shape), generator=g) *
          255).to(torch.uint8)
