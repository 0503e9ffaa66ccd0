"""The actor's T = 1 core step as ONE launch (csrc/kernels/actor_core.hip).

After the torso-FC GEMM an fp32 inference step used to be five dependent
launches (x-projection GEMM, its split-K reduce, the LSTM step, heads +
sampler, the board epilogue), each at its launch floor.  `actor_core_step`
does all of it in one exact-fp32 kernel: the workgroups that own the hidden
units hand their slice of the new state to the row tile's last arriver (no
workgroup waits for another), which forms the heads, samples and - on an
inference board - commits the masked state and packs the outputs.

`actor_core_step(..., dtype=torch.bfloat16)` is the same launch for a bf16
inference step (csrc/kernels/actor_core_bf16.hip): the gate product runs on
the bf16 MFMA with fp32 accumulation - h_aug, the kept h_in and the weights
rounded to bf16 once, everything else fp32.  That is the rounding of the
learner's bf16 gang recurrence, not of the bf16 ops step (whose LSTM step
takes h_in W_h in fp32): the two bf16 inference paths are close, not bitwise.
"""

import collections

import torch

from ._ext import ext
from .core import CORE

_TICKET_WORDS = 4096  # one per 16-row tile
_TICKETS = {}

# the inference board's epilogue folded into the step: mask [R] (or [R, 1])
# fp32, offs = byte offsets of (action, logits, baseline, c, h) in a slot
# block, M rows per slot, slot_bytes, out = the uint8 output block, out_addr
# != 0 = pack into that device-accessible address instead (masked rows only)
BoardEpilogue = collections.namedtuple(
    'BoardEpilogue', 'mask offs M slot_bytes out out_addr')


def tickets(device):
  """Arrival counters of the row tiles, zero between launches (the kernel
  re-arms them).  One tensor per (device, current stream): launches on one
  stream are ordered, launches of two inference lanes on two streams run
  side by side and must not share counters."""
  key = (torch.device(device), torch.cuda.current_stream(device).cuda_stream)
  t = _TICKETS.get(key)
  if t is None:
    t = torch.zeros(_TICKET_WORDS, dtype=torch.int32, device=device)
    _TICKETS[key] = t
  return t


def packed_rows(num_actions):
  """K_max: rows of W_x in the packed weights (the instruction columns
  included, padded to 16)."""
  return (CORE + 1 + num_actions + 64 + 15) // 16 * 16


def actor_core_pack(lstm_kernel, num_actions, out=None):
  """lstm_kernel [f_in + 256, 1024] -> [W_x[:K_max]; W_h] in the step
  kernel's B-operand layout, one launch (no backward packing)."""
  kmax = packed_rows(num_actions)
  if out is None:
    out = torch.empty((kmax + CORE) * 4 * CORE, dtype=torch.float32,
                      device=lstm_kernel.device)
  ext().actor_core_pack(lstm_kernel.detach().contiguous(),
                        CORE + 1 + num_actions + 64, out)
  return out


def packed_rows_bf16(num_actions):
  """K_max of the bf16 packing: rows of W_x (the instruction columns
  included) padded to the bf16 MFMA's k-step of 32."""
  return (CORE + 1 + num_actions + 64 + 31) // 32 * 32


def padded_k_bf16(k):
  """The W_x rows a bf16 step of width k reads: k padded to 32."""
  return (k + 31) // 32 * 32


def actor_core_bf16_pack(lstm_kernel, num_actions, out=None):
  """lstm_kernel [f_in + 256, 1024] fp32 -> wpk16: [W_x[:K_max]; W_h] rounded
  to bf16 (RNE) in the bf16 step kernel's B-operand layout.  One launch, no
  scratch."""
  kmax = packed_rows_bf16(num_actions)
  if out is None:
    out = torch.empty((kmax + CORE) * 4 * CORE, dtype=torch.bfloat16,
                      device=lstm_kernel.device)
  ext().actor_core_bf16_pack(lstm_kernel.detach().contiguous(),
                             CORE + 1 + num_actions + 64, out)
  return out


def actor_core_bf16_info(rows, k, num_actions):
  """Host only: {'grid', 'ksteps', 'kpad', 'width', 'max_k'} of the bf16
  step's launch for `rows` rows of a width-k core input."""
  return ext().actor_core_bf16_info(int(rows), int(k), int(num_actions))


def actor_core_step(h_aug, done, c_in, h_in, wpk, b_lstm, policy_w, policy_b,
                    baseline_w, baseline_b, stream, epilogue=None,
                    ticket_words=None, dtype=torch.float32, outs=None):
  """h_aug [R, K] fp32 (ops.core.core_input_f32), done [R] bool / uint8,
  state (c_in, h_in) [R, 256], wpk from actor_core_pack, b_lstm [1024],
  heads policy_w [256, A] (A <= heads.ACTOR_MAX_ACTIONS) / policy_b /
  baseline_w [256, Kv] / baseline_b (value head 0 is reported), stream a
  PhiloxStream (advanced by one).
  -> (action [R] int64, logits [R, A], baseline [R], c2, h2).

  epilogue (a BoardEpilogue): c_in / h_in also take c2 / h2 in place where
  the mask is set, and the five outputs are packed slot-major into its
  block, in the same launch.

  dtype=torch.bfloat16: the bf16 MFMA step.  wpk is actor_core_bf16_pack's;
  h_aug stays fp32 (rounded once on load) and may be a column range
  [R, K] of a wider matrix, K >= 257 + A its true width (the instruction
  columns only when there is an instruction).  outs: optional (action,
  logits, baseline, c2, h2) buffers of >= R rows; their first R rows are
  written and returned."""
  if dtype not in (torch.float32, torch.bfloat16):
    raise ValueError('actor_core_step: dtype must be float32 or bfloat16')
  bf16 = dtype == torch.bfloat16
  if outs is not None and not bf16:
    raise ValueError('actor_core_step: outs needs dtype=torch.bfloat16')
  if h_in.shape[0] > 16 * _TICKET_WORDS:
    raise ValueError('actor_core_step: at most %d rows' % (16 * _TICKET_WORDS))
  dev = h_aug.device
  tk = tickets(dev) if ticket_words is None else ticket_words
  done = done.contiguous()
  if done.dtype == torch.bool:
    done = done.view(torch.uint8)
  c_in, h_in = c_in.float(), h_in.float()
  if epilogue is not None and not (c_in.is_contiguous() and
                                   h_in.is_contiguous()):
    raise ValueError('actor_core_step: the epilogue commits into c_in / h_in, '
                     'which must be contiguous fp32')
  counter = None
  offset = 0
  if stream.counter is not None and stream.counter.device == dev:
    counter = stream.counter
  else:
    offset = stream.next_offset()
  kw = {}
  if epilogue is not None:
    kw = dict(epi_mask=epilogue.mask.reshape(-1), epi_offs=list(epilogue.offs),
              epi_out=epilogue.out, epi_M=int(epilogue.M),
              epi_slot_bytes=int(epilogue.slot_bytes),
              epi_out_addr=int(epilogue.out_addr))
  if bf16:
    step = ext().actor_core_bf16_step
    if outs is not None:
      kw['outs'] = list(outs)
  else:
    step = ext().actor_core_step
  action, logits, baseline, c2, h2 = step(
      h_aug, done, c_in.contiguous(), h_in.contiguous(), wpk,
      b_lstm.contiguous(), policy_w.contiguous(), policy_b.contiguous(),
      baseline_w.reshape(CORE, -1).contiguous(),
      baseline_b.reshape(-1).contiguous(), tk, stream.seed, offset, counter,
      **kw)
  return action, logits, baseline, c2, h2
