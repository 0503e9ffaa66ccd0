"""Time-major trajectory batch queue (native csrc/envpool/traj_queue.cc).

Replaces the reference's actor -> learner path (experiment.py:530-531
FIFOQueue(1) + enqueue, :576 dequeue_many, :579-585 time-major transposes,
:587-597 StagingArea put/get) with:

  actors ──(write [t, b] in place)──> shm slab = ONE learner batch
  learner ──(one memcpy)──> pinned staging buffer
          ──(ONE hipMemcpyAsync per step, copy stream)──> device slot
                 ──(event)──> captured learner graph

No unroll is ever stacked, transposed or memcpy'd on the host: each actor
claims a column b of the slab being filled and writes every step's fields
straight into their time-major position; the B-th commit publishes the slab.
The slabs are shared (pageable) memory that actor processes forked before
the GPU was initialised write to, so they cannot be allocated pinned; the
learner moves a full slab into a pinned buffer of its own (hipHostMalloc,
through torch's pin_memory) and releases the slab at once, and the DMA from
that buffer overlaps the previous step's compute.

`BatchLayout` is the flat byte layout of one batch (256-B aligned segments,
fields in ActorOutput order); the learner's device slots use the same layout,
so host slab -> device slot is one contiguous copy.
"""


import numpy as np
import torch

from ..structs import ActorOutput, AgentOutput, StepOutput, StepOutputInfo

ALIGN = 256


class BatchLayout(object):
  """Offsets of every field of one [T+1, B] learner batch in a flat buffer."""

  def __init__(self, T1, B, frame_shape, num_actions, use_instruction=False,
               instr_len=16, core_size=256):
    self.T1, self.B = T1, B
    self.use_instruction = use_instruction
    fields = [('level', (B,), np.int64),
              ('c', (B, core_size), np.float32),
              ('h', (B, core_size), np.float32),
              ('reward', (T1, B), np.float32),
              ('episode_return', (T1, B), np.float32),
              ('episode_step', (T1, B), np.int32),
              ('done', (T1, B), np.bool_),
              ('frame', (T1, B) + tuple(frame_shape), np.uint8)]
    if use_instruction:
      fields += [('instr_ids', (T1, B, instr_len), np.int64),
                 ('instr_len', (T1, B), np.int64)]
    fields += [('action', (T1, B), np.int64),
               ('policy_logits', (T1, B, num_actions), np.float32),
               ('baseline', (T1, B), np.float32)]
    self.fields = []
    off = 0
    for name, shape, dt in fields:
      off = (off + ALIGN - 1) // ALIGN * ALIGN
      nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
      self.fields.append((name, shape, np.dtype(dt), off, nbytes))
      off += nbytes
    self.nbytes = (off + ALIGN - 1) // ALIGN * ALIGN

  def numpy_views(self, buf):
    """buf: a writable buffer of >= nbytes -> {field: ndarray view}."""
    base = np.frombuffer(buf, dtype=np.uint8, count=self.nbytes)
    return {name: base[off:off + nb].view(dt).reshape(shape)
            for name, shape, dt, off, nb in self.fields}

  def torch_views(self, flat):
    """flat: a uint8 tensor (host or device) of >= nbytes -> ActorOutput of
    tensor views (level_name = the [B] level-index tensor)."""
    tdt = {np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32,
           np.dtype(np.int32): torch.int32, np.dtype(np.bool_): torch.bool,
           np.dtype(np.uint8): torch.uint8}
    v = {name: flat[off:off + nb].view(tdt[dt]).view(shape)
         for name, shape, dt, off, nb in self.fields}
    instr = ((v['instr_ids'], v['instr_len']) if self.use_instruction
             else None)
    return ActorOutput(
        level_name=v['level'], agent_state=(v['c'], v['h']),
        env_outputs=StepOutput(v['reward'],
                               StepOutputInfo(v['episode_return'],
                                              v['episode_step']),
                               v['done'], (v['frame'], instr)),
        agent_outputs=AgentOutput(v['action'], v['policy_logits'],
                                  v['baseline']))


class TrajectoryQueue(object):
  """K slabs of one learner batch each; see the module docstring.

  name='' : anonymous shared mapping (actor threads / forked processes);
  '/name': a named POSIX shm object other processes can attach to.
  """

  def __init__(self, layout, num_slabs, name=''):
    from . import native
    self.layout = layout
    self.q = native.TrajQueue(name, int(num_slabs), layout.nbytes, layout.B,
                              True)
    self.slab_bytes = self.q.slab_bytes
    self._views = [layout.numpy_views(self.q.slab_view(s))
                   for s in range(self.q.num_slabs)]
    self._tensors = [torch.frombuffer(self.q.slab_view(s),
                                      dtype=torch.uint8)[:layout.nbytes]
                     for s in range(self.q.num_slabs)]

  # ---------------------------------------------------------- producers
  def claim(self, timeout_ms=-1):
    """-> (slab, column, numpy views of the slab); slab < 0: timeout/closed."""
    s, col = self.q.claim(int(timeout_ms))
    return s, col, (self._views[s] if s >= 0 else None)

  def claim_n(self, n, timeout_ms=-1):
    """All-or-nothing claim of n columns -> list of (slab, column, views),
    or -1 (timeout) / -2 (closed)."""
    status, pairs = self.q.claim_n(int(n), int(timeout_ms))
    if status < 0:
      return status
    return [(s, c, self._views[s]) for s, c in pairs]

  def commit(self, slab):
    self.q.commit(int(slab))

  # ---------------------------------------------------------- consumer
  def acquire(self, timeout_ms=-1):
    return self.q.acquire(int(timeout_ms))

  def release(self, slab):
    self.q.release(int(slab))

  def host_tensor(self, slab):
    """uint8 tensor over the slab's bytes (pageable shared memory)."""
    return self._tensors[slab]

  def host_views(self, slab):
    return self._views[slab]

  @property
  def closed(self):
    return bool(self.q.closed)

  @property
  def num_ready(self):
    return self.q.num_ready

  def close(self):
    """Closes the native queue (wakes every waiter)."""
    self.q.close()
