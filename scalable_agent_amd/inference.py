"""Batched actor inference on the GPU (the reference's dynamic-batching path,
experiment.py:534-546 + dynamic_batching.py).

`InferenceModel` owns its OWN copy of the agent parameters on the device (a
versioned weight snapshot): the learner publishes new
weights after every update with one device-to-device copy of the flat buffer,
so an inference batch never reads half-updated weights.  Inference runs on a
dedicated HIP stream, concurrently with the learner stream.  On the HIP
backend the heads and the categorical sample are one kernel (actor_io.hip,
Gumbel-max over a device-side Philox stream) for up to
ops.heads.ACTOR_MAX_ACTIONS (63) actions; a larger action set samples with
torch.multinomial from a torch.Generator.

`make_batched_infer` wraps it with the C++ dynamic batcher: actor threads call
it with batch-1 numpy arrays; a runner thread executes batches of up to
`max_batch` rows (timeout `timeout_ms`).  On a GPU the runner is
`StagedBatchedInfer`: the native batcher gathers the request rows straight into
ONE pinned host slab (`GetInputsPacked`), the batch goes to the device with ONE
async copy, the five outputs come back packed in ONE device->host copy into a
pinned slab, and one stream synchronisation ends the batch (SURVEY.md §2.2
"beyond the reference").
"""

import logging
import threading
import time

import numpy as np
import torch

from . import dynamic_batching
from .optim import FlatParams
from .structs import StepOutput, StepOutputInfo


log = logging.getLogger('scalable_agent_amd')
_torch_sampler_logged = False


def _log_torch_sampler(num_actions, limit):
  """Once per process: why HIP actors do not use the device-side sampler."""
  global _torch_sampler_logged
  if not _torch_sampler_logged:
    _torch_sampler_logged = True
    log.info('actor inference samples with torch.multinomial: %d actions, the '
             'HIP heads + sampler kernels take at most %d (an inference board '
             'runs its Python serve loop)', num_actions, limit)


class InferenceModel(object):

  def __init__(self, agent, device, use_instruction=True, seed=0):
    self.device = torch.device(device)
    self.agent = agent.to(self.device)
    self.agent.eval()
    self.flat = FlatParams(self.agent)
    self.use_instruction = use_instruction
    self.version = 0
    self._lock = threading.Lock()
    self._stream = (torch.cuda.Stream(self.device)
                    if self.device.type == 'cuda' else None)
    hip = self.device.type == 'cuda' and getattr(agent, 'backend', '') == 'hip'
    if hip:
      # the sampler kernels' action limit; past it the agent samples with
      # torch.multinomial, which takes a torch.Generator
      from .ops.heads import ACTOR_MAX_ACTIONS, PhiloxStream
      if agent.num_actions > ACTOR_MAX_ACTIONS:
        _log_torch_sampler(agent.num_actions, ACTOR_MAX_ACTIONS)
        hip = False
    if hip:
      self._gen = PhiloxStream(seed, device=self.device)
    else:
      self._gen = torch.Generator(device=self.device).manual_seed(seed)
    # the core's per-step weight forms packed / cast once per publish, not
    # per step (HIP agent); this first fill runs on the current stream, which
    # the model's own stream does not wait for: finish it here
    if hasattr(self.agent, 'inference_cache'):
      self.agent.inference_cache()
      if self._stream is not None:
        torch.cuda.current_stream(self.device).synchronize()

  @property
  def stream(self):
    return self._stream

  @property
  def device_sampler(self):
    """True when the sampler's state lives on the device (a PhiloxStream): a
    captured step then draws fresh samples on every replay, also when it is
    launched from C++."""
    from .ops.heads import PhiloxStream
    return isinstance(self._gen, PhiloxStream)

  def publish(self, flat_params, version=None):
    """Copies the learner's flat parameter buffer into the snapshot.

    The copy runs on the inference stream (behind any queued inference
    replay, which still reads the previous snapshot) and the caller's stream
    then waits for it, so the learner's next RMSProp cannot overwrite
    `flat_params` while the copy is still queued: a snapshot never mixes
    two weight versions."""
    with self._lock:
      if self._stream is not None:
        # the learner's stream (its params may live on another device:
        # --inference_device)
        cur = (torch.cuda.current_stream(flat_params.device)
               if flat_params.is_cuda else None)
        if cur is not None:
          ev = torch.cuda.Event()
          ev.record(cur)
          self._stream.wait_event(ev)
        with torch.cuda.stream(self._stream):
          self.flat.params.copy_(flat_params, non_blocking=True)
          self._refresh_cache()
          done = torch.cuda.Event()
          done.record(self._stream)
        if cur is not None:
          cur.wait_event(done)
      else:
        self.flat.params.copy_(flat_params)
        self._refresh_cache()
      self.version = self.version + 1 if version is None else version

  def _refresh_cache(self):
    if hasattr(self.agent, 'refresh_inference_cache'):
      self.agent.refresh_inference_cache()

  @property
  def actor_core(self):
    """'fused' when this model's steps run the one-kernel actor core
    (Agent(actor_core='fused') where it applies), else 'ops'."""
    fused = getattr(self.agent, 'actor_core_fused', None)
    return ('fused' if fused is not None and
            fused(self._gen, self.device.type == 'cuda') else 'ops')

  @property
  def torso_precision(self):
    """'bf16' / 'fp32' (HIP kernels) or 'torch': the torso this model's steps
    actually run (Agent.inference_torso_precision)."""
    prec = getattr(self.agent, 'inference_torso_precision', None)
    return 'torch' if prec is None else prec(self.device.type == 'cuda')

  @property
  def torso_blocks(self):
    """The form this model's torso runs: 'heads' (as 'stage', and the stage-0
    and / or stage-1 head as one kernel: Agent(torso_blocks='heads') where the
    head kernel takes the frames), 'stage' (the last stage, or its two
    blocks, in one kernel and every other residual block as one kernel:
    Agent(torso_blocks='stage') where the stage kernel takes the frames),
    'fused' (one kernel per residual block: 'fused', or 'stage' on frames the
    stage kernel does not take), else 'ops'.  'whole': the shallow torso's
    x / 255 and three convs as one kernel (Agent(torso_blocks='whole') on an
    fp32 HIP shallow agent whose frames the kernel takes); a deep agent built
    with 'whole' reports what 'heads' would."""
    cuda = self.device.type == 'cuda'
    whole = getattr(self.agent, 'torso_whole_form', None)
    if whole is not None and whole(cuda):
      return 'whole'
    fused = getattr(self.agent, 'torso_blocks_fused', None)
    if fused is None or not fused(cuda):
      return 'ops'
    heads = getattr(self.agent, 'torso_head_form', None)
    if heads is not None and heads(cuda):
      return 'heads'
    form = getattr(self.agent, 'torso_stage_form', None)
    return 'stage' if form is not None and form(cuda) else 'fused'

  @property
  def torso_stages(self):
    """What Agent(torso_stages='fused') runs per stage of this model's bf16
    deep torso: a 3-tuple of 'stage', 'tail' or None (Agent.torso_stages_form);
    None where it was not asked for or does not apply (the torso runs as with
    'ops')."""
    form = getattr(self.agent, 'torso_stages_form', None)
    return None if form is None else form(self.device.type == 'cuda')

  @torch.no_grad()
  def step_device(self, last_action, reward, done, frame, instr_ids,
                  instr_len, c, h, has_instr, epilogue=None):
    """Device tensors in -> device tensors (action, logits, baseline, c, h).
    Call under `self._lock` on `self.stream`.  epilogue (only when
    `actor_core == 'fused'`): an ops.actor_core.BoardEpilogue - the step also
    commits the masked rows of the new state into c / h and packs the
    outputs into the board's block."""
    instr = (instr_ids, instr_len) if (self.use_instruction and
                                       has_instr) else None
    env_output = StepOutput(reward, StepOutputInfo(None, None), done,
                            (frame, instr))
    kw = {} if epilogue is None else {'epilogue': epilogue}
    out, (c2, h2) = self.agent.step(last_action, env_output, (c, h),
                                    generator=self._gen, **kw)
    return [out.action, out.policy_logits, out.baseline, c2, h2]

  @torch.no_grad()
  def infer(self, last_action, reward, done, frame, instr_ids, instr_len, c,
            h):
    """Batched numpy in -> numpy out (action, logits, baseline, c, h)."""
    dev = self.device
    with self._lock:
      ctx = (torch.cuda.stream(self._stream) if self._stream is not None
             else _null())
      with ctx:
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(
            dev, non_blocking=True)
        has_instr = int(np.max(instr_len, initial=0)) > 0
        res = self.step_device(t(last_action), t(reward), t(done), t(frame),
                               t(instr_ids), t(instr_len), t(c), t(h),
                               has_instr)
        res = [r.to('cpu', non_blocking=False) for r in res]
    return tuple(r.numpy() for r in res)


class _null(object):
  def __enter__(self):
    return self

  def __exit__(self, *a):
    return False


_ALIGN = 256


def _torch_dtype(np_dtype):
  return torch.from_numpy(np.empty(0, np.dtype(np_dtype))).dtype


class _BucketGraph(object):
  """One captured inference step for a padded batch of `rows` rows: static
  input views into the device slab, outputs copied into a device output
  slab inside the graph."""

  def __init__(self, rows, offsets, graph, out_dev, out_host, layout):
    self.rows, self.offsets, self.graph = rows, offsets, graph
    self.out_dev, self.out_host, self.layout = out_dev, out_host, layout
    self.out_bytes = layout[-1][2] + layout[-1][3]


class StagedBatchedInfer(object):
  """GPU inference server over the native batcher with pinned staging slabs.

  Same calling convention as `dynamic_batching.batch_fn` wrappers:
  `infer(last_action, reward, done, frame, instr_ids, instr_len, c, h)` on
  batch-1 numpy arrays from any number of actor threads, plus
  start/close/cancel/join/stats.

  graphs=True (HIP backend): batches are padded to power-of-two buckets
  (padding rows zeroed in the host slab) and each bucket's whole inference
  step - torso, core, heads + sampler - is ONE hipGraph replay between the
  one H2D and the one D2H copy, so the per-batch host cost no longer scales
  with the ~40 kernel launches of an agent step.
  """

  def __init__(self, model, min_batch=1, max_batch=1024, timeout_ms=100,
               graphs=None):
    self.model = model
    self.max_batch = int(max_batch)
    if graphs is None:
      graphs = (model.device.type == 'cuda' and
                getattr(model.agent, 'backend', '') == 'hip' and
                getattr(model, 'device_sampler', True))
    self.graphs = bool(graphs)
    self._bucket_graphs = {}
    self._pool = None
    self.busy_s = 0.0  # server time from batch taken to outputs scattered
    self._batcher = dynamic_batching.Batcher(min_batch, max_batch, timeout_ms)
    self._lock = threading.Lock()
    self._thread = None
    self._error = None
    self._stop_requested = False
    self._in_host = self._in_dev = None
    self._out_host = self._out_dev = None
    self.state = {'batcher': self._batcher}

  # ---- slabs -------------------------------------------------------------
  def _pinned(self, nbytes):
    t = torch.empty(nbytes, dtype=torch.uint8)
    return t.pin_memory() if self.model.device.type == 'cuda' else t

  def _ensure_in_slabs(self, args):
    if self._in_host is not None:
      return
    per_row = sum((np.asarray(a).nbytes + _ALIGN) for a in args)
    cap = self.max_batch * per_row + _ALIGN * len(args)
    self._in_host = self._pinned(cap)
    self._in_dev = torch.empty(cap, dtype=torch.uint8,
                               device=self.model.device)

  def _out_slabs(self, nbytes):
    if self._out_dev is None or self._out_dev.numel() < nbytes:
      cap = max(nbytes, 1 << 16)
      self._out_host = self._pinned(cap)
      self._out_dev = torch.empty(cap, dtype=torch.uint8,
                                  device=self.model.device)
    return self._out_host, self._out_dev

  # ---- runner ------------------------------------------------------------
  def _serve_one(self):
    if self.graphs:
      return self._serve_one_graph()
    m = self.model
    host = self._in_host
    n, cid, used, _, metas = self._batcher.get_inputs_packed(
        host.data_ptr(), host.numel(), _ALIGN)
    self._t_taken = time.perf_counter()
    hnp = host.numpy()
    ctx = torch.cuda.stream(m.stream) if m.stream is not None else _null()
    with m._lock, ctx:
      self._in_dev[:used].copy_(host[:used], non_blocking=True)
      views, hviews = [], []
      for dt, shape, off in metas:
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        views.append(self._in_dev[off:off + nb].view(
            _torch_dtype(dt)).view(*shape))
        hviews.append(hnp[off:off + nb].view(np.dtype(dt)).reshape(shape))
      has_instr = int(np.max(hviews[5], initial=0)) > 0
      outs = m.step_device(*views, has_instr=has_instr)
      outs = [o.contiguous() for o in outs]
      layout, off = [], 0
      for o in outs:
        layout.append((o.dtype, tuple(o.shape), off))
        off += (o.numel() * o.element_size() + _ALIGN - 1) // _ALIGN * _ALIGN
      ohost, odev = self._out_slabs(off)
      for o, (_, _, oo) in zip(outs, layout):
        odev[oo:oo + o.numel() * o.element_size()].copy_(
            o.view(-1).view(torch.uint8))
      ohost[:off].copy_(odev[:off], non_blocking=True)
      if m.stream is not None:
        m.stream.synchronize()
    onp = ohost.numpy()
    result = []
    for (dt, shape, oo), o in zip(layout, outs):
      npdt = torch.empty(0, dtype=dt).numpy().dtype
      nb = o.numel() * o.element_size()
      result.append(onp[oo:oo + nb].view(npdt).reshape(shape))
    self._batcher.set_outputs(result, cid)

  # ---- graph path ----------------------------------------------------------
  def _capture(self, rows, metas, has_instr):
    m = self.model
    views, layout = [], []
    for dt, shape, off in metas:
      nb = rows * int(np.prod(shape[1:], dtype=np.int64)) * np.dtype(dt).itemsize
      views.append(self._in_dev[off:off + nb].view(_torch_dtype(dt)).view(
          rows, *shape[1:]))
    s = m.stream
    with m._lock, torch.cuda.stream(s):
      for _ in range(2):  # warm-up: lazy library init outside the capture
        m.step_device(*views, has_instr=has_instr)
      s.synchronize()
      if self._pool is None:
        self._pool = torch.cuda.graph_pool_handle()
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g, pool=self._pool, stream=s,
                            capture_error_mode='thread_local'):
        outs = [o.contiguous() for o in m.step_device(*views,
                                                      has_instr=has_instr)]
        off = 0
        for o in outs:
          nb = o.numel() * o.element_size()
          layout.append((o.dtype, tuple(o.shape), off, nb))
          off += (nb + _ALIGN - 1) // _ALIGN * _ALIGN
        out_dev = torch.empty(off, dtype=torch.uint8, device=m.device)
        for o, (_, _, oo, nb) in zip(outs, layout):
          out_dev[oo:oo + nb].copy_(o.view(-1).view(torch.uint8))
    out_host = self._pinned(off)
    return _BucketGraph(rows, [x[2] for x in metas], g, out_dev, out_host,
                        layout)

  def _serve_one_graph(self):
    m = self.model
    host = self._in_host
    n, cid, used, rows, metas = self._batcher.get_inputs_packed(
        host.data_ptr(), host.numel(), _ALIGN, True)
    self._t_taken = time.perf_counter()
    hnp = host.numpy()
    len_dt, len_shape, len_off = metas[5]
    has_instr = int(np.max(hnp[len_off:len_off + n * 8].view(np.int64),
                           initial=0)) > 0
    for dt, shape, off in metas:  # zero the padding rows
      rb = int(np.prod(shape[1:], dtype=np.int64)) * np.dtype(dt).itemsize
      if rows > n:
        hnp[off + n * rb:off + rows * rb] = 0
    key = (rows, has_instr)
    bg = self._bucket_graphs.get(key)
    if bg is None or bg.offsets != [x[2] for x in metas]:
      self._in_dev[:used].copy_(host[:used])
      bg = self._capture(rows, metas, has_instr)
      self._bucket_graphs[key] = bg
    with m._lock, torch.cuda.stream(m.stream):
      self._in_dev[:used].copy_(host[:used], non_blocking=True)
      bg.graph.replay()
      bg.out_host.copy_(bg.out_dev, non_blocking=True)
      m.stream.synchronize()
    onp = bg.out_host.numpy()
    result = []
    for dt, shape, oo, nb in bg.layout:
      npdt = torch.empty(0, dtype=dt).numpy().dtype
      result.append(onp[oo:oo + nb].view(npdt).reshape(shape)[:n])
    self._batcher.set_outputs(result, cid)

  def _run(self):
    try:
      while True:
        self._serve_one()
        self.busy_s += time.perf_counter() - self._t_taken
    except dynamic_batching.CancelledError as e:
      if not self._stop_requested and 'Batcher is closed' not in str(e):
        self._error = e
    except BaseException as e:  # pylint: disable=broad-except
      self._error = e
      try:
        self._batcher.cancel()
      except Exception:  # pragma: no cover
        pass

  # ---- batch_fn-style API ------------------------------------------------
  def start(self):
    with self._lock:
      if self._thread is None:
        self._thread = threading.Thread(target=self._run, daemon=True,
                                        name='staged-inference')
        self._thread.start()

  def __call__(self, *args):
    if self._in_host is None:
      with self._lock:
        self._ensure_in_slabs(args)
    self.start()
    out = self._batcher.compute([np.asarray(a) for a in args])
    return tuple(out)

  def close(self):
    self._stop_requested = True
    self._batcher.close()

  def cancel(self):
    self._batcher.cancel()

  def join(self, timeout=None):
    if self._thread is not None:
      self._thread.join(timeout)
    if self._error is not None:
      raise self._error

  def stats(self):
    return {'batches': int(self._batcher.num_batches),
            'requests': int(self._batcher.num_requests),
            'busy_s': self.busy_s}


def make_batched_infer(model, min_batch=1, max_batch=1024, timeout_ms=100,
                       staged=None, graphs=None):
  """staged: None = pinned-slab server on a GPU, batch_fn runner on CPU;
  graphs: None = per-bucket hipGraph replay on the HIP backend."""
  if staged is None:
    staged = model.device.type == 'cuda'
  if staged:
    return StagedBatchedInfer(model, min_batch, max_batch, timeout_ms,
                              graphs=graphs)
  return dynamic_batching.batch_fn_with_options(
      minimum_batch_size=min_batch, maximum_batch_size=max_batch,
      timeout_ms=timeout_ms)(model.infer)


class VectorInfer(object):
  """Fixed-batch inference for one vectorised actor group
  (runtime/actor_group.py): `rows` envs step in lockstep, so there is no
  dynamic batcher - the group fills ONE pinned input slab, and one H2D copy,
  one captured hipGraph (torso, core, heads + sampler; the LSTM state stays
  on the device between steps) and one D2H copy of the packed outputs make
  an inference step.  Without a GPU (tests) the same calls run eagerly.

  Inputs (host numpy views, fill before `run()`): last_action [M] int64,
  reward [M] f32, done [M] bool, frame [M, H, W, C] u8, instr_ids [M, L]
  int64, instr_len [M] int64.  `run()` -> (action [M], logits [M, A],
  baseline [M], c [M, core], h [M, core]) host numpy views of the state
  AFTER the step (valid until the next run)."""

  _IN = (('last_action', (), np.int64), ('reward', (), np.float32),
         ('done', (), np.bool_), ('frame', None, np.uint8),
         ('instr_ids', ('L',), np.int64), ('instr_len', (), np.int64))

  def __init__(self, model, rows, frame_shape, num_actions, instr_len=16,
               core_size=256, use_graph=None):
    self.model = model
    self.rows = M = int(rows)
    dev = model.device
    self.cuda = dev.type == 'cuda'
    if use_graph is None:
      use_graph = (self.cuda and getattr(model.agent, 'backend', '') == 'hip'
                   and getattr(model, 'device_sampler', True))
    self.use_graph = bool(use_graph) and self.cuda
    shapes = {'frame': tuple(frame_shape), 'instr_ids': (int(instr_len),)}
    layout, off = [], 0
    for name, shape, dt in self._IN:
      shape = shapes.get(name, shape)
      nb = M * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
      layout.append((name, (M,) + tuple(shape), np.dtype(dt), off, nb))
      off += (nb + _ALIGN - 1) // _ALIGN * _ALIGN
    self._in_bytes = off
    self._in_host = self._host(off)
    self._in_dev = (torch.empty(off, dtype=torch.uint8, device=dev)
                    if self.cuda else self._in_host)
    hnp = self._in_host.numpy()
    self.inputs = {n: hnp[o:o + nb].view(dt).reshape(s)
                   for n, s, dt, o, nb in layout}
    self._dev_in = [self._in_dev[o:o + nb].view(_torch_dtype(dt)).view(*s)
                    for n, s, dt, o, nb in layout]
    # device-resident recurrent state
    self.c = torch.zeros(M, core_size, device=dev)
    self.h = torch.zeros(M, core_size, device=dev)
    outs = [('action', (M,), torch.int64), ('logits', (M, num_actions),
                                             torch.float32),
            ('baseline', (M,), torch.float32), ('c', (M, core_size),
                                                 torch.float32),
            ('h', (M, core_size), torch.float32)]
    self._out_layout, off = [], 0
    for n, s, dt in outs:
      nb = int(np.prod(s)) * torch.empty(0, dtype=dt).element_size()
      self._out_layout.append((n, s, dt, off, nb))
      off += (nb + _ALIGN - 1) // _ALIGN * _ALIGN
    self._out_host = self._host(off)
    self._out_dev = (torch.empty(off, dtype=torch.uint8, device=dev)
                     if self.cuda else self._out_host)
    onp = self._out_host.numpy()
    npdt = lambda dt: torch.empty(0, dtype=dt).numpy().dtype
    self._outs = [onp[o:o + nb].view(npdt(dt)).reshape(s)
                  for n, s, dt, o, nb in self._out_layout]
    self._graphs = {}
    self._done = None

  def _host(self, nbytes):
    t = torch.zeros(nbytes, dtype=torch.uint8)
    return t.pin_memory() if self.cuda else t

  def _body(self, has_instr):
    """Device step: inputs -> packed outputs, state updated in place."""
    m = self.model
    la, rw, dn, fr, ids, ln = self._dev_in
    action, logits, baseline, c2, h2 = m.step_device(
        la, rw, dn, fr, ids, ln, self.c, self.h, has_instr=has_instr)
    vals = [action, logits, baseline, c2, h2]
    for (n, s, dt, o, nb), v in zip(self._out_layout, vals):
      self._out_dev[o:o + nb].view(dt).view(*s).copy_(v)
    self.c.copy_(c2)
    self.h.copy_(h2)

  def _capture(self, has_instr):
    m = self.model
    s = m.stream
    with torch.cuda.stream(s):
      # warm-up (lazy library init) then restore the state it advanced
      c0, h0 = self.c.clone(), self.h.clone()
      for _ in range(2):
        self._body(has_instr)
      self.c.copy_(c0)
      self.h.copy_(h0)
      s.synchronize()
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g, stream=s, capture_error_mode='thread_local'):
        self._body(has_instr)
    return g

  @torch.no_grad()
  def launch(self):
    """Enqueues H2D + step + D2H on the model's stream; the input slab may
    be rewritten (and the outputs read) only after `wait()`."""
    m = self.model
    has_instr = bool(m.use_instruction and
                     int(self.inputs['instr_len'].max(initial=0)) > 0)
    if not self.cuda:
      self._body(has_instr)
      return
    with m._lock, torch.cuda.stream(m.stream):
      self._in_dev.copy_(self._in_host, non_blocking=True)
      if self.use_graph:
        g = self._graphs.get(has_instr)
        if g is None:
          g = self._graphs[has_instr] = self._capture(has_instr)
        g.replay()
      else:
        self._body(has_instr)
      self._out_host.copy_(self._out_dev, non_blocking=True)
      if self._done is None:
        self._done = torch.cuda.Event()
      self._done.record(m.stream)

  def wait(self):
    if self.cuda:
      # poll + yield: a spinning hipEventSynchronize per group process would
      # take CPU from the env workers, a blocking (interrupt) wait adds
      # wake-up latency to every step
      while not self._done.query():
        time.sleep(0)
    return tuple(self._outs)

  def run(self):
    self.launch()
    return self.wait()
