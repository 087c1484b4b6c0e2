"""The reference learners' optimizers as `torch.optim.Optimizer`s over CUDA
tensors, each in two HIP launches per `step()` whatever the number of parameter
tensors.

`LaProp`: embodied/jax/opt.py:109-164 chained by dreamerv3/agent.py:342-379:
adaptive gradient clipping per tensor, RMS scaling, bias-corrected momentum,
optional weight decay and a learning-rate schedule.  Per tensor, in float32, `t`
the number of this update counted from 1 (`eps` is not inside the root):

    unorm = ||g||2 ; pnorm = ||p||2                                   opt.py:116-117
    g1    = g * (1 / maximum(1, unorm / (agc * maximum(pmin, pnorm))))    agc == 0: g
    nu    = beta2 * nu + (1 - beta2) * (g1 * g1)                      opt.py:136-137
    u     = g1 / (sqrt(nu / (1 - beta2**t)) + eps)                    opt.py:138-140
    mu    = (1 - beta1) * u + beta1 * mu                              opt.py:156
    m_hat = mu / (1 - beta1**t)                                       opt.py:161
            nesterov: ((1 - beta1) * u + beta1 * mu) / (1 - beta1**t)  opt.py:157-159
    upd   = (m_hat + wd * p  if the tensor decays else  m_hat) * -lr(t - 1)
    p     = p + upd                                                   agent.py:361-378

`maximum` hands a NaN on, so a NaN anywhere in a tensor's gradient makes that
tensor's p, nu and mu NaN throughout; an infinity and no NaN gives the scale 0:
the finite elements go on with g1 = 0 and the infinite ones become NaN.  No other
tensor is touched.  There is no loss scaling and no skipped step (opt.py:25-29
belongs to float16 compute).

`Adam`: the PPO learner's chain, ppo/agent.py:114-124: optax.clip_by_global_norm,
scale_by_adam, add_decayed_weights, scale_by_learning_rate.  In float32, `t` as
above, count = t - 1:

    gnorm = sqrt(sum over EVERY tensor of sum g^2)                    optax.global_norm
    g1    = g  if clip == 0 or gnorm < clip  else  (g / gnorm) * clip    clip_by_global_norm
    mu    = beta1 * mu + (1 - beta1) * g1
    nu    = beta2 * nu + (1 - beta2) * (g1 * g1)
    u     = (mu / (1 - beta1**t)) / (sqrt(nu / (1 - beta2**t)) + eps)  scale_by_adam, eps_root = 0
    u     = u + wd * p  if the tensor decays                          add_decayed_weights
    upd   = u * -lr(count) ;  p = p + upd

The clip is a select on `gnorm < clip`, not a `min`, and the norm is one number
for all tensors.  So, on purpose unlike LaProp's per-tensor containment and as the
reference behaves: a NaN in ANY gradient makes p, mu and nu NaN in EVERY tensor;
an infinity and no NaN gives g / inf * clip, 0 for the finite elements of every
tensor and NaN for the infinite ones.  gnorm == 0 leaves the gradients alone.

Two paths each, as the heads in `outs.py`: the composed one restates the
reference line by line in torch ops and is the definition; the fused one is
csrc/optim.hip.

`SlowModel`: the reference's slow (EMA) target network, embodied/jax/utils.py:94-127,
`self.slowval.update()` of dreamerv3/agent.py:142: in one launch of its own, or
inside the update launch of an optimizer it is attached to.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import api

MAX_ELEMENTS = 2 ** 31 - 1          # per tensor, on the kernels; any total


def _geometry():
  chunk, record = C.c_int64(0), C.c_int64(0)
  api.emb_optim_table(None, None, None, 0, None, None, 0, None, C.byref(chunk), C.byref(record))
  return chunk.value, record.value


# Elements per chunk (one tensor's, one workgroup's, one partial sum's) and bytes
# per record of the device table: csrc/optim.h holds both.
CHUNK, RECORD_BYTES = _geometry()
BF16, DECAY = 1, 2                  # EMB_OPTIM_BF16, EMB_OPTIM_DECAY
_GRADS = {torch.float32: 0, torch.bfloat16: BF16}


def optimizer_launches():
  """Kernel launches `emb_optim_norms`, `emb_optim_update`, `emb_optim_grad_norms`,
  `emb_optim_adam_update` and `emb_optim_metrics` have issued in this process, and
  those of `SlowModel`: `emb_slow_update`, one per stand-alone `update()` that is
  due, and `emb_optim_update_slow` / `emb_optim_adam_update_slow`, which take the
  place of an attached optimizer's update launch."""
  return _lib.launches('optim')


def warmup_schedule(lr, warmup):
  """`count -> lr * min(count / warmup, 1)`: the reference's default schedule,
  join_schedules([linear_schedule(0, lr, warmup), constant_schedule(lr)],
  [warmup]) of agent.py:367-378, and optax.linear_schedule(0, lr, warmup) of
  ppo/agent.py:118, which is the same function.  warmup == 0: the constant."""
  lr, warmup = float(lr), int(warmup)
  if not warmup:
    return lambda count: lr
  return lambda count: lr * min(count / warmup, 1.0)


def _check_param(index, param):
  """A parameter the optimizers take: a CUDA float32 tensor."""
  if not torch.is_tensor(param):
    raise TypeError(f'embodied_amd.optim: parameter {index} is a {type(param).__name__}, not a tensor')
  if param.dtype != torch.float32:
    raise TypeError(f'embodied_amd.optim: parameter {index} must be float32, got {param.dtype} '
                    '(no CPU fallback, no other dtype)')
  if not param.is_cuda:
    raise RuntimeError(f'embodied_amd.optim runs as HIP kernels: parameter {index} is not a CUDA tensor '
                       '(no CPU fallback)')


def _check_hyper(who, betas, amounts, lr, warmup):
  """The checks both optimizers make before they touch a parameter.  Returns the
  schedule: the callable `lr`, or None for a float."""
  for name, value in betas.items():
    if not 0.0 <= value < 1.0:
      raise ValueError(f'{who}: {name} = {value!r} is outside [0, 1)')
  for name, value in amounts.items():
    if not (value >= 0.0 and np.isfinite(value)):
      raise ValueError(f'{who}: {name} = {value!r} must be finite and not negative')
  if int(warmup) != warmup or warmup < 0:
    raise ValueError(f'{who}: warmup = {warmup!r} must be a whole number of updates, 0 or more')
  if callable(lr):
    if warmup:
      raise ValueError(f'{who}: warmup goes with a float lr; a callable lr is the whole schedule')
    return lr
  if not np.isfinite(lr):
    raise ValueError(f'{who}: lr = {lr!r} must be finite')
  return None


# `fused=None`: the kernels wherever they fit.  On the MI355X the fused median is
# below the composed one at all six rows of profiles/optim_bench.txt -- 1 M
# parameters in 40 tensors 72.2 us against 6572.8 (bf16 gradients 74.8 / 6917.9),
# the 12.2 M PPO model 81.8 / 7532.0 (80.4 / 7750.6), the 166 M DreamerV3 model
# 1050.5 / 15853.6 (941.7 / 17519.4) -- so there is no size below which the
# composed path is taken and no crossover constant here.
# The same holds for `Adam` at all six rows of profiles/adam_bench.txt -- 1 M
# parameters in 40 tensors 73.0 us against 5510.8 (bf16 gradients 73.5 / 5181.9),
# the 12.2 M PPO model 78.8 / 5847.2 (78.6 / 5326.5), the 166 M model 1005.1 /
# 11384.1 (866.9 / 11645.8) -- so `Adam` has no crossover constant either.


def _path(fused, params, who='LaProp'):
  """True: the kernels, False: the composed path.  The kernels take contiguous
  tensors of fewer than 2^31 elements each; one that is not puts the whole
  optimizer on the composed path (fused=None) or is refused (fused=True)."""
  why = None
  for index, param in enumerate(params):
    if not param.is_contiguous():
      why = f'parameter {index} of shape {tuple(param.shape)} is not contiguous'
    elif param.numel() > MAX_ELEMENTS:
      why = f'parameter {index} has {param.numel()} elements, the kernels index 0 .. 2^31 - 1 per tensor'
    if why:
      break
  if fused and why:
    raise ValueError(f'{who}(fused=True): {why} (fused=None or False composes it)')
  if fused is None:
    return why is None
  return bool(fused)


def _new_plan(device, counts, record_bytes):
  """Pinned staging and device buffers for a table of `record_bytes` per tensor
  and the chunk map of csrc/optim.h over tensors of `counts` elements."""
  counts = np.array(counts, np.int64)
  n_chunks = int(sum(-(-int(n) // CHUNK) for n in counts))
  chunks = torch.empty(max(n_chunks, 1) * 8, dtype=torch.uint8).pin_memory()
  table = torch.empty(max(len(counts), 1) * record_bytes, dtype=torch.uint8).pin_memory()
  return {'device': device, 'counts': counts, 'n_chunks': n_chunks, 'host_table': table, 'host_chunks': chunks,
          'table': torch.empty(table.numel(), dtype=torch.uint8, device=device),
          'chunks': torch.empty(chunks.numel(), dtype=torch.uint8, device=device), 'addrs': None}


def _upload(plan, first, build):
  """Write the table into pinned memory with `build(table, chunks or None,
  chunk_capacity, n_chunks out)` and copy it to the device on the stream; the
  chunk map only the `first` time, it depends on the sizes alone."""
  if not first:
    # the pinned staging buffer of the previous upload may still be in flight: a
    # new one (the host allocator keeps the old block until its copy is done)
    plan['host_table'] = torch.empty_like(plan['host_table']).pin_memory()
  counted = C.c_int64(-1)
  build(plan['host_table'].data_ptr(), plan['host_chunks'].data_ptr() if first else None, plan['n_chunks'],
        C.byref(counted))
  assert counted.value == plan['n_chunks'], (counted.value, plan['n_chunks'])
  plan['table'].copy_(plan['host_table'], non_blocking=True)
  if first:
    plan['chunks'].copy_(plan['host_chunks'], non_blocking=True)


def _moment_like(param):
  """Zeros of the parameter's shape that start at the parameter's address modulo
  16 bytes: a parameter that is a view at an odd element offset into a flat buffer
  then still takes the kernels' 16-byte accesses (csrc/optim.h: optim_plan)."""
  offset = (param.data_ptr() // 4) % 4
  flat = torch.zeros(param.numel() + offset, dtype=torch.float32, device=param.device)
  return flat[offset:].view(param.shape)


class _TableOptimizer(torch.optim.Optimizer):
  """What `LaProp` and `Adam` share: one parameter group of CUDA float32 tensors,
  the float32 moments `nu` and `mu` in `state[p]`, the update count in
  `param_groups[0]['updates']`, the schedule, the checks of a step's gradients,
  the device table of csrc/optim.h with its uploads, and the metrics.  A
  subclass has `_composed_step` and `_fused_step`."""

  def _setup(self, params, defaults, schedule, wd_mask, fused, moments):
    who = type(self).__name__
    self._schedule = schedule
    params = list(params)
    if any(isinstance(entry, dict) for entry in params):
      raise ValueError(f'{who}: one parameter group; pass the tensors themselves')
    for index, param in enumerate(params):
      _check_param(index, param)
    torch.optim.Optimizer.__init__(self, params, defaults)
    group = self.param_groups[0]['params']
    if wd_mask is None:
      wd_mask = [param.dim() >= 2 for param in group]
    wd_mask = [bool(flag) for flag in wd_mask]
    if len(wd_mask) != len(group):
      raise ValueError(f'{who}: wd_mask has {len(wd_mask)} entries for {len(group)} parameters')
    self.wd_mask = tuple(wd_mask)
    self.fused = _path(fused, group, who)
    self.param_count = sum(param.numel() for param in group)
    for param in group:
      self.state[param] = {name: _moment_like(param) for name in moments}
    self._plan = None               # the device tables, made by the first fused step
    self._sums = None               # the composed path's sums of squares of the last step
    self.table_uploads = 0          # how often the device table was (re)written
    self._stepped = False
    self._slow = None               # the attached SlowModel

  # ------------------------------------------------------------------ both paths

  def _hyper(self):
    """(group, lr of this update, 1 - beta1**t, 1 - beta2**t)."""
    group = self.param_groups[0]
    count = group['updates']
    if self._schedule is not None:
      lr = float(self._schedule(count))
    else:
      lr = warmup_schedule(group['lr'], group['warmup'])(count)
    t = count + 1                                      # optax.safe_int32_increment, opt.py:135, 155
    return group, lr, 1 - group['beta1'] ** t, 1 - group['beta2'] ** t

  def _gradients(self, group):
    who = type(self).__name__
    grads = []
    for index, param in enumerate(group['params']):
      grad = param.grad
      if grad is None:
        raise ValueError(f'{who}.step: parameter {index} has no gradient (the reference has one for every leaf, '
                         'and the norm of a missing tensor has no definition)')
      if grad.dtype not in _GRADS:
        raise TypeError(f'{who}.step: the gradient of parameter {index} must be float32 or bfloat16, got {grad.dtype}')
      if grad.shape != param.shape or grad.device != param.device:
        raise ValueError(f'{who}.step: the gradient of parameter {index} is {tuple(grad.shape)} on {grad.device}, '
                         f'the parameter {tuple(param.shape)} on {param.device}')
      grads.append(grad)
    return grads

  @torch.no_grad()
  def step(self, closure=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    group, lr, c1, c2 = self._hyper()
    grads = self._gradients(group)
    moments = [self.state[param] for param in group['params']]
    why = self._misfit(group['params'], grads, moments) if self.fused else 'composed'
    if self.fused and why:
      raise ValueError(f'{type(self).__name__}.step (fused): {why}')
    if self.fused:
      self._fused_step(group, grads, moments, lr, c1, c2)
    else:
      self._composed_step(group, grads, moments, lr, c1, c2)
    group['updates'] += 1
    self._stepped = True
    if self._slow is not None:
      self._slow.count += 1         # the update launch wrote the slow copy where it was due
    return loss

  def metrics(self):
    """opt.py:64-79 of the last `step()`: device float32 scalars `grad_norm`
    (optax.global_norm of the raw gradients), `grad_rms`, `update_rms` and
    `param_rms` (nets.rms of the raw gradients, of upd and of the parameters
    after the update), Python ints `updates` and `param_count`.  No host
    synchronisation; on the fused path one launch, issued here and only here."""
    if not self._stepped:
      raise RuntimeError(f'{type(self).__name__}.metrics: no step yet')
    if self.fused:
      plan = self._plan
      out = _lib.empty((4,), torch.float32, plan['device'])
      api.emb_optim_metrics(plan['partials'].data_ptr(), plan['n_chunks'], self.param_count, out.data_ptr(),
                            _lib.raw_stream(plan['device']))
      grad_norm, grad_rms, update_rms, param_rms = out.unbind(0)
    else:
      gsq, usq, psq = self._sums
      count = torch.tensor(float(self.param_count), dtype=torch.float32, device=gsq.device)
      grad_norm = torch.sqrt(gsq)                                          # opt.py:64
      grad_rms, update_rms, param_rms = (torch.sqrt(x / count) for x in (gsq, usq, psq))    # nets.py:123-124
    return {'grad_norm': grad_norm, 'grad_rms': grad_rms, 'update_rms': update_rms, 'param_rms': param_rms,
            'updates': self.param_groups[0]['updates'], 'param_count': self.param_count}

  # ------------------------------------------------------------------- the fused path

  @staticmethod
  def _misfit(params, grads, moments):
    """Why this step cannot run on the kernels, or None."""
    for index, (param, grad, state) in enumerate(zip(params, grads, moments)):
      nu, mu = state['nu'], state['mu']
      for name, tensor in (('parameter', param), ('gradient', grad), ('nu', nu), ('mu', mu)):
        if not tensor.is_contiguous():
          return f'the {name} of parameter {index} is not contiguous'
      if nu.dtype != torch.float32 or mu.dtype != torch.float32 or nu.shape != param.shape or mu.shape != param.shape:
        return f'the moments of parameter {index} are not float32 of the parameter\'s shape'
      if nu.device != param.device or mu.device != param.device or param.device != params[0].device:
        return f'parameter {index} and its moments are not on one device'
    return None

  def _make_plan(self, params, flags):
    device = params[0].device if params else torch.device('cuda')
    plan = _new_plan(device, [param.numel() for param in params], RECORD_BYTES)
    plan.update(partials=torch.zeros((4, max(plan['n_chunks'], 1)), dtype=torch.float32, device=device), flags=None,
                slow_addrs=None, slow=None)
    return plan

  def _refresh(self, params, addrs, flags, slow_addrs=None):
    """(Re)write the device table on the stream: the first step, and whenever an
    address or a gradient's dtype has changed (gradients come back elsewhere after
    zero_grad(set_to_none=True), moments after load_state_dict); with an attached
    `SlowModel`, the addresses of its tensors beside it."""
    flag_array = np.array(flags, np.int32)
    plan = self._plan
    first = plan is None
    if first:
      plan = self._plan = self._make_plan(params, flag_array)
    addr_array = np.array(addrs, np.int64)
    _upload(plan, first, lambda table, chunks, capacity, counted: api.emb_optim_table(
        addr_array.ctypes.data, plan['counts'].ctypes.data, flag_array.ctypes.data, len(params), table, chunks,
        capacity, counted, None, None))
    if slow_addrs is not None:
      staged = torch.tensor(slow_addrs or [0], dtype=torch.int64).pin_memory()
      plan['slow'] = staged.to(plan['device'], non_blocking=True)
    plan['addrs'], plan['flags'], plan['slow_addrs'] = addrs, flags, slow_addrs
    self.table_uploads += 1

  def _tables(self, group, grads, moments):
    """The plan with the table of this step's addresses on the device, uploaded
    only where one differs from the last step's."""
    params = group['params']
    wd = group['wd']
    addrs, flags = [], []
    for param, grad, state, decays in zip(params, grads, moments, self.wd_mask):
      addrs += (param.data_ptr(), grad.data_ptr(), state['nu'].data_ptr(), state['mu'].data_ptr())
      flags.append(_GRADS[grad.dtype] | (DECAY if wd and decays else 0))
    slow_addrs = None if self._slow is None else self._slow._addresses_for(params)
    plan = self._plan
    if plan is None or plan['addrs'] != addrs or plan['flags'] != flags or plan['slow_addrs'] != slow_addrs:
      self._refresh(params, addrs, flags, slow_addrs)
      plan = self._plan
    return plan

  def _slow_args(self, plan):
    """(slow, mix, omm) of the `_slow` entry points where the attached `SlowModel`
    is due on this step, else None: the plain entry point."""
    slow = self._slow
    if slow is None or slow.count % slow.every:
      return None
    return plan['slow'].data_ptr(), slow.mix, slow.omm


class LaProp(_TableOptimizer):
  """`LaProp(params, lr=4e-5, agc=0.3, pmin=1e-3, eps=1e-20, beta1=0.9,
  beta2=0.999, nesterov=False, wd=0.0, wd_mask=None, warmup=0, fused=None)`

  params    an iterable of CUDA float32 tensors, one parameter group
  lr        a float, or a callable `count -> float` evaluated on the host with
            count = the number of updates applied so far (the first sees 0, as
            optax.scale_by_schedule)
  warmup    with a float lr: lr * min(count / warmup, 1), so the very first update
            has step size 0 (agent.py:375-377); anneals go through the callable
  wd_mask   one bool per parameter; None decays tensors with dim() >= 2, the
            torch-side counterpart of the reference's r'/kernel$' (agent.py:352)
  fused     None: the kernels where they fit; True / False force a path, True
            raises where they do not fit and says why

  Gradients are float32 or bfloat16, widened to float32 in registers; the
  moments are float32 and live in `state[p]['nu']`, `state[p]['mu']`; the update
  count is `param_groups[0]['updates']`, so `state_dict` carries all of it.
  """

  def __init__(self, params, lr=4e-5, agc=0.3, pmin=1e-3, eps=1e-20, beta1=0.9, beta2=0.999, nesterov=False, wd=0.0,
               wd_mask=None, warmup=0, fused=None):
    schedule = _check_hyper('LaProp', dict(beta1=beta1, beta2=beta2), dict(agc=agc, pmin=pmin, eps=eps, wd=wd), lr,
                            warmup)
    defaults = dict(lr=None if callable(lr) else float(lr), agc=float(agc), pmin=float(pmin), eps=float(eps),
                    beta1=float(beta1), beta2=float(beta2), nesterov=bool(nesterov), wd=float(wd), warmup=int(warmup),
                    updates=0)
    self._setup(params, defaults, schedule, wd_mask, fused, ('nu', 'mu'))

  def _composed_step(self, group, grads, moments, lr, c1, c2):
    """The reference's chain restated line by line; the definition."""
    agc, pmin, eps, wd = group['agc'], group['pmin'], group['eps'], group['wd']
    beta1, beta2, nesterov = group['beta1'], group['beta2'], group['nesterov']
    gsq, usq, psq = [], [], []
    for param, grad, state, decays in zip(group['params'], grads, moments, self.wd_mask):
      nu, mu = state['nu'], state['mu']
      g = grad.to(torch.float32)
      gsq.append(torch.square(g).sum())
      if agc:                                                              # opt.py:120
        unorm = torch.sqrt(gsq[-1])                                        # opt.py:116, as jnp.linalg.norm does it:
        pnorm = torch.sqrt(torch.square(param).sum())                      # opt.py:117  sqrt(sum(x * x))
        upper = agc * torch.maximum(torch.full_like(pnorm, pmin), pnorm)   # opt.py:118
        g = g * (1 / torch.maximum(torch.ones_like(unorm), unorm / upper))  # opt.py:119
      nu.copy_(beta2 * nu + (1 - beta2) * (g * g))                         # opt.py:136-137
      u = g / (torch.sqrt(nu / c2) + eps)                                  # opt.py:138-140, optax.bias_correction
      mu.copy_((1 - beta1) * u + beta1 * mu)                               # opt.py:156, optax.update_moment
      m = (1 - beta1) * u + beta1 * mu if nesterov else mu                 # opt.py:157-161
      m = m / c1
      if wd and decays:                                                    # agent.py:361-365
        m = m + wd * param
      upd = m * -lr                                                        # agent.py:378, scale_by_learning_rate
      param.add_(upd)                                                      # opt.py:62, optax.apply_updates
      usq.append(torch.square(upd).sum())
      psq.append(torch.square(param).sum())
    self._sums = tuple(torch.stack(x).sum() for x in (gsq, usq, psq))      # nets.py:123

  def _fused_step(self, group, grads, moments, lr, c1, c2):
    plan = self._tables(group, grads, moments)
    if not plan['n_chunks']:
      return
    stream = _lib.raw_stream(plan['device'])
    table, chunks, partials = plan['table'].data_ptr(), plan['chunks'].data_ptr(), plan['partials'].data_ptr()
    beta1, beta2 = group['beta1'], group['beta2']
    api.emb_optim_norms(table, chunks, plan['n_chunks'], partials, stream)
    args = (table, chunks, plan['n_chunks'], partials, lr, beta1, 1 - beta1, c1, beta2, 1 - beta2, c2, group['eps'],
            group['agc'], group['pmin'], group['wd'], int(group['nesterov']))
    slow = self._slow_args(plan)
    if slow:
      api.emb_optim_update_slow(*args, *slow, stream)
    else:
      api.emb_optim_update(*args, stream)


class Adam(_TableOptimizer):
  """`Adam(params, lr=3e-4, clip=10.0, eps=1e-7, beta1=0.9, beta2=0.999, wd=0.0,
  wd_mask=None, warmup=1000, fused=None)`: the PPO learner's optimizer
  (ppo/agent.py:114-124 with the defaults of ppo/configs.yaml:101), in place of
  `nn.utils.clip_grad_norm_` followed by `torch.optim.Adam`.

  params    an iterable of CUDA float32 tensors, one parameter group
  lr        a float, or a callable `count -> float` evaluated on the host with
            count = the number of updates applied so far (the first sees 0); a
            callable is the whole schedule and goes with warmup=0
  clip      the bound on the global norm of all gradients; 0 switches it off
  warmup    with a float lr: lr * min(count / warmup, 1), optax.linear_schedule(0,
            lr, warmup): the very first update has step size 0
  wd_mask   one bool per parameter; None decays tensors with dim() >= 2, the
            torch-side counterpart of the reference's r'/kernel$'
  fused     None: the kernels where they fit; True / False force a path, True
            raises where they do not fit and says why

  The clip decision is one for all tensors, and it is a select on `gnorm < clip`:
  a NaN in any gradient makes p, mu and nu NaN in EVERY tensor, an infinity and
  no NaN gives g1 = 0 at the finite elements of every tensor and NaN at the
  infinite ones.  That is the reference's behaviour and differs on purpose from
  `LaProp`, whose clipping and whose NaN stay inside one tensor.

  Gradients are float32 or bfloat16, widened to float32 in registers; the
  moments are float32 and live in `state[p]['mu']`, `state[p]['nu']`; the update
  count is `param_groups[0]['updates']`, so `state_dict` carries all of it.
  `metrics()` is `LaProp.metrics()`: `grad_norm` is the norm of the raw gradients.
  """

  def __init__(self, params, lr=3e-4, clip=10.0, eps=1e-7, beta1=0.9, beta2=0.999, wd=0.0, wd_mask=None, warmup=1000,
               fused=None):
    schedule = _check_hyper('Adam', dict(beta1=beta1, beta2=beta2), dict(clip=clip, eps=eps, wd=wd), lr, warmup)
    defaults = dict(lr=None if callable(lr) else float(lr), clip=float(clip), eps=float(eps), beta1=float(beta1),
                    beta2=float(beta2), wd=float(wd), warmup=int(warmup), updates=0)
    self._setup(params, defaults, schedule, wd_mask, fused, ('mu', 'nu'))

  def _composed_step(self, group, grads, moments, lr, c1, c2):
    """The reference's chain restated line by line; the definition."""
    clip, eps, wd = group['clip'], group['eps'], group['wd']
    beta1, beta2 = group['beta1'], group['beta2']
    gs = [grad.to(torch.float32) for grad in grads]
    gsq = torch.stack([torch.square(g).sum() for g in gs]).sum()
    if clip:                                                               # optax.clip_by_global_norm
      gnorm = torch.sqrt(gsq)                                              # optax.global_norm
      trigger = gnorm < clip
      gs = [torch.where(trigger, g, (g / gnorm) * clip) for g in gs]
    usq, psq = [], []
    for param, g, state, decays in zip(group['params'], gs, moments, self.wd_mask):
      mu, nu = state['mu'], state['nu']
      mu.copy_(beta1 * mu + (1 - beta1) * g)                               # optax.scale_by_adam: update_moment
      nu.copy_(beta2 * nu + (1 - beta2) * (g * g))                         #   update_moment_per_elem_norm
      u = (mu / c1) / (torch.sqrt(nu / c2) + eps)                          #   bias_correction, eps_root = 0
      if wd and decays:                                                    # optax.add_decayed_weights
        u = u + wd * param
      upd = u * -lr                                                        # optax.scale_by_learning_rate
      param.add_(upd)                                                      # optax.apply_updates
      usq.append(torch.square(upd).sum())
      psq.append(torch.square(param).sum())
    self._sums = (gsq, torch.stack(usq).sum(), torch.stack(psq).sum())

  def _fused_step(self, group, grads, moments, lr, c1, c2):
    plan = self._tables(group, grads, moments)
    if not plan['n_chunks']:
      return
    stream = _lib.raw_stream(plan['device'])
    table, chunks, partials = plan['table'].data_ptr(), plan['chunks'].data_ptr(), plan['partials'].data_ptr()
    beta1, beta2 = group['beta1'], group['beta2']
    api.emb_optim_grad_norms(table, chunks, plan['n_chunks'], partials, stream)
    args = (table, chunks, plan['n_chunks'], partials, lr, beta1, 1 - beta1, c1, beta2, 1 - beta2, c2, group['eps'],
            group['clip'], group['wd'])
    slow = self._slow_args(plan)
    if slow:
      api.emb_optim_adam_update_slow(*args, *slow, stream)
    else:
      api.emb_optim_adam_update(*args, stream)


# ---------------------------------------------------------------- the slow model

def _slow_geometry():
  record = C.c_int64(0)
  api.emb_slow_table(None, None, 0, None, None, 0, None, C.byref(record))
  return record.value


SLOW_RECORD_BYTES = _slow_geometry()                  # csrc/optim.h: SlowTensor


def slow_mix(rate):
  """(mix, omm) as the reference forms them on a float32 scalar (utils.py:117-118):
  mix = float32(rate) and omm = float32(1) - mix, the subtraction in float32.  A
  double `1 - rate` rounded once can differ from that in the last bit."""
  mix = np.float32(rate)
  return mix, np.float32(1) - mix


def _named_tensors(who, thing):
  """(keys, tensors) of a module's `named_parameters()` or of a sequence of tensors."""
  if isinstance(thing, torch.nn.Module):
    named = dict(thing.named_parameters())
    return list(named), list(named.values())
  if torch.is_tensor(thing) or isinstance(thing, (str, bytes, dict)):
    raise TypeError(f'SlowModel: {who} is a {type(thing).__name__}, not a torch.nn.Module or a sequence of tensors')
  tensors = list(thing)
  return list(range(len(tensors))), tensors


# `SlowModel(fused=None)`: the kernel wherever it fits.  On the MI355X the median of
# `update()` is below the composed one at all four rows of
# profiles/slow_model_bench.txt -- the reference's value MLP at size1m 7.9 us
# against 160.4, at size200m 23.6 / 140.7, at size400m 50.8 / 171.1, 1 M parameters
# in 40 tensors 13.2 / 607.9 -- so there is no crossover constant here either.


class SlowModel:
  """`SlowModel(model, source, rate=1.0, every=1, fused=None)`: the reference's
  slowly updated copy of a network (embodied/jax/utils.py:94-127), DreamerV3's
  `slowval` (dreamerv3/agent.py:142; its `pred()` is the `slow_pred` of
  `TwoHot.loss_sum`, `dreamer_targets` and `imag_metrics`).

  model, source   two `torch.nn.Module`s whose `named_parameters()` have the same
                  keys and shapes, or two sequences of tensors of equal length;
                  CUDA float32 throughout.  Construction copies source into model
                  (the reference's `_initonce`); that is no update.
  rate            1, or 0 <= rate < 0.5 (utils.py:97)
  every           a whole number of updates, 1 or more
  fused           None: the kernel where it fits; True / False force a path, True
                  raises where it does not fit and says why

  `update()`, on the calls where `count % every == 0` (count starts at 0), per
  element and in float32, two rounded products and one rounded sum:

      dst = mix * src + omm * dst       mix = float32(rate), omm = float32(1) - mix

  in ONE launch for all tensors (csrc/optim.hip: slow_update_kernel); the composed
  path, the definition, is `dst.mul_(omm).add_(src * mix)` per tensor.  Then
  `count += 1`.  Calls and attribute access go to `model`.

  `attach(optimizer)` folds the update into a fused `LaProp` or `Adam` whose
  parameters include every source tensor: from then on `optimizer.step()` writes
  the slow copy from the new parameter it holds in registers, in the update launch
  it issues anyway, and advances `count`; `update()` raises, `detach()` undoes it.

  Different from the reference, on purpose:
  * An off-step (`count % every != 0`) touches nothing.  The reference computes
    `0 * src + 1 * dst`, which turns a non-finite source element into a NaN in the
    copy.  On an update step the expression is evaluated as written: a NaN or an
    infinity behaves as in the reference and stays inside its element.
  * `count` is a Python int on the host.  Under graph capture an `update()` replays
    the decision taken at capture time: right for `every == 1`, unsupported otherwise.
  """

  def __init__(self, model, source, rate=1.0, every=1, fused=None):
    self.model = model
    self.source = source
    self._set_schedule(rate, every)
    keys, dst = _named_tensors('model', model)
    source_keys, src = _named_tensors('source', source)
    if set(keys) != set(source_keys) or len(keys) != len(source_keys):
      raise ValueError(f'SlowModel: model and source differ in their parameters: {sorted(map(str, set(keys) ^ set(source_keys)))[:4]} '
                       f'({len(keys)} against {len(source_keys)})')
    order = {key: i for i, key in enumerate(keys)}
    dst = [dst[order[key]] for key in source_keys]                 # in the source's order
    for index, (d, s) in enumerate(zip(dst, src)):
      _check_param(index, s)
      _check_param(index, d)
      if d.shape != s.shape:
        raise ValueError(f'SlowModel: parameter {index} ({source_keys[index]!r}) is {tuple(d.shape)} in model and '
                         f'{tuple(s.shape)} in source')
      if d.device != src[0].device or s.device != src[0].device:
        raise ValueError(f'SlowModel: parameter {index} ({source_keys[index]!r}) is not on {src[0].device}')
      if d is s or (d.numel() and d.data_ptr() == s.data_ptr()):
        raise ValueError(f'SlowModel: parameter {index} ({source_keys[index]!r}) of model IS the source\'s tensor')
    self._dst, self._src = dst, src
    self.fused = _path(fused, dst + src, 'SlowModel')
    self.count = 0
    self.table_uploads = 0            # how often the device table was (re)written
    self._plan = None
    self._attached = None
    with torch.no_grad():             # utils.py:121-124, _initonce
      for d, s in zip(dst, src):
        d.copy_(s)

  def _set_schedule(self, rate, every):
    rate = float(rate)
    if not (rate == 1.0 or 0.0 <= rate < 0.5):
      raise ValueError(f'SlowModel: rate = {rate!r} must be 1 or in [0, 0.5)')
    if isinstance(every, bool) or int(every) != every or every < 1:
      raise ValueError(f'SlowModel: every = {every!r} must be a whole number of updates, 1 or more')
    self.rate, self.every = rate, int(every)
    mix, omm = slow_mix(rate)
    self.mix, self.omm = float(mix), float(omm)       # float32 values, exact as Python floats

  def __getattr__(self, name):                        # only what the instance itself does not have
    if name.startswith('__') or name in ('model', 'source'):
      raise AttributeError(name)
    return getattr(self.model, name)

  def __call__(self, *args, **kwargs):
    return self.model(*args, **kwargs)

  # ------------------------------------------------------------------- stand-alone

  @torch.no_grad()
  def update(self):
    if self._attached is not None:
      raise RuntimeError('SlowModel.update: attached to an optimizer, whose step() has done it (detach() first)')
    if self.count % self.every == 0:
      if self.fused:
        self._fused_update()
      else:
        for d, s in zip(self._dst, self._src):        # utils.py:118, the definition
          d.mul_(self.omm).add_(s * self.mix)
    self.count += 1

  def _fused_update(self):
    addrs = []
    for index, (d, s) in enumerate(zip(self._dst, self._src)):
      if not (d.is_contiguous() and s.is_contiguous()):
        raise ValueError(f'SlowModel.update (fused): parameter {index} is not contiguous')
      addrs += (d.data_ptr(), s.data_ptr())
    plan = self._plan
    if plan is None or plan['addrs'] != addrs:
      first = plan is None
      if first:
        device = self._src[0].device if self._src else torch.device('cuda')
        plan = self._plan = _new_plan(device, [s.numel() for s in self._src], SLOW_RECORD_BYTES)
      addr_array = np.array(addrs, np.int64)
      _upload(plan, first, lambda table, chunks, capacity, counted: api.emb_slow_table(
          addr_array.ctypes.data, plan['counts'].ctypes.data, len(self._src), table, chunks, capacity, counted, None))
      plan['addrs'] = addrs
      self.table_uploads += 1
    if plan['n_chunks']:
      api.emb_slow_update(plan['table'].data_ptr(), plan['chunks'].data_ptr(), plan['n_chunks'], self.mix, self.omm,
                          _lib.raw_stream(plan['device']))

  # ------------------------------------------------------- inside an optimizer's step

  def attach(self, optimizer):
    """Have `optimizer.step()` write the slow copy in its update launch."""
    if self._attached is not None:
      raise RuntimeError('SlowModel.attach: already attached (detach() first)')
    if not isinstance(optimizer, _TableOptimizer) or not optimizer.fused:
      raise TypeError('SlowModel.attach: a fused embodied_amd.optim.LaProp or Adam, the composed path has no launch '
                      'to fold the update into')
    if optimizer._slow is not None:
      raise RuntimeError('SlowModel.attach: the optimizer already has a SlowModel, one per optimizer')
    params = optimizer.param_groups[0]['params']
    where = {id(param): i for i, param in enumerate(params)}
    taken = {param.data_ptr() for param in params if param.numel()}
    slots = []
    for index, (d, s) in enumerate(zip(self._dst, self._src)):
      if id(s) not in where:
        raise ValueError(f'SlowModel.attach: source tensor {index} of shape {tuple(s.shape)} is not a parameter of the '
                         'optimizer')
      if d.numel() and d.data_ptr() in taken:
        raise ValueError(f'SlowModel.attach: model tensor {index} is a parameter of the optimizer')
      if d.device != params[0].device:
        raise ValueError(f'SlowModel.attach: model tensor {index} is not on the optimizer\'s device')
      slots.append(where[id(s)])
    self._slots = slots
    self._attached = optimizer
    optimizer._slow = self

  def detach(self):
    if self._attached is None:
      raise RuntimeError('SlowModel.detach: not attached')
    self._attached._slow = None
    self._attached = None

  def _addresses_for(self, params):
    """One address per parameter of the optimizer: its slow copy, 0 for none."""
    out = [0] * len(params)
    for index, (slot, d, s) in enumerate(zip(self._slots, self._dst, self._src)):
      if params[slot] is not s:
        raise ValueError(f'SlowModel: source tensor {index} is no longer parameter {slot} of the optimizer')
      if not d.is_contiguous():
        raise ValueError(f'SlowModel (attached): model tensor {index} is not contiguous')
      out[slot] = d.data_ptr() if d.numel() else 0
    return out

  # --------------------------------------------------------------------------- state

  def state_dict(self):
    return {'count': self.count, 'rate': self.rate, 'every': self.every}

  def load_state_dict(self, state):
    self._set_schedule(state['rate'], state['every'])
    self.count = int(state['count'])
