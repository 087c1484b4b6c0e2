"""The reference learners' optimizer (embodied/jax/opt.py:109-164 chained by
dreamerv3/agent.py:342-379) as a `torch.optim.Optimizer` over CUDA tensors:
adaptive gradient clipping per tensor, RMS scaling, bias-corrected momentum,
optional weight decay and a learning-rate schedule, in two HIP launches per
`step()` whatever the number of parameter tensors.

Per tensor, in float32, `t` the number of this update counted from 1 (`eps` is
not inside the root):

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

Two paths, as the heads in `outs.py`: the composed one restates the reference
line by line in torch ops and is the definition; the fused one is csrc/optim.hip.
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

# `fused=None`: the kernels wherever they fit.  On the MI355X the fused median is
# below the composed one at all six rows of profiles/optim_bench.txt -- 1 M
# parameters in 40 tensors 72.2 us against 6572.8 (bf16 gradients 74.8 / 6917.9),
# the 12.2 M PPO model 81.8 / 7532.0 (80.4 / 7750.6), the 166 M DreamerV3 model
# 1050.5 / 15853.6 (941.7 / 17519.4) -- so there is no size below which the
# composed path is taken and no crossover constant here.


def optimizer_launches():
  """Kernel launches `emb_optim_norms`, `emb_optim_update` and `emb_optim_metrics`
  have issued in this process."""
  return _lib.launches('optim')


def warmup_schedule(lr, warmup):
  """`count -> lr * min(count / warmup, 1)`: the reference's default schedule,
  join_schedules([linear_schedule(0, lr, warmup), constant_schedule(lr)],
  [warmup]) of agent.py:367-378.  warmup == 0: the constant."""
  lr, warmup = float(lr), int(warmup)
  if not warmup:
    return lambda count: lr
  return lambda count: lr * min(count / warmup, 1.0)


def _check_param(index, param):
  """A parameter the optimizer takes: a CUDA float32 tensor."""
  if not torch.is_tensor(param):
    raise TypeError(f'LaProp: parameter {index} is a {type(param).__name__}, not a tensor')
  if param.dtype != torch.float32:
    raise TypeError(f'LaProp: parameter {index} must be float32, got {param.dtype} (no CPU fallback, no other dtype)')
  if not param.is_cuda:
    raise RuntimeError(f'embodied_amd.optim runs as HIP kernels: parameter {index} is not a CUDA tensor '
                       '(no CPU fallback)')


def _path(fused, params):
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
    raise ValueError(f'LaProp(fused=True): {why} (fused=None or False composes it)')
  if fused is None:
    return why is None
  return bool(fused)


def _moment_like(param):
  """Zeros of the parameter's shape that start at the parameter's address modulo
  16 bytes: a parameter that is a view at an odd element offset into a flat buffer
  then still takes the kernels' 16-byte accesses (csrc/optim.h: optim_plan)."""
  offset = (param.data_ptr() // 4) % 4
  flat = torch.zeros(param.numel() + offset, dtype=torch.float32, device=param.device)
  return flat[offset:].view(param.shape)


class LaProp(torch.optim.Optimizer):
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
    for name, value in (('beta1', beta1), ('beta2', beta2)):
      if not 0.0 <= value < 1.0:
        raise ValueError(f'LaProp: {name} = {value!r} is outside [0, 1)')
    for name, value in (('agc', agc), ('pmin', pmin), ('eps', eps), ('wd', wd)):
      if not (value >= 0.0 and np.isfinite(value)):
        raise ValueError(f'LaProp: {name} = {value!r} must be finite and not negative')
    if int(warmup) != warmup or warmup < 0:
      raise ValueError(f'LaProp: warmup = {warmup!r} must be a whole number of updates, 0 or more')
    if callable(lr):
      if warmup:
        raise ValueError('LaProp: warmup goes with a float lr; a callable lr is the whole schedule')
      self._schedule = lr
    else:
      if not np.isfinite(lr):
        raise ValueError(f'LaProp: lr = {lr!r} must be finite')
      self._schedule = None
    defaults = dict(lr=None if callable(lr) else float(lr), agc=float(agc), pmin=float(pmin), eps=float(eps),
                    beta1=float(beta1), beta2=float(beta2), nesterov=bool(nesterov), wd=float(wd), warmup=int(warmup),
                    updates=0)
    params = list(params)
    if any(isinstance(entry, dict) for entry in params):
      raise ValueError('LaProp: one parameter group; pass the tensors themselves')
    for index, param in enumerate(params):
      _check_param(index, param)
    super().__init__(params, defaults)
    group = self.param_groups[0]['params']
    if wd_mask is None:
      wd_mask = [param.dim() >= 2 for param in group]
    wd_mask = [bool(flag) for flag in wd_mask]
    if len(wd_mask) != len(group):
      raise ValueError(f'LaProp: wd_mask has {len(wd_mask)} entries for {len(group)} parameters')
    self.wd_mask = tuple(wd_mask)
    self.fused = _path(fused, group)
    self.param_count = sum(param.numel() for param in group)
    for param in group:
      self.state[param] = {'nu': _moment_like(param), 'mu': _moment_like(param)}
    self._plan = None               # the device tables, made by the first fused step
    self._sums = None               # the composed path's sums of squares of the last step
    self.table_uploads = 0          # how often the device table was (re)written
    self._stepped = False

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
    grads = []
    for index, param in enumerate(group['params']):
      grad = param.grad
      if grad is None:
        raise ValueError(f'LaProp.step: parameter {index} has no gradient (the reference has one for every leaf, '
                         'and AGC of a missing tensor has no definition)')
      if grad.dtype not in _GRADS:
        raise TypeError(f'LaProp.step: the gradient of parameter {index} must be float32 or bfloat16, got {grad.dtype}')
      if grad.shape != param.shape or grad.device != param.device:
        raise ValueError(f'LaProp.step: the gradient of parameter {index} is {tuple(grad.shape)} on {grad.device}, '
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
      raise ValueError(f'LaProp.step (fused): {why}')
    if self.fused:
      self._fused_step(group, grads, moments, lr, c1, c2)
    else:
      self._composed_step(group, grads, moments, lr, c1, c2)
    group['updates'] += 1
    self._stepped = True
    return loss

  def metrics(self):
    """opt.py:64-79 of the last `step()`: device float32 scalars `grad_norm`
    (optax.global_norm of the raw gradients), `grad_rms`, `update_rms` and
    `param_rms` (nets.rms of the raw gradients, of upd and of the parameters
    after the update), Python ints `updates` and `param_count`.  No host
    synchronisation; on the fused path one launch, issued here and only here."""
    if not self._stepped:
      raise RuntimeError('LaProp.metrics: no step yet')
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

  # ---------------------------------------------------------------- the composed path

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
    counts = np.array([param.numel() for param in params], np.int64)
    n_chunks = int(sum(-(-int(n) // CHUNK) for n in counts))
    chunks = torch.empty(max(n_chunks, 1) * 8, dtype=torch.uint8).pin_memory()
    table = torch.empty(max(len(params), 1) * RECORD_BYTES, dtype=torch.uint8).pin_memory()
    plan = {'device': device, 'counts': counts, 'n_chunks': n_chunks, 'host_table': table,
            'table': torch.empty(table.numel(), dtype=torch.uint8, device=device),
            'chunks': torch.empty(chunks.numel(), dtype=torch.uint8, device=device),
            'partials': torch.zeros((4, max(n_chunks, 1)), dtype=torch.float32, device=device),
            'addrs': None, 'flags': None, 'host_chunks': chunks}
    return plan

  def _refresh(self, params, addrs, flags):
    """(Re)write the device table on the stream: the first step, and whenever an
    address or a gradient's dtype has changed (gradients come back elsewhere after
    zero_grad(set_to_none=True), moments after load_state_dict)."""
    flag_array = np.array(flags, np.int32)
    plan = self._plan
    first = plan is None
    if first:
      plan = self._plan = self._make_plan(params, flag_array)
    else:
      # the pinned staging buffer of the previous upload may still be in flight: a
      # new one (the host allocator keeps the old block until its copy is done)
      plan['host_table'] = torch.empty_like(plan['host_table']).pin_memory()
    addr_array = np.array(addrs, np.int64)
    counted = C.c_int64(-1)
    api.emb_optim_table(addr_array.ctypes.data, plan['counts'].ctypes.data, flag_array.ctypes.data, len(params),
                        plan['host_table'].data_ptr(), plan['host_chunks'].data_ptr() if first else None,
                        plan['n_chunks'], C.byref(counted), None, None)
    assert counted.value == plan['n_chunks'], (counted.value, plan['n_chunks'])
    plan['table'].copy_(plan['host_table'], non_blocking=True)
    if first:
      plan['chunks'].copy_(plan['host_chunks'], non_blocking=True)
    plan['addrs'], plan['flags'] = addrs, flags
    self.table_uploads += 1

  def _fused_step(self, group, grads, moments, lr, c1, c2):
    params = group['params']
    wd = group['wd']
    addrs, flags = [], []
    for param, grad, state, decays in zip(params, grads, moments, self.wd_mask):
      addrs += (param.data_ptr(), grad.data_ptr(), state['nu'].data_ptr(), state['mu'].data_ptr())
      flags.append(_GRADS[grad.dtype] | (DECAY if wd and decays else 0))
    plan = self._plan
    if plan is None or plan['addrs'] != addrs or plan['flags'] != flags:
      self._refresh(params, addrs, flags)
      plan = self._plan
    if not plan['n_chunks']:
      return
    stream = _lib.raw_stream(plan['device'])
    table, chunks, partials = plan['table'].data_ptr(), plan['chunks'].data_ptr(), plan['partials'].data_ptr()
    beta1, beta2 = group['beta1'], group['beta2']
    api.emb_optim_norms(table, chunks, plan['n_chunks'], partials, stream)
    api.emb_optim_update(table, chunks, plan['n_chunks'], partials, lr, beta1, 1 - beta1, c1, beta2, 1 - beta2, c2,
                         group['eps'], group['agc'], group['pmin'], wd, int(group['nesterov']), stream)
