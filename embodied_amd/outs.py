"""Output heads on device: the `symexp_twohot` head of DreamerV3's reward and
value networks (embodied/jax/heads.py:132-144, embodied/jax/outs.py:273-330),
the one-hot latents' KL pair of its world model (`OneHot`, `rssm_kl`:
dreamerv3/rssm.py:123-132, embodied/jax/outs.py:40-76, 208-263), the
actor's discrete policy head and loss (`Categorical`, `policy_loss`:
dreamerv3/agent.py:411-415, embodied/jax/outs.py:208-240), the draw of
both (`OneHot.sample` / `pred`, `Categorical.sample`: dreamerv3/rssm.py:87, 100,
dreamerv3/agent.py:18, 126, 192, embodied/jax/outs.py:219-224, 248-254, 265-270),
the reconstruction heads (`MSE`, `ImageMSE`, `Binary`), and the actor's
continuous policy head, its loss and its draw (`Normal`, `normal_policy_loss`:
embodied/jax/heads.py:146-162, embodied/jax/outs.py:161-186).

It sits on both sides of `scans.dreamer_targets`: that function's `pred`
argument is `value.pred()` / `slowvalue.pred()` and its `tar_padded` result goes
into `value.loss(...)` (dreamerv3/agent.py:398-399, 420-422, 461-462, 471-473).

Logits are torch CUDA tensors, float32 or bfloat16; the arithmetic is float32.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import address as _address, api

# What the kernels take: a row of at most 1024 bins stays in one wave's
# registers, indices are 32-bit.  Structural, not a crossover: the fused median
# is below the composed one at every shape and piece of profiles/twohot_bench.txt
# -- (16384, 255) f32: pred 16.2 us against 65.8, loss_sum of two targets 27.3
# against 477.1, backward 44.9 against 95.2; (1008, 255): 15.5 / 52.7, 27.7 /
# 411.1, 42.0 / 120.8 -- so no size constant sits beside `_path`.  (The backward
# rows at 16 384 rows have rounds that overlap; the file says how they were timed.)
TWOHOT_MAX_BINS = 1024
TWOHOT_MAX_LOGITS = 2 ** 31 - 1
TWOHOT_MAX_TARGETS = 4

_DTYPES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def symexp_twohot_bins(n=255):
  """The bins of `Head.symexp_twohot` (heads.py:136-143) as a float32 numpy
  array: symexp of `linspace(-20, 0)` and its mirror image, with one middle bin
  (exactly 0) for odd `n` and the two middle bins 0.0, -0.0 for even `n`.  Built on the host."""
  n = int(n)
  if n < 1:
    raise ValueError(f'symexp_twohot_bins: n = {n}, needs at least one bin')
  symexp = lambda x: np.sign(x) * np.expm1(np.abs(x))      # nets.py:63-64
  if n % 2 == 1:
    half = symexp(np.linspace(-20, 0, (n - 1) // 2 + 1, dtype=np.float32))
    bins = np.concatenate([half, -half[:-1][::-1]], 0)
  else:
    half = symexp(np.linspace(-20, 0, n // 2, dtype=np.float32))
    bins = np.concatenate([half, -half[::-1]], 0)
  assert bins.dtype == np.float32 and bins.shape == (n,)
  return bins


def twohot_launches():
  """Kernel launches `emb_twohot_stats`, `emb_twohot_loss` and `emb_twohot_grad`
  have issued in this process."""
  return _lib.launches('twohot')


def _check_device(logits):
  if not (torch.is_tensor(logits) and logits.is_cuda):
    raise RuntimeError('embodied_amd.outs runs as HIP kernels: pass CUDA tensors (no CPU fallback)')


def _cuda_device(device):
  """`device` (None: the current CUDA device) as a torch.device, which must be a CUDA one."""
  device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
  if device.type != 'cuda':
    raise RuntimeError('embodied_amd.outs runs as HIP kernels: pass a CUDA device (no CPU fallback)')
  return device


def _fused_path(head, fused, *limits):
  """The decision every head and net makes between its two paths.  True: the
  kernels, False: the composed path.  `limits` is what the kernels take, in the
  order it is checked, as (holds, wording).  `fused=None` takes the kernels
  wherever every limit holds -- each family's kernels were below its composed
  path at every shape measured; the figures stand beside its `*_MAX_*` constants
  or its `_xxx_path` -- and any other value forces a path by its truth; forcing
  the kernels past a limit raises the wording of the first that fails.

  Where everything holds -- every call of a training step -- the `_xxx_path`
  functions answer `fused is None or bool(fused)` themselves and do not come
  here: a decision is part of the host's enqueue, which is all a small fused
  call costs, and the wordings are only worth making for a refusal."""
  fits = True
  for holds, wording in limits:
    if not holds:
      if fused:
        raise ValueError(f'{head}(fused=True): {wording} (fused=None or False composes it)')
      fits = False
  return fits if fused is None else bool(fused)


def _host_bins(bins, n):
  """`bins` as a checked float32 numpy array of `n` finite values, none below
  the one before it.  (Not "strictly increasing": the reference's own bins for an
  even n hold 0.0 and -0.0 side by side, heads.py:141-143, and its counts
  `bins <= t`, `bins > t` -- the kernels' too -- are well defined with ties.)"""
  if torch.is_tensor(bins):
    bins = bins.detach().cpu().numpy()
  bins = np.asarray(bins)
  if bins.dtype != np.float32:
    raise ValueError(f'TwoHot: bins must be float32 (outs.py:278), got {bins.dtype}')
  if bins.ndim != 1 or len(bins) != n:
    raise ValueError(f'TwoHot: {n} logits per row need {n} bins, got shape {bins.shape}')
  if n < 1 or not np.all(np.isfinite(bins)) or not np.all(bins[1:] >= bins[:-1]):
    raise ValueError('TwoHot: bins must be finite and increasing (equal neighbours are allowed)')
  return np.ascontiguousarray(bins)


_BINS = {}


def _device_bins(host, device):
  """The bins on `device`: uploaded once per (bins, device)."""
  key = (host.tobytes(), device)
  tensor = _BINS.get(key)
  if tensor is None:
    if len(_BINS) > 64:
      _BINS.clear()
    tensor = _BINS[key] = torch.from_numpy(host.copy()).to(device)
  return tensor


def _path(fused, n, rows):
  """True: the kernels, False: the composed path (`TwoHot` says when).  The
  kernels' median was below the composed path's at every shape and piece measured
  (profiles/twohot_bench.txt), so `fused=None` takes them wherever they fit."""
  row, index = n <= TWOHOT_MAX_BINS, rows * n <= TWOHOT_MAX_LOGITS
  if row and index:
    return fused is None or bool(fused)
  return _fused_path(
      'TwoHot', fused,
      (row, f'{n} bins, the kernels keep a row of at most {TWOHOT_MAX_BINS} in one wave\'s registers'),
      (index, f'{rows} x {n} logits, the kernels index at most 2^31 - 1'))


def _check_sum(targets, coefs):
  """The (targets, coefs) of `loss_sum` as two tuples; refuses what the launch does not take."""
  targets, coefs = tuple(targets), tuple(float(c) for c in coefs)
  if len(targets) != len(coefs):
    raise ValueError(f'TwoHot.loss_sum: {len(targets)} targets and {len(coefs)} coefs')
  if not 1 <= len(targets) <= TWOHOT_MAX_TARGETS:
    raise ValueError(
        f'TwoHot.loss_sum: {len(targets)} targets, one launch takes 1 .. {TWOHOT_MAX_TARGETS} '
        '(add the results of several calls)')
  return targets, coefs


def _twohot(bins, target):
  """outs.py:313-327: the two-hot encoding (..., n) of `target` (...)."""
  n = len(bins)
  t = target[..., None]
  below = (bins <= t).to(torch.int32).sum(-1) - 1
  above = n - (bins > t).to(torch.int32).sum(-1)
  below = torch.clip(below, 0, n - 1)
  above = torch.clip(above, 0, n - 1)
  equal = below == above
  one = torch.ones((), dtype=torch.float32, device=target.device)
  dist_to_below = torch.where(equal, one, torch.abs(bins[below] - target))
  dist_to_above = torch.where(equal, one, torch.abs(bins[above] - target))
  total = dist_to_below + dist_to_above
  weight_below = dist_to_above / total
  weight_above = dist_to_below / total
  one_hot = torch.nn.functional.one_hot
  return (one_hot(below, n).to(torch.float32) * weight_below[..., None] +
          one_hot(above, n).to(torch.float32) * weight_above[..., None])


class _FusedLoss(torch.autograd.Function):
  """`loss_sum` on the kernels: one launch forward, one launch backward."""

  @staticmethod
  def forward(ctx, logits, head, targets, coefs):
    lse, _ = head._stats()
    rows, n = head._x.shape
    loss = _lib.empty((rows,), torch.float32, logits.device)
    ctx.head = head
    ctx.args = ((C.c_void_p * len(targets))(*[t.data_ptr() for t in targets]),
                (C.c_float * len(coefs))(*coefs), len(targets))
    ctx.targets = targets                   # keeps the memory behind the addresses
    api.emb_twohot_loss(
        head._x.data_ptr(), head._dtype, rows, n, head._bins.data_ptr(), lse.data_ptr(), *ctx.args,
        loss.data_ptr(), _lib.raw_stream(logits.device))
    return loss.view(head._lead)

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    head = ctx.head
    x = head._x
    rows, n = x.shape
    gout = gout.to(torch.float32).expand(head._lead).contiguous()
    grad = torch.empty_like(x)
    api.emb_twohot_grad(
        x.data_ptr(), head._dtype, rows, n, head._bins.data_ptr(), head._lse.data_ptr(), *ctx.args,
        gout.data_ptr(), grad.data_ptr(), _lib.raw_stream(x.device))
    return grad.view(head._shape), None, None, None


class TwoHot:
  """The reference's `TwoHot` output (outs.py:273-330) over `logits` (..., n), a
  CUDA tensor of float32 or bfloat16, and `bins`, a float32 numpy array or tensor
  of n increasing values (`symexp_twohot_bins`; equal neighbours are allowed).  The reference computes
  in float32 (outs.py:276) and so does this: bfloat16 logits are widened in
  registers, the gradient comes back in bfloat16.

  `bins` is checked on the host (ValueError) and uploaded once per (bins,
  device); a device tensor is copied back for that check, so pass the numpy
  array.  Logits that are not contiguous are made contiguous with one torch op.

  Two paths compute it:
    composed  torch ops restating the reference line by line: every n.  The
              definition; about a dozen passes over the logits.
    fused     `emb_twohot_stats` (one pass: the rows' log-sum-exp and `pred`,
              kept for the object's life), `emb_twohot_loss` (two logits per row
              and target) and `emb_twohot_grad` (one read, one write): n <= 1024.
  `fused=None` takes the kernels where they fit, True / False force a path (True
  raises where they do not fit, and says why).  No rows: the composed path,
  nothing is launched.

  Non-finite logits: a NaN or +inf logit, or a row of -inf, makes that row's
  `pred`, loss and gradient NaN on both paths, and no other row's.  One -inf
  logit is a bin of probability 0; `pred` and the gradient stay finite.  Its
  LOSS differs between the paths: composed is the definition, the product with
  the two-hot target over the whole row, NaN (0 * -inf) unless the -inf bin
  carries weight (then +inf); fused reads the two logits at `below` and `above`
  alone, so a -inf logit in any other bin is not seen and the loss is finite.
  DESIGN.md says why that stands."""

  def __init__(self, logits, bins, fused=None):
    n = logits.shape[-1] if torch.is_tensor(logits) and logits.dim() else np.shape(logits)[-1]
    host = _host_bins(bins, n)
    _check_device(logits)
    if logits.dtype not in _DTYPES:
      raise TypeError(f'TwoHot: logits must be float32 or bfloat16, got {logits.dtype}')
    self.logits = logits
    self._shape = logits.shape
    self._lead = logits.shape[:-1]
    rows = int(np.prod(self._lead, dtype=np.int64))
    self.fused = _path(fused, n, rows) and rows > 0
    self._dtype = _DTYPES[logits.dtype]
    self._bins = _device_bins(host, logits.device)
    self._x = logits.detach().contiguous().view(rows, n)
    self._lse = self._pred = None

  def _stats(self):
    """(lse, pred) of every row: one launch, the first time either is needed."""
    if self._lse is None:
      rows, n = self._x.shape
      lse, pred = _lib.empty((2, rows), torch.float32, self._x.device).unbind(0)
      api.emb_twohot_stats(
          self._x.data_ptr(), self._dtype, rows, n, self._bins.data_ptr(), lse.data_ptr(), pred.data_ptr(),
          _lib.raw_stream(self._x.device))
      self._lse, self._pred = lse, pred
    return self._lse, self._pred

  def pred(self):
    """(...) float32: the symmetric weighted average of outs.py:285-309 -- every
    mirrored pair p[i] * b[i] + p[n-1-i] * b[n-1-i] is formed before any other
    addition, so uniform logits over antisymmetric bins give exactly 0.0.

    Carries no gradient: every use of `.pred()` in dreamerv3/agent.py reaches a
    loss only under `sg` (the lambda-return's bootstrap, the slow regulariser's
    target, the metrics).  A second call returns the kept result."""
    if self.fused:
      return self._stats()[1].view(self._lead)
    if self._pred is None:
      with torch.no_grad():
        bins, n = self._bins, self._x.shape[-1]
        probs = torch.softmax(self._x.to(torch.float32), -1)
        if n % 2 == 1:
          m = (n - 1) // 2
          p1, p2, p3 = probs[..., :m], probs[..., m: m + 1], probs[..., m + 1:]
          b1, b2, b3 = bins[:m], bins[m: m + 1], bins[m + 1:]
          wavg = (p2 * b2).sum(-1) + ((p1 * b1).flip(-1) + (p3 * b3)).sum(-1)
        else:
          p1, p2 = probs[..., :n // 2], probs[..., n // 2:]
          b1, b2 = bins[:n // 2], bins[n // 2:]
          wavg = ((p1 * b1).flip(-1) + (p2 * b2)).sum(-1)
        self._pred = wavg
    return self._pred.view(self._lead)

  def _target(self, target):
    if not torch.is_tensor(target):
      target = torch.as_tensor(np.asarray(target, np.float32))
    target = target.detach().to(device=self.logits.device, dtype=torch.float32)
    if target.shape != self._lead:
      raise ValueError(f'TwoHot.loss: target of shape {tuple(target.shape)}, the logits need {tuple(self._lead)}')
    return target.contiguous()

  def loss(self, target):
    """(...) float32: outs.py:311-330, the cross entropy against the two-hot
    encoding of `target` (...) float32.  Differentiable with respect to the
    logits (once); the target is a constant, as under the reference's `sg`.
    A NaN target gives a NaN loss; a target beyond an outer bin lands on it."""
    return self.loss_sum((target,), (1.0,))

  def loss_sum(self, targets, coefs):
    """sum_k coefs[k] * loss(targets[k]) for 1 .. 4 targets, the terms added in
    the order given -- `value.loss(tar_padded) + slowreg * value.loss(slowvalue.pred())`
    (agent.py:420-422) is `loss_sum((tar_padded, slow), (1.0, slowreg))`.  On the
    kernels that is ONE launch forward and ONE backward whatever the count."""
    targets, coefs = _check_sum(targets, coefs)
    targets = tuple(self._target(t) for t in targets)
    if self.fused:
      return _FusedLoss.apply(self.logits, self, targets, coefs)
    logits = self.logits.to(torch.float32)
    # logits - logsumexp(logits) as one op, whose backward makes a row with a
    # +inf logit NaN throughout, as the closed form and the kernel do (the
    # subtraction's backward leaves a single NaN in it)
    log_pred = torch.log_softmax(logits, -1)
    total = None
    for target, coef in zip(targets, coefs):
      with torch.no_grad():
        twohot = _twohot(self._bins, target)
      term = coef * -(twohot * log_pred).sum(-1)
      total = term if total is None else total + term
    return total


# ---- OneHot: the RSSM's latent distribution, its KL pair and entropies ------

# What the kernels take: a group of at most 256 classes stays in one wave's
# registers, indices are 32-bit.  Structural, not a crossover: the fused median
# is below the composed one at all 24 rows of profiles/rssm_kl_bench.txt (rows
# 1024 and 16 384, (32, 32), (32, 64), (32, 96), float32 and bfloat16, forward and
# forward + backward) -- (16384, 32, 64) bf16: forward 261.1 us against 3926.7,
# forward + backward 518.5 against 5085.3; (1024, 32, 32) f32: 24.2 / 292.9 and
# 122.8 / 693.6 -- so no size constant sits beside `_kl_path`.
ONEHOT_MAX_CLASSES = 256
ONEHOT_MAX_LOGITS = 2 ** 31 - 1


def onehot_kl_launches():
  """Kernel launches `emb_onehot_kl` and `emb_onehot_kl_grad` have issued in
  this process."""
  return _lib.launches('onehot_kl')


def _kl_path(fused, rows, stoch, classes):
  """True: the kernels, False: the composed path (`rssm_kl` says when).
  The kernels' median was below the composed path's at every shape, dtype and
  piece measured (profiles/rssm_kl_bench.txt), so `fused=None` takes them
  wherever they fit."""
  group = 1 <= classes <= ONEHOT_MAX_CLASSES
  index = stoch >= 1 and rows * stoch * classes <= ONEHOT_MAX_LOGITS
  if group and index:
    return fused is None or bool(fused)
  return _fused_path(
      'OneHot', fused,
      (group, f'{classes} classes, the kernels keep a group of at most {ONEHOT_MAX_CLASSES} in one wave\'s registers'),
      (index, f'{rows} x {stoch} x {classes} logits, the kernels index 1 .. 2^31 - 1'))


def _onehot_logits(logits, unimix):
  """outs.py:210-217, `Categorical.__init__`."""
  logits = logits.to(torch.float32)
  if unimix:
    probs = torch.softmax(logits, -1)
    uniform = torch.ones_like(probs) / probs.shape[-1]
    probs = (1 - unimix) * probs + unimix * uniform
    logits = torch.log(probs)
  return logits


def _composed_kl(logits, other):
  """outs.py:236-240 under `Agg(..., 1, sum)` (outs.py:73-76)."""
  logprob = torch.log_softmax(logits, -1)
  logother = torch.log_softmax(other, -1)
  prob = torch.softmax(logits, -1)
  return (prob * (logprob - logother)).sum(-1).sum(-1)


def _composed_entropy(logits):
  """outs.py:230-234 under `Agg(..., 1, sum)` (outs.py:69-71)."""
  logprob = torch.log_softmax(logits, -1)
  prob = torch.softmax(logits, -1)
  return (-(prob * logprob).sum(-1)).sum(-1)


def _kl_forward(x, y, dtype, unimix, free_nats):
  """One launch: (kl, ent_post, ent_prior, dyn, rep), each (rows,) float32."""
  rows, stoch, classes = x.shape
  out = _lib.empty((5, rows), torch.float32, x.device)
  kl, ent_post, ent_prior, dyn, rep = out.unbind(0)
  api.emb_onehot_kl(
      x.data_ptr(), y.data_ptr(), dtype, rows, stoch, classes, unimix, free_nats, kl.data_ptr(),
      ent_post.data_ptr(), ent_prior.data_ptr(), dyn.data_ptr(), rep.data_ptr(), _lib.raw_stream(x.device))
  return kl, ent_post, ent_prior, dyn, rep


def _kl_backward(x, y, dtype, unimix, free_nats, kl, g_rep, g_dyn, lead):
  """One launch: (grad_post, grad_prior); a side whose upstream gradient is None
  is not written and comes back None."""
  rows, stoch, classes = x.shape
  row_grad = lambda g: None if g is None else g.to(torch.float32).expand(lead).contiguous()
  g_rep, g_dyn = row_grad(g_rep), row_grad(g_dyn)
  if g_rep is None and g_dyn is None:
    return None, None
  grad_post = None if g_rep is None else torch.empty_like(x)
  grad_prior = None if g_dyn is None else torch.empty_like(y)
  api.emb_onehot_kl_grad(
      x.data_ptr(), y.data_ptr(), dtype, rows, stoch, classes, unimix, free_nats, kl.data_ptr(), _address(g_rep),
      _address(g_dyn), _address(grad_post), _address(grad_prior), _lib.raw_stream(x.device))
  return grad_post, grad_prior


class _FusedRssmKL(torch.autograd.Function):
  """(dyn, rep, dyn_ent, rep_ent) on the kernels: one launch forward, one
  backward.  dyn's gradient goes to prior, rep's to post."""

  @staticmethod
  def forward(ctx, post, prior, unimix, free_nats):
    x, y = (t.detach().contiguous().view(-1, *t.shape[-2:]) for t in (post, prior))
    lead = post.shape[:-2]
    kl, ent_post, ent_prior, dyn, rep = _kl_forward(x, y, _DTYPES[post.dtype], unimix, free_nats)
    ctx.saved = (x, y, kl, _DTYPES[post.dtype], unimix, free_nats, lead, post.shape)
    ctx.set_materialize_grads(False)
    dyn, rep, dyn_ent, rep_ent = (t.view(lead) for t in (dyn, rep, ent_prior, ent_post))
    ctx.mark_non_differentiable(dyn_ent, rep_ent)
    return dyn, rep, dyn_ent, rep_ent

  @staticmethod
  @once_differentiable
  def backward(ctx, g_dyn, g_rep, _dyn_ent, _rep_ent):
    x, y, kl, dtype, unimix, free_nats, lead, shape = ctx.saved
    needs = ctx.needs_input_grad
    grad_post, grad_prior = _kl_backward(
        x, y, dtype, unimix, free_nats, kl, g_rep if needs[0] else None, g_dyn if needs[1] else None, lead)
    view = lambda g: None if g is None else g.view(shape)
    return view(grad_post), view(grad_prior), None, None


class _FusedKL(torch.autograd.Function):
  """`OneHot.kl(other)` on the kernels: the raw kl, its gradient to both operands."""

  @staticmethod
  def forward(ctx, logits, other, unimix):
    x, y = (t.detach().contiguous().view(-1, *t.shape[-2:]) for t in (logits, other))
    lead = logits.shape[:-2]
    kl = _kl_forward(x, y, _DTYPES[logits.dtype], unimix, 0.0)[0]
    ctx.saved = (x, y, kl, _DTYPES[logits.dtype], unimix, lead, logits.shape)
    ctx.set_materialize_grads(False)
    return kl.view(lead)

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    x, y, kl, dtype, unimix, lead, shape = ctx.saved
    needs = ctx.needs_input_grad
    grad_self, grad_other = _kl_backward(
        x, y, dtype, unimix, 0.0, kl, gout if needs[0] else None, gout if needs[1] else None, lead)
    view = lambda g: None if g is None else g.view(shape)
    return view(grad_self), view(grad_other), None


def _check_onehot(who, logits):
  _check_device(logits)
  if logits.dtype not in _DTYPES:
    raise TypeError(f'{who}: logits must be float32 or bfloat16, got {logits.dtype}')
  if logits.dim() < 2:
    raise ValueError(f'{who}: logits of shape {tuple(logits.shape)}, needs (..., stoch, classes)')


def _check_pair(who, post, prior):
  _check_onehot(who, post)
  _check_onehot(who, prior)
  if post.shape != prior.shape:
    raise ValueError(f'{who}: logits of shapes {tuple(post.shape)} and {tuple(prior.shape)}')
  if post.dtype != prior.dtype or post.device != prior.device:
    raise TypeError(f'{who}: logits of {post.dtype} on {post.device} and {prior.dtype} on {prior.device}')


def _check_unimix(who, unimix):
  unimix = float(unimix)
  if not 0.0 <= unimix < 1.0:
    raise ValueError(f'{who}: unimix = {unimix}, needs 0 <= unimix < 1')
  return unimix


def _rows_of(logits):
  return int(np.prod(logits.shape[:-2], dtype=np.int64))


# ---- the draw: OneHot.sample / pred, Categorical.sample ----------------------

# What the kernels take: a group of at most 256 classes stays in one wave's
# registers, indices are 32-bit.  Structural, not a crossover: the fused median
# is below the composed one at all 28 rows of profiles/onehot_sample_bench.txt
# (rows 16, 1024 and 16 384 of (32, 32), (32, 64), (32, 65) and the actor's (1, 18),
# float32 and bfloat16, forward and forward + backward), and below the
# torch.multinomial composition's at every one too, so no size constant sits
# beside `_sample_path`; the figures are quoted there.
SAMPLE_MAX_CLASSES = 256
SAMPLE_MAX_LOGITS = 2 ** 31 - 1
_SAMPLE_DRAW, _SAMPLE_PRED = 0, 1


def onehot_sample_launches():
  """Kernel launches `emb_philox_uniform`, `emb_onehot_sample` and
  `emb_onehot_sample_grad` have issued in this process."""
  return _lib.launches('onehot_sample')


def _check_counter(who, name, value):
  if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
    raise TypeError(f'{who}: {name} must be an integer, got {type(value).__name__}')
  value = int(value)
  if not 0 <= value < 2 ** 64:
    raise ValueError(f'{who}: {name} = {value}, needs 0 <= {name} < 2^64')
  return value


def _philox(entry, who, what, seed, offset, first, count, device):
  """`philox_uniform` and `philox_normal`: `entry` is the entry point that fills
  the result, `who` the function's name in the refusals, `what` what it counts."""
  seed = _check_counter(who, 'seed', seed)
  offset = _check_counter(who, 'offset', offset)
  first = _check_counter(who, 'first', first)
  count = int(count)
  if count < 0 or first + count > 2 ** 64:
    raise ValueError(f'{who}: count = {count} from first = {first}, needs 0 <= count and {what} below 2^64')
  out = torch.empty((count,), dtype=torch.float32, device=_cuda_device(device))
  if count:
    entry(seed, offset, first, count, out.data_ptr(), _lib.raw_stream(out.device))
  return out


def philox_uniform(seed, offset=0, first=0, count=1, device=None):
  """(count,) float32 on `device`: the uniforms the sample kernels draw for the
  groups `first .. first + count - 1` -- Philox4x32-10 with key
  (seed & 0xffffffff, seed >> 32) and counter (g & 0xffffffff, g >> 32,
  offset & 0xffffffff, offset >> 32), u = (word 0 >> 8) * 2^-24 in [0, 1).  One
  launch (`emb_philox_uniform`); count = 0 launches nothing."""
  return _philox(api.emb_philox_uniform, 'philox_uniform', 'groups', seed, offset, first, count, device)


def _sample_path(who, fused, rows, groups, classes):
  """True: the kernels, False: the composed path (`OneHot.sample` says when).
  The kernels' median was below the composed path's at every shape, dtype and
  piece measured (profiles/onehot_sample_bench.txt) -- the RSSM's observe step,
  (16, 32, 32) f32: forward 17.9 us against 274.4, forward + backward 113.7
  against 416.5; its imagination step, (1024, 32, 32) f32: 17.0 / 244.0 and 70.4 /
  328.4; (16384, 32, 64) bf16: 238.5 / 3619.9 and 465.0 / 4162.9 -- so `fused=None`
  takes them wherever they fit.  Up to 1024 rows the fused forward is the host's
  enqueue, about 17 us whatever the size (the entry point alone: 4 .. 18 us)."""
  group = 1 <= classes <= SAMPLE_MAX_CLASSES
  index = groups >= 1 and rows * groups * classes <= SAMPLE_MAX_LOGITS
  if group and index:
    return fused is None or bool(fused)
  return _fused_path(
      who, fused,
      (group, f'{classes} classes, the kernels keep a group of at most {SAMPLE_MAX_CLASSES} in one wave\'s registers'),
      (index, f'{rows} x {groups} x {classes} logits, the kernels index 1 .. 2^31 - 1'))


def _sample_args(who, logits, seed, offset, uniform):
  """(seed, offset, uniform) checked; `uniform` None or float32 on the logits'
  device, one value per group, contiguous."""
  if not logits.is_contiguous():
    raise ValueError(f'{who}: logits of shape {tuple(logits.shape)} and strides {logits.stride()} are not contiguous')
  offset = _check_counter(who, 'offset', offset)
  if uniform is None:
    return _check_counter(who, 'seed', seed), offset, None
  seed = 0 if seed is None else _check_counter(who, 'seed', seed)
  if not (torch.is_tensor(uniform) and uniform.dtype == torch.float32 and uniform.device == logits.device):
    raise TypeError(f'{who}: uniform must be a float32 tensor on {logits.device}')
  if uniform.shape != logits.shape[:-1] or not uniform.is_contiguous():
    raise ValueError(f'{who}: uniform of shape {tuple(uniform.shape)}, needs a contiguous {tuple(logits.shape[:-1])}')
  return seed, offset, uniform.detach()


def _fused_sample(x, rows, groups, unimix, mode, seed, offset, uniform, want_index, want_onehot):
  """One launch: (index int32 (rows * groups,) or None, onehot like x or None)."""
  index = _lib.empty((rows * groups,), torch.int32, x.device) if want_index else None
  onehot = torch.empty_like(x) if want_onehot else None
  api.emb_onehot_sample(
      x.data_ptr(), _DTYPES[x.dtype], rows, groups, x.shape[-1], unimix, mode, seed, offset, _address(uniform),
      _address(index), _address(onehot), _lib.raw_stream(x.device))
  return index, onehot


class _FusedSample(torch.autograd.Function):
  """The straight-through one-hot on the kernels: one launch forward, one backward."""

  @staticmethod
  def forward(ctx, logits, geometry, unimix, mode, seed, offset, uniform):
    rows, groups = geometry
    x = logits.detach()
    onehot = _fused_sample(x, rows, groups, unimix, mode, seed, offset, uniform, False, True)[1]
    ctx.saved = (x, rows, groups, unimix)
    ctx.set_materialize_grads(False)
    return onehot

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    if gout is None:
      return (None,) * 7
    x, rows, groups, unimix = ctx.saved
    gout = gout.to(x.dtype).contiguous()
    grad = torch.empty_like(x)
    api.emb_onehot_sample_grad(
        x.data_ptr(), gout.data_ptr(), _DTYPES[x.dtype], rows, groups, x.shape[-1], unimix, grad.data_ptr(),
        _lib.raw_stream(x.device))
    return (grad,) + (None,) * 6


def _composed_uniform(logits, seed, offset, uniform):
  """One uniform per group, shaped as the logits without their classes: the
  caller's, or the Philox stream the kernels draw from."""
  if uniform is not None:
    return uniform
  shape = logits.shape[:-1]
  return philox_uniform(seed, offset, 0, int(np.prod(shape, dtype=np.int64)), logits.device).view(shape)


def _composed_index(probs, u):
  """The smallest k with p_k > 0 and C_k > u C_last, C = cumsum(p) in float32; none
  (rounding): the last class with p > 0; a group whose probabilities are NaN: -1."""
  cdf = torch.cumsum(probs, -1)
  hit = (cdf > u[..., None] * cdf[..., -1:]) & (probs > 0)
  index = torch.argmax(hit.to(torch.int8), -1)                       # the first True
  classes = probs.shape[-1]
  last = classes - 1 - torch.argmax((probs > 0).flip(-1).to(torch.int8), -1)
  index = torch.where(hit.any(-1), index, last)
  return torch.where(torch.isnan(probs).any(-1), -1, index)


def _composed_value(logits, unimix, index):
  """outs.py:265-270, `_onehot_with_grad`, in float32 and cast to the logits' dtype.
  `index` -1 (a group of NaN probabilities): the row is NaN by `probs - sg(probs)`."""
  dist = _onehot_logits(logits, unimix)
  value = torch.nn.functional.one_hot(index.clamp(min=0).to(torch.int64), logits.shape[-1]).to(torch.float32)
  probs = torch.softmax(dist, -1)
  value = value.detach() + (probs - probs.detach())
  return value.to(logits.dtype)


def _composed_draw(logits, unimix, seed, offset, uniform):
  """int64 indices, shaped as the logits without their classes, no gradient."""
  with torch.no_grad():
    probs = torch.softmax(_onehot_logits(logits, unimix), -1)        # outs.py:210-217, then what :223 samples from
    return _composed_index(probs, _composed_uniform(logits, seed, offset, uniform))


def _composed_argmax(logits):
  """argmax(x), the first on ties; a group with a NaN or +inf logit or nothing but -inf: -1."""
  with torch.no_grad():
    x = logits.to(torch.float32)
    top = x.amax(-1)
    bad = torch.isnan(x).any(-1) | torch.isinf(top)
    return torch.where(bad, -1, torch.argmax(x, -1))


class OneHot:
  """The reference's `Agg(OneHot(logits, unimix), 1, sum)` (rssm.py:173-176,
  outs.py:40-76, 208-263) over `logits` (..., stoch, classes), a CUDA tensor of
  float32 or bfloat16: `.entropy()` and `.kl(other)`, each (...) float32, and
  `.sample(seed)` / `.pred()`, the straight-through one-hot shaped and typed like
  the logits.  The reference computes in float32 (outs.py:211) and so does this;
  bfloat16 logits are widened in registers and the gradients come back in bfloat16.

  Two paths, as `TwoHot`: composed restates the reference line by line in torch
  (the definition, every size); fused is `emb_onehot_kl` / `emb_onehot_kl_grad`
  and `emb_onehot_sample` / `emb_onehot_sample_grad`, classes <= 256.
  `fused=None` takes the kernels where they fit, True / False
  force a path (True raises where they do not fit, and says why).  No rows: the
  composed path, nothing is launched.  `rssm_kl` documents the arithmetic and
  the non-finite logits."""

  def __init__(self, logits, unimix=0.0, fused=None):
    _check_onehot('OneHot', logits)
    self.logits = logits
    self.unimix = _check_unimix('OneHot', unimix)
    self._lead = logits.shape[:-2]
    rows = _rows_of(logits)
    self._fused_arg = fused
    self.fused = _kl_path(fused, rows, *logits.shape[-2:]) and rows > 0

  def _sample_fused(self):
    rows, (groups, classes) = _rows_of(self.logits), self.logits.shape[-2:]
    return _sample_path('OneHot', self._fused_arg, rows, groups, classes) and rows * groups > 0

  def sample(self, seed=None, offset=0, uniform=None):
    """rssm.py:87, 100 over outs.py:252-254, 265-270: one class per group drawn
    from p = (1 - unimix) softmax(logits) + unimix / classes, as the straight-through
    one-hot `sg(onehot) + (probs - sg(probs))` -- exactly 0 or 1, shaped and typed
    like the logits, differentiable once: the gradient is
    (1 - unimix) s (g - sum_k s_k g_k), s = softmax(logits), whatever was drawn.

    The draw is the inverse CDF of one uniform per group: the smallest k with
    p_k > 0 and C_k > u C_last, C the float32 prefix sum of p in class order (a
    class of probability exactly 0 is never returned).  u comes from
    Philox4x32-10 keyed by `seed` at counter (g, `offset`), g the group's flat
    index (`philox_uniform`): it depends on (seed, offset, g) alone, not on the
    dtype, the path, the launch geometry or the rows that follow.  Give every
    call its own `offset` (a step counter) or `seed`; both are integers in
    [0, 2^64).  `uniform`, a float32 tensor of one value in [0, 1) per group
    (shaped as the logits without their classes), replaces the counter for
    callers who bring their own generator.  It is also the way to fresh draws
    inside a captured graph: `seed` and `offset` travel to the kernel by value,
    so a replayed graph repeats the draw it captured, while a `uniform` tensor
    refilled between replays is read anew.

    On the kernels that is ONE launch forward and ONE backward; the composed
    path draws the same uniforms with `emb_philox_uniform` and takes `cumsum`,
    the comparison and `argmax`, so both paths draw the same class except
    where u lies within rounding of a boundary of the CDF.  The logits must be
    contiguous.  A group with a NaN or +inf logit, or nothing but -inf, gives a
    NaN row and a NaN gradient, and touches no other group."""
    seed, offset, uniform = _sample_args('OneHot.sample', self.logits, seed, offset, uniform)
    if self._sample_fused():
      geometry = (_rows_of(self.logits), self.logits.shape[-2])
      return _FusedSample.apply(self.logits, geometry, self.unimix, _SAMPLE_DRAW, seed, offset, uniform)
    index = _composed_draw(self.logits, self.unimix, seed, offset, uniform)
    return _composed_value(self.logits, self.unimix, index)

  def pred(self):
    """outs.py:248-250: the straight-through one-hot of argmax(logits), the first
    class on ties (the mix is increasing in the logits, so it is the argmax of
    outs.py:219-220 too); same gradient, launches and non-finite groups as `sample`."""
    _sample_args('OneHot.pred', self.logits, 0, 0, None)
    if self._sample_fused():
      geometry = (_rows_of(self.logits), self.logits.shape[-2])
      return _FusedSample.apply(self.logits, geometry, self.unimix, _SAMPLE_PRED, 0, 0, None)
    return _composed_value(self.logits, self.unimix, _composed_argmax(self.logits))

  def entropy(self):
    """(...) float32, no gradient: the reference uses it for metrics only
    (rssm.py:131-132).  On the kernels: the forward launch with these logits on
    both sides."""
    with torch.no_grad():
      if self.fused:
        x = self.logits.detach().contiguous().view(-1, *self.logits.shape[-2:])
        return _kl_forward(x, x, _DTYPES[x.dtype], self.unimix, 0.0)[1].view(self._lead)
      return _composed_entropy(_onehot_logits(self.logits, self.unimix))

  def kl(self, other):
    """(...) float32: kl(self || other), differentiable once with respect to
    both operands.  `other` is a `OneHot` of the same shape, dtype and unimix."""
    if not isinstance(other, OneHot):
      raise TypeError(f'OneHot.kl: other must be a OneHot, got {type(other).__name__}')
    _check_pair('OneHot.kl', self.logits, other.logits)
    if other.unimix != self.unimix:
      raise ValueError(f'OneHot.kl: unimix {self.unimix} against {other.unimix}')
    if self.fused:
      return _FusedKL.apply(self.logits, other.logits, self.unimix)
    return _composed_kl(_onehot_logits(self.logits, self.unimix), _onehot_logits(other.logits, self.unimix))


def rssm_kl(post, prior, unimix=0.01, free_nats=1.0, fused=None):
  """The KL pair of `RSSM.loss` (rssm.py:123-132) over `post` and `prior`
  (..., stoch, classes), CUDA tensors of float32 or bfloat16:

      dyn = max(kl(sg(post) || prior), free_nats)      gradient to prior only
      rep = max(kl(post || sg(prior)), free_nats)      gradient to post only
      dyn_ent = entropy(prior), rep_ent = entropy(post)      no gradient

  as a dict of four (...) float32 tensors (the metrics' `.mean()` is the
  caller's).  `free_nats == 0` takes no maximum (rssm.py:127).  On the kernels
  that is ONE launch forward and ONE backward: dyn and rep have the same value,
  and both gradients have a closed form.  The maximum's gradient is 1 above
  free_nats, 0 below and 1/2 at equality, as `jnp.maximum`'s.  An output that
  takes no part in the loss costs nothing: its side is not written.

  Per group the reference mixes, takes the log, and then runs softmax and
  log_softmax over that log again (outs.py:212-216, 231-232, 237-239).  The
  composed path repeats that; the kernels do not: after the mix the
  probabilities sum to 1 up to rounding, so the second pass is the identity.
  With `unimix == 0` both work in the log domain (`log_softmax`), finite for a
  class whose probability underflows.

  Non-finite logits.  A NaN or +inf logit, or a group of -inf, makes that row's
  dyn and rep and the entropy of the side it is in NaN on both paths and touches
  no other row (the other side's entropy is what it was).  Its gradients: on the
  kernels the whole row's, on both sides, are NaN (a NaN kl is on neither side
  of free_nats); composed is the definition, NaN in the poisoned group on both
  sides and whatever autograd leaves in the row's other groups.  With
  `unimix > 0` a -inf logit is a class of probability unimix / classes and
  everything stays finite.  With `unimix == 0` a -inf logit in `post` is
  0 * -inf in the definition: both paths return NaN for that row's dyn, rep and
  rep_ent (dyn_ent stays finite) and for post's gradient in that group (the
  kernels: both gradients over the whole row); one in `prior` alone makes dyn
  and rep +inf and dyn_ent NaN."""
  _check_pair('rssm_kl', post, prior)
  unimix = _check_unimix('rssm_kl', unimix)
  free_nats = float(free_nats)
  if not free_nats >= 0.0:
    raise ValueError(f'rssm_kl: free_nats = {free_nats}, needs >= 0 (0: no maximum)')
  rows = _rows_of(post)
  if _kl_path(fused, rows, *post.shape[-2:]) and rows > 0:
    dyn, rep, dyn_ent, rep_ent = _FusedRssmKL.apply(post, prior, unimix, free_nats)
    return {'dyn': dyn, 'rep': rep, 'dyn_ent': dyn_ent, 'rep_ent': rep_ent}
  dist = lambda logits: _onehot_logits(logits, unimix)
  dyn = _composed_kl(dist(post.detach()), dist(prior))
  rep = _composed_kl(dist(post), dist(prior.detach()))
  if free_nats:
    floor = torch.full((), free_nats, dtype=torch.float32, device=post.device)
    dyn = torch.maximum(dyn, floor)
    rep = torch.maximum(rep, floor)
  with torch.no_grad():
    dyn_ent = _composed_entropy(dist(prior))
    rep_ent = _composed_entropy(dist(post))
  return {'dyn': dyn, 'rep': rep, 'dyn_ent': dyn_ent, 'rep_ent': rep_ent}


# ---- Categorical: the actor's discrete policy, its logp, entropy and loss ----

# What the kernels take: a group of at most 256 classes stays in one wave's
# registers, indices are 32-bit.  Structural, not a crossover: the fused median
# is below the composed one at all 48 rows of profiles/policy_loss_bench.txt (N
# 1024 and 16 384, T 16, classes 6, 18 and 256, one group and four, float32 and
# bfloat16, forward and forward + backward) -- (16384, 16, 4, 256) f32: forward
# 488.9 us against 4436.5, forward + backward 1710.5 against 8926.0; the closest,
# (16384, 16, 6) bf16: 75.3 / 100.4 and 195.6 / 259.0 -- so no size constant sits
# beside `_policy_path`.
POLICY_MAX_CLASSES = 256
POLICY_MAX_LOGITS = 2 ** 31 - 1


def policy_loss_launches():
  """Kernel launches `emb_policy_loss` and `emb_policy_loss_grad` have issued in
  this process."""
  return _lib.launches('policy_loss')


def _policy_path(fused, rows, groups, classes):
  """True: the kernels, False: the composed path (`policy_loss` says when);
  `rows` counts the logits' rows, a dropped step's included.  The kernels' median
  was below the composed path's at every shape, dtype and piece measured
  (profiles/policy_loss_bench.txt), so `fused=None` takes them wherever they fit."""
  group = 1 <= classes <= POLICY_MAX_CLASSES
  index = groups >= 1 and rows * groups * classes <= POLICY_MAX_LOGITS
  if group and index:
    return fused is None or bool(fused)
  return _fused_path(
      'Categorical', fused,
      (group, f'{classes} classes, the kernels keep a group of at most {POLICY_MAX_CLASSES} in one wave\'s registers'),
      (index, f'{rows} x {groups} x {classes} logits, the kernels index 1 .. 2^31 - 1'))


def _check_categorical(who, logits, dims):
  _check_device(logits)
  if logits.dtype not in _DTYPES:
    raise TypeError(f'{who}: logits must be float32 or bfloat16, got {logits.dtype}')
  if dims not in (0, 1):
    raise ValueError(f'{who}: dims = {dims!r}, needs 0 (..., classes) or 1 (..., groups, classes); '
                     'flatten more action dimensions into the groups')
  if logits.dim() < 1 + dims or logits.shape[-1] < 1:
    raise ValueError(f'{who}: logits of shape {tuple(logits.shape)}, needs '
                     f'{"(..., groups, classes)" if dims else "(..., classes)"}')


def _actions(who, act, logits, dims):
  """`act` as int32 on the logits' device, shaped as the logits without their
  classes.  Values stay what they are: the one-hot is a comparison, an action
  outside [0, classes) matches no class."""
  want = logits.shape[:-1]
  if not torch.is_tensor(act):
    act = torch.as_tensor(np.asarray(act))
  if act.dtype.is_floating_point or act.dtype in (torch.bool, torch.complex64, torch.complex128):
    raise TypeError(f'{who}: actions must be integers, got {act.dtype}')
  if act.shape != want:
    raise ValueError(f'{who}: actions of shape {tuple(act.shape)}, the logits need {tuple(want)}')
  act = act.detach().to(logits.device)
  if act.dtype != torch.int32:
    if act.dtype == torch.int64:        # what does not fit int32 is out of range before and after
      act = act.clamp(-1, logits.shape[-1])
    act = act.to(torch.int32)
  return act.contiguous()


def _composed_logp(logits, act, dims):
  """outs.py:226-228 under `Agg.logp` (outs.py:63-64): `logits` is what
  `Categorical.__init__` keeps, `act` int32.  jax.nn.one_hot as a comparison
  with arange: a row of zeros for an action outside [0, classes)."""
  classes = logits.shape[-1]
  onehot = (act[..., None] == torch.arange(classes, dtype=torch.int32, device=act.device)).to(torch.float32)
  logp = (torch.log_softmax(logits, -1) * onehot).sum(-1)
  return logp.sum(-1) if dims else logp


def _composed_cat_entropy(logits, dims):
  """outs.py:230-234 under `Agg.entropy` (outs.py:69-71)."""
  logprob = torch.log_softmax(logits, -1)
  prob = torch.softmax(logits, -1)
  entropy = -(prob * logprob).sum(-1)
  return entropy.sum(-1) if dims else entropy


class _FusedPolicy(torch.autograd.Function):
  """(loss, logpi, ent), each (N * (T - drop),) float32, on the kernels: one
  launch forward, one backward.  Only `loss` carries a gradient, to the logits."""

  @staticmethod
  def forward(ctx, logits, act, adv, weight, stride, geometry, unimix, actent):
    n, t, drop, groups, classes = geometry
    x = logits.detach().contiguous()
    dtype = _DTYPES[logits.dtype]
    loss, logpi, ent = _lib.empty((3, n * (t - drop)), torch.float32, x.device).unbind(0)
    api.emb_policy_loss(
        x.data_ptr(), _address(act), dtype, n, t, drop, groups, classes, unimix, actent, _address(adv),
        _address(weight), stride, loss.data_ptr(), logpi.data_ptr(), ent.data_ptr(), _lib.raw_stream(x.device))
    ctx.saved = (x, act, adv, weight, stride, geometry, unimix, actent, dtype, logits.shape)
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(logpi, ent)
    return loss, logpi, ent

  @staticmethod
  @once_differentiable
  def backward(ctx, gout, _logpi, _ent):
    if gout is None:
      return (None,) * 8
    x, act, adv, weight, stride, geometry, unimix, actent, dtype, shape = ctx.saved
    n, t, drop, groups, classes = geometry
    gout = gout.to(torch.float32).contiguous()
    grad = torch.empty_like(x)
    api.emb_policy_loss_grad(
        x.data_ptr(), _address(act), dtype, n, t, drop, groups, classes, unimix, actent, _address(adv),
        _address(weight), stride, gout.data_ptr(), grad.data_ptr(), _lib.raw_stream(x.device))
    return (grad.view(shape),) + (None,) * 7


class Categorical:
  """The reference's `Agg(Categorical(logits, unimix), dims, sum)` (heads.py:90-91,
  101-110, outs.py:40-76, 208-240), the discrete policy head, over a CUDA tensor
  of float32 or bfloat16:

    dims=0   logits (..., classes), actions (...)
    dims=1   logits (..., groups, classes), actions (..., groups), `logp` and
             `entropy` summed over the groups; more action dimensions are
             flattened into the groups by the caller

  `.logp(act)` and `.entropy()` are (...) float32 and differentiable once with
  respect to the logits (the entropy is part of the actor's loss, agent.py:412-414);
  `.pred()` is the argmax (composed torch ops).  `.minent = 0` and
  `.maxent = log(classes) * groups` are what agent.py:440-442 reads.  `.sample(seed)`
  draws int32 actions (`emb_onehot_sample`).  An action outside [0, classes) has log-probability 0, as the row
  of zeros `jax.nn.one_hot` gives it; it is never used as an address.

  Two paths, as `OneHot`: composed restates the reference line by line in torch
  (the definition, every size); fused is `emb_policy_loss` /
  `emb_policy_loss_grad`, classes <= 256, one launch per call and one per
  backward.  `fused=None` takes the kernels where they fit, True / False force a
  path (True raises where they do not fit, and says why).  No rows: the composed
  path, nothing is launched.  `policy_loss` documents the arithmetic and the
  non-finite logits."""

  def __init__(self, logits, unimix=0.0, dims=0, fused=None):
    _check_categorical('Categorical', logits, dims)
    self.logits = logits
    self.unimix = _check_unimix('Categorical', unimix)
    self.dims = dims
    self._lead = logits.shape[:-1 - dims]
    self._groups = logits.shape[-2] if dims else 1
    self._classes = logits.shape[-1]
    self._rows = int(np.prod(self._lead, dtype=np.int64))
    self._fused_arg = fused
    self.fused = _policy_path(fused, self._rows, self._groups, self._classes) and self._rows > 0 and self._groups > 0
    self.minent = 0.0
    self.maxent = float(np.log(self._classes)) * self._groups

  def _launch(self, act, actent):
    geometry = (self._rows, 1, 0, self._groups, self._classes)
    return _FusedPolicy.apply(self.logits, act, None, None, 1, geometry, self.unimix, actent)[0].view(self._lead)

  def pred(self):
    """outs.py:219-220: the argmax over the classes, int64, (...) or (..., groups)."""
    return torch.argmax(_onehot_logits(self.logits.detach(), self.unimix), -1)

  def sample(self, seed=None, offset=0, uniform=None):
    """agent.py:18, 126, 192 over outs.py:222-224: int32 class indices shaped as the
    logits without their classes, (...) or (..., groups), no gradient -- what
    `logp` and `policy_loss` take as `act`.  The draw, `seed`, `offset` and
    `uniform` are `OneHot.sample`'s: the same kernel with the one-hot store off,
    so both return the same class for the same (seed, offset).  `seed` and
    `offset` travel by value and replay as captured inside a graph; `uniform`
    is read anew.  The logits must be contiguous.  A group with a NaN or +inf
    logit, or nothing but -inf: -1."""
    seed, offset, uniform = _sample_args('Categorical.sample', self.logits, seed, offset, uniform)
    count = self._rows * self._groups
    if _sample_path('Categorical', self._fused_arg, self._rows, self._groups, self._classes) and count > 0:
      index = _fused_sample(self.logits.detach(), self._rows, self._groups, self.unimix, _SAMPLE_DRAW, seed, offset,
                            uniform, True, False)[0]
      return index.view(self.logits.shape[:-1])
    return _composed_draw(self.logits.detach(), self.unimix, seed, offset, uniform).to(torch.int32)

  def logp(self, act):
    """(...) float32: the log-probability of `act` (int32 or int64; a constant)."""
    act = _actions('Categorical.logp', act, self.logits, self.dims)
    if self.fused:
      return -self._launch(act, 0.0)              # the launch's loss with adv = weight = 1, actent = 0 is -logp
    return _composed_logp(_onehot_logits(self.logits, self.unimix), act, self.dims)

  def entropy(self):
    """(...) float32."""
    if self.fused:
      return self._launch(None, -1.0)             # no action and actent = -1: the launch's loss is the entropy
    return _composed_cat_entropy(_onehot_logits(self.logits, self.unimix), self.dims)


# The frame of the actor's loss (agent.py:411-415), what `policy_loss` and
# `normal_policy_loss` share: `who` is the caller's name in the refusals.

def _loss_frame(who, what, x, lead, actent, drop_last):
  """(actent, n, t, drop, kept, out_shape) of a loss over the leading shape `lead`
  of `x`, the `what` of the time-axis refusal: n sequences of t steps, of which
  the first `kept` make the outputs."""
  actent = float(actent)
  if not np.isfinite(actent):
    raise ValueError(f'{who}: actent = {actent}, needs a finite value')
  drop = 1 if drop_last else 0
  if drop and not lead:
    raise ValueError(f'{who}: drop_last needs a time axis, {what} of shape {tuple(x.shape)}')
  n, t = (int(np.prod(lead[:-1], dtype=np.int64)), lead[-1]) if drop else (int(np.prod(lead, dtype=np.int64)), 1)
  kept = max(t - drop, 0)
  return actent, n, t, drop, kept, (*lead[:-1], kept) if drop else tuple(lead)


def _loss_constant(who, name, value, shapes, device):
  """`adv` or `weight`: float32 and contiguous on `device`, in one of `shapes`; a constant."""
  if not torch.is_tensor(value):
    value = torch.as_tensor(np.asarray(value, np.float32))
  if tuple(value.shape) not in shapes:
    raise ValueError(f'{who}: {name} of shape {tuple(value.shape)}, needs ' +
                     ' or '.join(str(tuple(s)) for s in shapes))
  return value.detach().to(device=device, dtype=torch.float32).contiguous()


def _kept_steps(lead, drop, kept, weight, *tensors):
  """The reference's [:, :-1], taken before the arithmetic instead of after: a dropped step takes no part."""
  if not drop:
    return (weight, *tensors)
  axis = len(lead) - 1
  return (weight[..., :kept], *(x.narrow(axis, 0, kept) for x in tensors))


def _composed_loss(logpi, ent, adv, weight, actent):
  loss = weight * -(logpi * adv + actent * ent)
  return {'loss': loss, 'logpi': logpi.detach(), 'ent': ent.detach()}


def policy_loss(logits, act, adv, weight, actent=3e-4, unimix=0.0, dims=0, drop_last=True, fused=None):
  """The actor's loss of `imag_loss` (agent.py:411-415) for one action key:

      logpi = policy.logp(sg(act))[:, :-1]
      ent   = policy.entropy()[:, :-1]
      loss  = sg(weight[:, :-1]) * -(logpi * sg(adv) + actent * ent)

  with policy = `Categorical(logits, unimix, dims)`, as a dict of three float32
  tensors.  `loss` is differentiable once with respect to the logits and to
  nothing else: `adv` and `weight` are constants, the reference's `sg`.  `logpi`
  and `ent` carry no gradient; they are for `metrics['ent/...']`
  (agent.py:438-442).

  `logits` is (N.., T, [groups,] classes) and `act` (N.., T[, groups]) int32 or
  int64.  With `drop_last` the last step of every sequence is dropped, the
  reference's `[:, :-1]`: the outputs and `adv` are (N.., T - 1), and `weight` is
  (N.., T) as `scans.dreamer_targets` returns it or (N.., T - 1).  Without it all
  three are the leading shape of the logits, whatever its rank.  The kernels read
  the kept rows in place: the logits are neither sliced nor copied and a dropped
  step is not read.

  A dict of actions needs no fused sum of heads: the loss is linear in `logpi`
  and `ent`, so the reference's sum over action keys (agent.py:411-414) is the sum
  of one `policy_loss` per key.

  Two paths, as `Categorical`.  On the kernels that is ONE launch forward and ONE
  backward.  No output rows (N = 0, or T = 1 with `drop_last`): nothing is
  launched and the gradient is zeros.

  Per group the reference mixes, takes the log, and then runs softmax and
  log_softmax over that log again (outs.py:212-216, 228, 231-232).  The composed
  path repeats that; the kernels do not: after the mix the probabilities sum to 1
  up to rounding, so the second pass is the identity.  With `unimix == 0` both
  work in the log domain (`log_softmax`), finite for a class whose probability
  underflows.

  Non-finite logits.  A NaN or +inf logit, or a group of -inf, in a kept step
  makes that output row's `loss`, `logpi` and `ent` NaN on both paths and touches
  no other row.  Its gradient: on the kernels the whole row's is NaN; composed is
  the definition, NaN in the poisoned group and whatever autograd leaves in the
  row's other groups.  The same values in a dropped step touch nothing: every
  output has the bits of the clean run and that step's gradient is zeros.  With
  `unimix > 0` a single -inf logit is a class of probability unimix / classes and
  everything stays finite.  With `unimix == 0` it is 0 * -inf in the definition's
  entropy and in its product with the one-hot: both paths return NaN for that
  row's three outputs."""
  _check_categorical('policy_loss', logits, dims)
  unimix = _check_unimix('policy_loss', unimix)
  lead = logits.shape[:-1 - dims]
  groups, classes = (logits.shape[-2] if dims else 1), logits.shape[-1]
  actent, n, t, drop, kept, out_shape = _loss_frame('policy_loss', 'logits', logits, lead, actent, drop_last)
  act = _actions('policy_loss', act, logits, dims)
  adv = _loss_constant('policy_loss', 'adv', adv, (out_shape,), logits.device)
  weight = _loss_constant('policy_loss', 'weight', weight, (out_shape, tuple(lead)), logits.device)
  if _policy_path(fused, n * t, groups, classes) and n * kept > 0 and groups > 0:
    stride, geometry = weight.shape[-1] if drop else 1, (n, t, drop, groups, classes)
    loss, logpi, ent = _FusedPolicy.apply(logits, act, adv, weight, stride, geometry, unimix, actent)
    return {'loss': loss.view(out_shape), 'logpi': logpi.view(out_shape), 'ent': ent.view(out_shape)}
  weight, logits, act = _kept_steps(lead, drop, kept, weight, logits, act)
  dist = _onehot_logits(logits, unimix)
  return _composed_loss(_composed_logp(dist, act, dims), _composed_cat_entropy(dist, dims), adv, weight, actent)


# ---- the reconstruction heads: image MSE from uint8, symlog MSE, Binary ----------

# What the kernels take: indices are 32-bit.  Structural, not a crossover; what
# `fused=None` does with it is written beside `_recon_path`.
RECON_MAX_ELEMENTS = 2 ** 31 - 1
_RECON_TARGETS = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.uint8: _lib.U8}


def recon_loss_launches():
  """Kernel launches `emb_recon_loss` and `emb_recon_loss_grad` have issued in
  this process."""
  return _lib.launches('recon_loss')


def _recon_path(who, fused, rows, units):
  """True: the kernels, False: the composed path (`ImageMSE` says when).  The
  kernels' median was below the composed path's at all 18 rows of
  profiles/recon_loss_bench.txt (images (1024, 64, 64, 3) and (4096, 64, 64, 3) in
  bfloat16 and float32 and (1024, 96, 96, 3), symlog vectors (1024, 1024) and
  (1024, 7), the continue head (1024,) and (16384,), forward and forward +
  backward) -- the image loss at (1024, 64, 64, 3) bfloat16: forward 24.8 us
  against 115.3, forward + backward 122.8 against 210.0; the closest, symlog
  (1024, 1024): 16.6 / 37.3 and 70.5 / 94.2 -- so `fused=None` takes them wherever
  they fit and no size constant sits here.  Below about a megabyte the fused
  forward is the host's enqueue, about 16.5 us whatever the size."""
  if units >= 1 and rows * units <= RECON_MAX_ELEMENTS:
    return fused is None or bool(fused)
  return _fused_path(who, fused, (False, f'{rows} x {units} elements, the kernels index 1 .. 2^31 - 1'))


def _recon_geometry(who, x, dims):
  """(lead, rows, units) of summing the last `dims` axes of `x`."""
  if isinstance(dims, bool) or not isinstance(dims, (int, np.integer)) or not 0 <= dims <= x.dim():
    raise ValueError(f'{who}: dims = {dims!r}, needs 0 .. {x.dim()} for a shape of {tuple(x.shape)}')
  lead = x.shape[:x.dim() - dims]
  return lead, int(np.prod(lead, dtype=np.int64)), int(np.prod(x.shape[x.dim() - dims:], dtype=np.int64))


def _recon_input(who, x, name='x'):
  _check_device(x)
  if x.dtype not in _DTYPES:
    raise TypeError(f'{who}: {name} must be float32 or bfloat16, got {x.dtype}')


def _recon_target(who, target, x, kinds):
  """`target` on the device of `x` in a dtype the launch takes, shaped like `x`; a constant."""
  if not torch.is_tensor(target):
    target = torch.as_tensor(np.asarray(target))
  if tuple(target.shape) != tuple(x.shape):
    raise ValueError(f'{who}: target of shape {tuple(target.shape)}, needs {tuple(x.shape)}')
  if target.dtype not in kinds:
    raise TypeError(f'{who}: target must be one of {", ".join(str(k) for k in kinds)}, got {target.dtype}')
  return target.detach().to(x.device)


class _FusedRecon(torch.autograd.Function):
  """The row sums on the kernels: one launch forward, one launch backward."""

  @staticmethod
  def forward(ctx, x, target, op, div, geometry):
    lead, rows, units = geometry
    xc = x.detach().contiguous()
    target = target.contiguous()
    if target.dtype == torch.bool:
      target = target.view(torch.uint8)
    loss = _lib.empty((rows,), torch.float32, x.device)
    args = (xc.data_ptr(), _DTYPES[xc.dtype], target.data_ptr(), _RECON_TARGETS[target.dtype], div, rows, units, op)
    api.emb_recon_loss(*args, loss.data_ptr(), _lib.raw_stream(x.device))
    ctx.saved = (xc, target, args, lead, x.shape)
    ctx.set_materialize_grads(False)
    return loss.view(lead)

  @staticmethod
  @once_differentiable
  def backward(ctx, gout):
    if gout is None:
      return (None,) * 5
    xc, target, args, lead, shape = ctx.saved
    gout = gout.to(torch.float32).expand(lead).contiguous()
    grad = torch.empty_like(xc)
    api.emb_recon_loss_grad(*args, gout.data_ptr(), grad.data_ptr(), _lib.raw_stream(xc.device))
    return (grad.view(shape),) + (None,) * 4


def _agg(loss, dims):
  """outs.py:56-58, `Agg.loss` with `jnp.sum` over the last `dims` axes."""
  return loss.sum(tuple(range(-dims, 0))) if dims else loss


def _symlog(x):
  """nets.py symlog."""
  return torch.sign(x) * torch.log1p(torch.abs(x))


class MSE:
  """The reference's `Agg(MSE(mean, squash), dims, sum)` (outs.py:40-58, 129-141;
  `symlog_mse`: heads.py:127-130) over `mean`, a CUDA tensor of float32 or
  bfloat16.  `squash` is None or 'symlog' (nets.py symlog, applied to the target).
  The reference computes in float32 (outs.py:132) and so does this; a bfloat16
  mean is widened in registers and its gradient comes back in bfloat16.

  Two paths, as `TwoHot`: composed restates the reference operation by operation
  in torch (the definition, every size); fused is `emb_recon_loss` /
  `emb_recon_loss_grad`, one launch forward and one backward, at most 2^31 - 1
  elements.  `fused=None` takes the kernels where they fit, True / False force a
  path (True raises where they do not fit, and says why).  No rows: the composed
  path, nothing is launched.  A `mean` that is not contiguous is made contiguous
  with one torch op.

  A NaN or infinite element of `mean` makes its own row's loss and its own
  gradient element NaN on the kernels and touches no other row (composed: what
  the definition gives, +inf for an infinite element)."""

  def __init__(self, mean, squash=None, fused=None):
    _recon_input('MSE', mean, 'mean')
    if squash not in (None, 'symlog'):
      raise ValueError(f"MSE: squash = {squash!r}, needs None or 'symlog'")
    self.mean = mean
    self.squash = squash
    self._fused_arg = fused

  def pred(self):
    """outs.py:135-136: the mean in float32, no gradient."""
    return self.mean.detach().to(torch.float32)

  def loss(self, target, dims=0):
    """The squared error against `target` (float32 or bfloat16, the shape of
    `mean`; a constant) summed over the last `dims` axes: float32, shaped as the
    axes before them.  `dims=0` is elementwise.  Differentiable once with respect
    to `mean`."""
    lead, rows, units = _recon_geometry('MSE.loss', self.mean, dims)
    target = _recon_target('MSE.loss', target, self.mean, (torch.float32, torch.bfloat16))
    if _recon_path('MSE', self._fused_arg, rows, units) and rows > 0:
      op = _lib.EMB_RECON_MSE_SYMLOG if self.squash else _lib.EMB_RECON_MSE
      return _FusedRecon.apply(self.mean, target, op, 1.0, (lead, rows, units))
    target = target.to(torch.float32)
    if self.squash:
      target = _symlog(target)
    return _agg(torch.square(self.mean.to(torch.float32) - target), dims)


class ImageMSE:
  """The image reconstruction loss (agent.py:170-182): the decoder's last line
  `jax.nn.sigmoid(x)` (rssm.py:349) under `Agg(MSE(out), 3, sum)` (rssm.py:353-356),
  trained against `f32(image) / 255` (agent.py:181).  `x` is the decoder's
  PRE-sigmoid output (..., H, W, C), a CUDA tensor of float32 or bfloat16;
  `sigmoid=False` is the plain MSE of `x` against `image / 255`.

  Two paths, as `MSE`.  On the kernels the uint8 frames are read once, widened
  and divided by 255 in registers (the float32 division the reference writes);
  no float copy of the batch is made, forward or backward.

  One difference, as `nets.norm_act` documents its own: the reference rounds
  sigmoid(x) to the compute dtype before `MSE` widens it again (rssm.py:349,
  outs.py:132).  The composed path keeps that rounding; the kernels do not --
  they take the sigmoid of the widened x in float32 and never round it.  For
  float32 there is no difference."""

  def __init__(self, x, sigmoid=True, fused=None):
    _recon_input('ImageMSE', x)
    self.x = x
    self.sigmoid = bool(sigmoid)
    self._fused_arg = fused

  def pred(self):
    """sigmoid(x) (or x) in float32, no gradient: composed torch ops, for the report path."""
    x = self.x.detach()
    return (torch.sigmoid(x) if self.sigmoid else x).to(torch.float32)

  def loss(self, image, dims=3):
    """The squared error against `image / 255` (uint8, the shape of `x`; a
    constant) summed over the last `dims` axes: float32.  Differentiable once
    with respect to `x`."""
    lead, rows, units = _recon_geometry('ImageMSE.loss', self.x, dims)
    image = _recon_target('ImageMSE.loss', image, self.x, (torch.uint8,))
    if _recon_path('ImageMSE', self._fused_arg, rows, units) and rows > 0:
      op = _lib.EMB_RECON_SIGMOID_MSE if self.sigmoid else _lib.EMB_RECON_MSE
      return _FusedRecon.apply(self.x, image, op, 255.0, (lead, rows, units))
    mean = torch.sigmoid(self.x) if self.sigmoid else self.x          # rssm.py:349, in the compute dtype
    # agent.py:181 divides; torch turns a division by a Python scalar into a product with its
    # reciprocal, which rounds k / 255 differently for some k: divide by a tensor
    scale = torch.full((), 255.0, dtype=torch.float32, device=image.device)
    return _agg(torch.square(mean.to(torch.float32) - image.to(torch.float32) / scale), dims)


class Binary:
  """The reference's `Binary` (outs.py:189-205), the continue head (agent.py:177),
  over `logit`, a CUDA tensor of float32 or bfloat16; `dims` sums the last axes as
  `Agg` does.  Two paths, as `MSE`; the kernels compute
  logsigmoid(x) = min(x, 0) - log1p(exp(-|x|)), so logit = +-1e4 against the
  wrong label costs |logit| and stays finite."""

  def __init__(self, logit, fused=None):
    _recon_input('Binary', logit, 'logit')
    self.logit = logit
    self._fused_arg = fused

  def pred(self):
    """outs.py:194-195."""
    return self.logit.detach() > 0

  def _event(self, who, event):
    kinds = (torch.bool, torch.uint8, torch.float32, torch.bfloat16, torch.float16, torch.float64)
    event = _recon_target(who, event, self.logit, kinds)
    return event.to(torch.float32) if event.dtype in (torch.float16, torch.float64) else event

  def loss(self, target, dims=0):
    """-logp(target) (outs.py:21-22): float32, differentiable once with respect to the logit."""
    lead, rows, units = _recon_geometry('Binary.loss', self.logit, dims)
    target = self._event('Binary.loss', target)
    if _recon_path('Binary', self._fused_arg, rows, units) and rows > 0:
      return _FusedRecon.apply(self.logit, target, _lib.EMB_RECON_BINARY, 1.0, (lead, rows, units))
    return -self._composed_logp(target, dims)

  def logp(self, event, dims=0):
    """outs.py:197-201: event * logsigmoid(logit) + (1 - event) * logsigmoid(-logit);
    `event` is torch.bool, uint8 or a float tensor of the logit's shape."""
    return -self.loss(event, dims)

  def _composed_logp(self, event, dims):
    logit = self.logit.to(torch.float32)
    event = event.to(torch.float32)
    logp = torch.nn.functional.logsigmoid(logit)
    lognotp = torch.nn.functional.logsigmoid(-logit)
    return _agg(event * logp + (1 - event) * lognotp, dims)

  def sample(self, seed=None, offset=0, uniform=None):
    """outs.py:203-205: `u < sigmoid(logit)`, a torch.bool tensor, with one uniform
    per element from `philox_uniform(seed, offset)` or the caller's `uniform`
    (float32, the logit's shape).  Composed torch ops: not a hot path."""
    offset = _check_counter('Binary.sample', 'offset', offset)
    logit = self.logit.detach()
    if uniform is None:
      seed = _check_counter('Binary.sample', 'seed', seed)
      uniform = philox_uniform(seed, offset, 0, logit.numel(), logit.device).view(logit.shape)
    elif not (torch.is_tensor(uniform) and uniform.dtype == torch.float32 and uniform.device == logit.device
              and uniform.shape == logit.shape):
      raise TypeError(f'Binary.sample: uniform must be a float32 tensor of shape {tuple(logit.shape)} on {logit.device}')
    return uniform < torch.sigmoid(logit.to(torch.float32))


# ---- Normal: the actor's continuous policy, its logp, entropy, loss and draw ----

# What the kernels take: a row of at most 256 action dimensions stays in one
# wave's registers, indices are 32-bit.  Structural, not a crossover: the fused
# median is below the composed one at all 48 rows of profiles/normal_policy_bench.txt
# (N 1024 and 16 384, T 16, A 1, 6, 21 and 38, float32 and bfloat16, forward,
# forward + backward and sample), so no size constant sits beside `_normal_path`;
# the figures are quoted there.
NORMAL_MAX_ACTIONS = 256
NORMAL_MAX_ELEMENTS = 2 ** 31 - 1
_NORMAL_KINDS = {'bounded': _lib.NORMAL_BOUNDED, 'logstd': _lib.NORMAL_LOGSTD}
_HALF_LOG_2PI = float(np.float32(0.5 * np.log(2 * np.pi)))
_TWO_PI = float(np.float32(2 * np.pi))


def normal_policy_launches():
  """Kernel launches `emb_normal_policy_loss`, `emb_normal_policy_loss_grad`,
  `emb_normal_sample` and `emb_philox_normal` have issued in this process."""
  return _lib.launches('normal_policy')


def philox_normal(seed, offset=0, first=0, count=1, device=None):
  """(count,) float32 on `device`: the standard normals the sample kernel draws
  for the elements `first .. first + count - 1` -- the Philox4x32-10 block keyed as
  `philox_uniform`'s, u1 = ((word 0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (word 1 >> 8) *
  2^-24, eps = sqrt(-2 ln u1) cos(2 pi u2).  One launch (`emb_philox_normal`);
  count = 0 launches nothing."""
  return _philox(api.emb_philox_normal, 'philox_normal', 'elements', seed, offset, first, count, device)


def _normal_path(fused, rows, actions):
  """True: the kernels, False: the composed path (`normal_policy_loss` says
  when); `rows` counts the inputs' rows, a dropped step's included.  The
  kernels' median was below the composed path's at every shape, dtype and piece
  measured (profiles/normal_policy_bench.txt) -- the closest, (16384, 16, 38)
  bf16: forward 102.0 us against 343.6, forward + backward 231.6 against 795.8,
  sample 47.7 against 156.2; (1024, 16, 6) f32: 23.0 / 126.4, 95.1 / 392.0 and 12.5 /
  43.2 -- so `fused=None` takes them wherever they fit.  Up to (16384, 16, 6) the
  fused figures are the host's enqueue (23 us forward, 95 with autograd's
  backward, 12.5 for the sample) whatever the size."""
  row, index = 1 <= actions <= NORMAL_MAX_ACTIONS, rows * actions <= NORMAL_MAX_ELEMENTS
  if row and index:
    return fused is None or bool(fused)
  return _fused_path(
      'Normal', fused,
      (row, f'{actions} action dimensions, the kernels keep a row of at most {NORMAL_MAX_ACTIONS} in one wave\'s '
            'registers'),
      (index, f'{rows} x {actions} elements, the kernels index 1 .. 2^31 - 1'))


def _check_normal(who, mean_raw, std_raw, kind, minstd, maxstd, dims):
  """(kind id, lo, hi) with lo and hi the float32 values the kernels are handed."""
  _check_device(mean_raw)
  _check_device(std_raw)
  if mean_raw.dtype not in _DTYPES:
    raise TypeError(f'{who}: mean_raw must be float32 or bfloat16, got {mean_raw.dtype}')
  if std_raw.dtype != mean_raw.dtype or std_raw.device != mean_raw.device:
    raise TypeError(f'{who}: mean_raw is {mean_raw.dtype} on {mean_raw.device}, std_raw {std_raw.dtype} on '
                    f'{std_raw.device}')
  if std_raw.shape != mean_raw.shape:
    raise ValueError(f'{who}: mean_raw of shape {tuple(mean_raw.shape)}, std_raw of {tuple(std_raw.shape)}')
  if kind not in _NORMAL_KINDS:
    raise ValueError(f"{who}: kind = {kind!r}, needs 'bounded' or 'logstd'")
  if dims not in (0, 1):
    raise ValueError(f'{who}: dims = {dims!r}, needs 0 (...) or 1 (..., actions); '
                     'flatten more action dimensions into the last axis')
  if mean_raw.dim() < dims or (dims and mean_raw.shape[-1] < 1):
    raise ValueError(f'{who}: inputs of shape {tuple(mean_raw.shape)}, needs (..., actions)')
  lo, hi = float(np.float32(minstd)), float(np.float32(maxstd))
  if kind == 'bounded' and not (0.0 < lo <= hi and np.isfinite(hi)):
    raise ValueError(f'{who}: minstd = {minstd}, maxstd = {maxstd}, bounded needs finite maxstd >= minstd > 0')
  return _NORMAL_KINDS[kind], lo, hi


def _normal_actions(who, act, like):
  """`act` as float32 on the inputs' device, shaped like them; a constant."""
  if not torch.is_tensor(act):
    act = torch.as_tensor(np.asarray(act))
  if not act.dtype.is_floating_point:
    raise TypeError(f'{who}: actions must be floating point (outs.py:175), got {act.dtype}')
  if act.shape != like.shape:
    raise ValueError(f'{who}: actions of shape {tuple(act.shape)}, the inputs need {tuple(like.shape)}')
  return act.detach().to(device=like.device, dtype=torch.float32).contiguous()


def _normal_moments(mean_raw, std_raw, kind, lo, hi):
  """heads.py:150-152 (`bounded_normal`) or heads.py:161 (`normal_logstd`) in
  float32 (outs.py:164-165): (mean, stddev)."""
  m, s = mean_raw.to(torch.float32), std_raw.to(torch.float32)
  if kind == _lib.NORMAL_BOUNDED:
    span = float(np.float32(hi) - np.float32(lo))
    return torch.tanh(m), span * torch.sigmoid(s + 2.0) + lo
  return m, torch.exp(s)


def _composed_normal_logp(mean, std, act, dims):
  """outs.py:174-176 under `Agg.logp` (outs.py:63-64)."""
  z = (act - mean) / std
  logp = -(z * z) * 0.5 - torch.log(std) - _HALF_LOG_2PI
  return logp.sum(-1) if dims else logp


def _composed_normal_entropy(std, dims):
  """outs.py:178-179 under `Agg.entropy` (outs.py:69-71)."""
  entropy = 0.5 * torch.log(_TWO_PI * (std * std)) + 0.5
  return entropy.sum(-1) if dims else entropy


class _FusedNormalPolicy(torch.autograd.Function):
  """(loss, logpi, ent), each (N * (T - drop),) float32, on the kernels: one
  launch forward, one backward.  Only `loss` carries a gradient, to both raw inputs."""

  @staticmethod
  def forward(ctx, mean_raw, std_raw, act, adv, weight, stride, geometry, head, actent):
    n, t, drop, actions = geometry
    m, s = mean_raw.detach().contiguous(), std_raw.detach().contiguous()
    dtype = _DTYPES[m.dtype]
    loss, logpi, ent = _lib.empty((3, n * (t - drop)), torch.float32, m.device).unbind(0)
    api.emb_normal_policy_loss(
        m.data_ptr(), s.data_ptr(), _address(act), dtype, n, t, drop, actions, *head, actent, _address(adv),
        _address(weight), stride, loss.data_ptr(), logpi.data_ptr(), ent.data_ptr(), _lib.raw_stream(m.device))
    ctx.saved = (m, s, act, adv, weight, stride, geometry, head, actent, dtype, mean_raw.shape)
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(logpi, ent)
    return loss, logpi, ent

  @staticmethod
  @once_differentiable
  def backward(ctx, gout, _logpi, _ent):
    if gout is None:
      return (None,) * 9
    m, s, act, adv, weight, stride, geometry, head, actent, dtype, shape = ctx.saved
    n, t, drop, actions = geometry
    gout = gout.to(torch.float32).contiguous()
    grad_mean, grad_std = torch.empty_like(m), torch.empty_like(s)
    api.emb_normal_policy_loss_grad(
        m.data_ptr(), s.data_ptr(), _address(act), dtype, n, t, drop, actions, *head, actent, _address(adv),
        _address(weight), stride, gout.data_ptr(), grad_mean.data_ptr(), grad_std.data_ptr(), _lib.raw_stream(m.device))
    return (grad_mean.view(shape), grad_std.view(shape)) + (None,) * 7


class Normal:
  """The reference's `Agg(Normal(mean, stddev), dims, sum)` (outs.py:40-76, 161-186)
  as `Head.bounded_normal` and `Head.normal_logstd` build it (heads.py:146-162),
  the continuous policy head, over the two linear layers' raw outputs
  `mean_raw` and `std_raw`, CUDA tensors of float32 or bfloat16 (both the same):

    kind='bounded'  mean = tanh(mean_raw), stddev = (maxstd - minstd) sigmoid(std_raw + 2) + minstd
    kind='logstd'   mean = mean_raw,       stddev = exp(std_raw)
    dims=0          inputs and actions (...): a scalar action per row
    dims=1          inputs and actions (..., actions), `logp` and `entropy` summed over
                    the last axis; more action axes are flattened into it by the caller

  `.logp(act)` and `.entropy()` are (...) float32 and differentiable once with
  respect to both raw inputs; `.pred()` is the mean (composed torch ops, no
  gradient); `.sample(seed)` draws float32 actions without a gradient (`imag_loss`
  takes `sg(act)`, and no loss of the reference uses the reparameterised gradient).
  `.minent` and `.maxent` are heads.py:153-154 summed over the actions, what
  agent.py:440-442 reads (None for 'logstd', which sets neither).  `.kl` is not
  part of this.

  Two paths, as `Categorical`: composed restates the reference line by line in
  torch (the definition, every size); fused is `emb_normal_policy_loss` /
  `emb_normal_policy_loss_grad` / `emb_normal_sample`, at most 256 actions, one
  launch per call and one per backward.  `fused=None` takes the kernels where
  they fit, True / False force a path (True raises where they do not fit, and says
  why).  No rows: the composed path, nothing is launched.  `normal_policy_loss`
  documents the arithmetic and the non-finite inputs."""

  def __init__(self, mean_raw, std_raw, kind='bounded', minstd=1.0, maxstd=1.0, dims=1, fused=None):
    self._head = _check_normal('Normal', mean_raw, std_raw, kind, minstd, maxstd, dims)
    self.mean_raw, self.std_raw = mean_raw, std_raw
    self.kind, self.dims = kind, dims
    self._lead = mean_raw.shape[:mean_raw.dim() - dims]
    self._actions = mean_raw.shape[-1] if dims else 1
    self._rows = int(np.prod(self._lead, dtype=np.int64))
    self.fused = _normal_path(fused, self._rows, self._actions) and self._rows > 0
    if kind == 'bounded':
      _, lo, hi = self._head
      entropy = lambda std: (0.5 * float(np.log(2 * np.pi * std * std)) + 0.5) * self._actions
      self.minent, self.maxent = entropy(lo), entropy(hi)
    else:
      self.minent = self.maxent = None

  def _moments(self):
    return _normal_moments(self.mean_raw, self.std_raw, *self._head)

  def _launch(self, act, actent):
    geometry = (self._rows, 1, 0, self._actions)
    loss = _FusedNormalPolicy.apply(self.mean_raw, self.std_raw, act, None, None, 1, geometry, self._head, actent)[0]
    return loss.view(self._lead)

  def pred(self):
    """outs.py:167-168: the mean, float32, shaped like the inputs."""
    with torch.no_grad():
      return self._moments()[0]

  def sample(self, seed=None, offset=0, eps=None):
    """outs.py:170-172: `mean + stddev * eps`, float32, shaped like the inputs, no
    gradient -- what `logp` and `normal_policy_loss` take as `act`.  `eps` is one
    standard normal per element from `philox_normal(seed, offset)`: element e of
    the flattened inputs takes the Philox block at counter (e, `offset`) under
    key `seed`, so the noise depends on (seed, offset, e) alone, not on the dtype,
    the path or the launch geometry.  `seed` and `offset` are integers in
    [0, 2^64) and travel to the kernel by value: a replayed graph repeats the
    draw it captured.  `eps`, a float32 tensor shaped like the inputs, replaces
    the counter and is read anew on every replay.  On the kernels ONE launch;
    composed draws the same noise with `emb_philox_normal` and uses torch ops."""
    who = 'Normal.sample'
    offset = _check_counter(who, 'offset', offset)
    like = self.mean_raw
    if eps is None:
      seed = _check_counter(who, 'seed', seed)
    else:
      seed = 0 if seed is None else _check_counter(who, 'seed', seed)
      if not (torch.is_tensor(eps) and eps.dtype == torch.float32 and eps.device == like.device):
        raise TypeError(f'{who}: eps must be a float32 tensor on {like.device}')
      if eps.shape != like.shape:
        raise ValueError(f'{who}: eps of shape {tuple(eps.shape)}, needs {tuple(like.shape)}')
      eps = eps.detach().contiguous()
    count = self._rows * self._actions
    if self.fused and count > 0:
      m, s = self.mean_raw.detach().contiguous(), self.std_raw.detach().contiguous()
      act = torch.empty(like.shape, dtype=torch.float32, device=like.device)
      api.emb_normal_sample(
          m.data_ptr(), s.data_ptr(), _DTYPES[m.dtype], self._rows, self._actions, *self._head, seed, offset,
          None if eps is None else eps.data_ptr(), act.data_ptr(), _lib.raw_stream(like.device))
      return act
    with torch.no_grad():
      if eps is None:
        eps = philox_normal(seed, offset, 0, count, like.device).view(like.shape)
      mean, std = self._moments()
      return mean + std * eps

  def logp(self, act):
    """(...) float32: the log-density of `act` (any floating dtype; a constant)."""
    act = _normal_actions('Normal.logp', act, self.mean_raw)
    if self.fused:
      return -self._launch(act, 0.0)              # the launch's loss with adv = weight = 1, actent = 0 is -logp
    mean, std = self._moments()
    return _composed_normal_logp(mean, std, act, self.dims)

  def entropy(self):
    """(...) float32."""
    if self.fused:
      return self._launch(None, -1.0)             # no action and actent = -1: the launch's loss is the entropy
    return _composed_normal_entropy(self._moments()[1], self.dims)


def normal_policy_loss(mean_raw, std_raw, act, adv, weight, actent=3e-4, kind='bounded', minstd=0.1, maxstd=1.0,
                       dims=1, drop_last=True, fused=None):
  """The actor's loss of `imag_loss` (agent.py:411-415) for one continuous action key:

      logpi = policy.logp(sg(act))[:, :-1]
      ent   = policy.entropy()[:, :-1]
      loss  = sg(weight[:, :-1]) * -(logpi * sg(adv) + actent * ent)

  with policy = `Normal(mean_raw, std_raw, kind, minstd, maxstd, dims)`, as a dict
  of three float32 tensors.  Per element, in float32,

      z = (act - mean) / std
      logp_a = -z^2 / 2 - log(std) - log(2 pi) / 2        ent_a = log(2 pi std^2) / 2 + 1 / 2

  `loss` is differentiable once with respect to both raw inputs and to nothing
  else: `act`, `adv` and `weight` are constants, the reference's `sg`.  `logpi`
  and `ent` carry no gradient; they are for `metrics['ent/...']` (agent.py:438-442).

  The inputs are (N.., T[, actions]) and `act` has their shape, in any floating
  dtype (converted to float32; integers raise TypeError).  With `drop_last` the
  last step of every sequence is dropped, the reference's `[:, :-1]`: the outputs
  and `adv` are (N.., T - 1), and `weight` is (N.., T) as `scans.dreamer_targets`
  returns it or (N.., T - 1).  Without it all three are the leading shape of the
  inputs, whatever its rank.  The kernels read the kept rows in place: nothing is
  sliced or copied and a dropped step is not read.

  Two paths, as `Normal`.  On the kernels that is ONE launch forward and ONE
  backward, whose closed form takes 1 - tanh^2(m) from exp(-2 |m|) (autograd's
  1 - tanh(m)^2 loses digits from |m| of about 5 on).  No output rows (N = 0, or
  T = 1 with `drop_last`): nothing is launched and the gradient is zeros.

  Non-finite inputs.  A NaN in `mean_raw`, `std_raw` or `act` of a kept step
  makes that output row's `loss`, `logpi` and `ent` and its gradient rows NaN on
  the kernels and touches no other row; composed is the definition: `logpi` and
  `loss` are NaN, `ent` is where the NaN is in `std_raw` (the entropy does not
  read the mean or the action), and the gradient is what autograd leaves.  The
  same values in a dropped step touch nothing: every output has the bits of the
  clean run and that step's gradient is zeros.  'bounded' stays finite for raw
  values of +-1e4: the stddev is the formula's value at sigmoid = 0 or 1 and the
  gradient to `mean_raw` is exactly 0 on the kernels.  'logstd' returns what the
  float32 definition returns when `exp` overflows (+-inf or NaN), confined to the row."""
  who = 'normal_policy_loss'
  head = _check_normal(who, mean_raw, std_raw, kind, minstd, maxstd, dims)
  lead = mean_raw.shape[:mean_raw.dim() - dims]
  actions = mean_raw.shape[-1] if dims else 1
  actent, n, t, drop, kept, out_shape = _loss_frame(who, 'inputs', mean_raw, lead, actent, drop_last)
  act = _normal_actions(who, act, mean_raw)
  adv = _loss_constant(who, 'adv', adv, (out_shape,), mean_raw.device)
  weight = _loss_constant(who, 'weight', weight, (out_shape, tuple(lead)), mean_raw.device)
  if _normal_path(fused, n * t, actions) and n * kept > 0:
    stride, geometry = weight.shape[-1] if drop else 1, (n, t, drop, actions)
    loss, logpi, ent = _FusedNormalPolicy.apply(mean_raw, std_raw, act, adv, weight, stride, geometry, head, actent)
    return {'loss': loss.view(out_shape), 'logpi': logpi.view(out_shape), 'ent': ent.view(out_shape)}
  weight, mean_raw, std_raw, act = _kept_steps(lead, drop, kept, weight, mean_raw, std_raw, act)
  mean, std = _normal_moments(mean_raw, std_raw, *head)
  return _composed_loss(_composed_normal_logp(mean, std, act, dims), _composed_normal_entropy(std, dims), adv, weight,
                        actent)


# ------------------------------------------------------------ the loss total --
# The largest loss (elements) up to which `total_loss(fused=None)` takes the
# kernels: one workgroup reduces one loss, and one more reduces all of them again
# for the total.  At both shapes of profiles/stat_metrics_bench.txt the fused
# median is below the composed one -- K = 10 at (16, 64): forward 33.8 us against
# 135.1 (1 device operation against 30), forward + backward 193.8 against 491.3 (3
# against 51); at (64, 64): 36.9 against 164.5 and 127.9 against 396.4; every fused
# figure is the host's enqueue time -- so the constant stays at what the kernels
# index.  Nothing larger was measured.
TOTAL_LOSS_FUSED_MAX = 2 ** 31 - 1
TOTAL_LOSS_MAX_ELEMENTS = 2 ** 31 - 1


def stat_rows_launches():
  """Kernel launches `emb_stat_rows` and `emb_mean_fill` have issued in this process."""
  return _lib.launches('stat_rows')


def _total_loss_path(fused, float32, contiguous, count, smallest, largest):
  """True: the kernels, False: the composed path (`total_loss` says when).
  `float32`: every loss is a float32 CUDA tensor; `contiguous`: every one is;
  `count` losses of `smallest` .. `largest` elements."""
  fits = _fused_path(
      'total_loss', fused,
      (float32, 'the kernels read float32 CUDA tensors'),
      (contiguous, 'the kernels read and write contiguous tensors'),
      (count <= _lib.STAT_MAX_ENTRIES,
       f'{count} losses, the total is formed by one launch of at most {_lib.STAT_MAX_ENTRIES} entries'),
      (smallest >= 1, 'a loss without elements (its mean is NaN)'),
      (largest <= TOTAL_LOSS_MAX_ELEMENTS, f'a loss of {largest} elements, the kernels index at most 2^31 - 1'))
  if fused is None:
    return fits and largest <= TOTAL_LOSS_FUSED_MAX
  return fits


class _FusedTotal(torch.autograd.Function):
  """(total, stats (K, 6)) of K losses: one launch forward (`emb_stat_rows` with
  its total), one backward (`emb_mean_fill`).  Only `total` carries a gradient."""

  @staticmethod
  def forward(ctx, scales, *losses):
    device = losses[0].device
    count = len(losses)
    flat = _lib.empty((count * _lib.STAT_VALUES + 1,), torch.float32, device)
    stats, total = flat[:-1].view(count, _lib.STAT_VALUES), flat[-1]
    table = (_lib.StatEntry * count)()
    for entry, scale, v in zip(table, scales, losses):
      n = v.numel()
      entry.x, entry.rows, entry.cols, entry.stride, entry.weight = v.data_ptr(), 1, n, n, scale
    _lib.fast.emb_stat_rows(table, count, stats.data_ptr(), total.data_ptr(), _lib.raw_stream(device))
    ctx.saved = (scales, [v.shape for v in losses], device)
    ctx.set_materialize_grads(False)
    ctx.mark_non_differentiable(stats)
    return total, stats

  @staticmethod
  @once_differentiable
  def backward(ctx, gout, _stats):
    scales, shapes, device = ctx.saved
    wanted = [k for k, need in enumerate(ctx.needs_input_grad[1:]) if need]
    if gout is None or not wanted:
      return (None,) * (1 + len(shapes))
    gout = gout.to(torch.float32).contiguous()
    # one allocation; every gradient starts on a 16-byte boundary (the kernel's wide stores)
    sizes = [(shapes[k].numel() + 3) // 4 * 4 for k in wanted]
    flat = _lib.empty((sum(sizes),), torch.float32, device)
    table = (_lib.FillEntry * len(wanted))()
    grads, start = [None] * len(shapes), 0
    for entry, k, size in zip(table, wanted, sizes):
      n = shapes[k].numel()
      grads[k] = flat[start:start + n].view(shapes[k])
      entry.out, entry.n, entry.scale = grads[k].data_ptr(), n, scales[k]
      start += size
    _lib.fast.emb_mean_fill(table, len(wanted), gout.data_ptr(), _lib.raw_stream(device))
    return (None, *grads)


def total_loss(losses, scales, fused=None):
  """The end of Agent.loss (dreamerv3/agent.py:237-240) -> (loss, metrics):
  metrics[f'loss/{k}'] = losses[k].mean(), detached, and loss =
  sum([losses[k].mean() * scales[k] ...]) -- a 0-d float32 with autograd, the
  products added in dict order in float32 from 0, as Python's `sum` does.
  `losses` is a dict of tensors of any shape, `scales` a dict of numbers with the
  same keys (ValueError otherwise: the reference's assert, agent.py:237).
  Two paths compute it:
    composed  torch's `mean`, multiply and add: every dtype, every layout.  The
              definition.
    fused     float32 contiguous CUDA losses, at most 48 of them: ONE launch
              forward (a workgroup per loss writes its mean; one more reduces
              every loss again and adds the products, so no result depends on the
              order in which workgroups finish) and ONE backward, which writes
              (g * scales[k]) / n_k into every loss's gradient.  The metrics are
              views of the launch's result buffer, which this call allocates.
  `fused=None` takes the kernels where they fit and no loss is larger than
  TOTAL_LOSS_FUSED_MAX; True / False force a path (True raises where they do not
  fit, and says why).  A NaN or infinity in one loss shows in its own `loss/{k}`
  and in the total, and in nothing else."""
  if set(losses) != set(scales):
    raise ValueError(f'total_loss: losses {sorted(losses)} and scales {sorted(scales)} do not have the same keys')
  if not losses:
    raise ValueError('total_loss: no losses')
  values = list(losses.values())
  float32 = all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32 for v in values)
  sizes = [v.numel() for v in values]
  if not _total_loss_path(fused, float32, all(v.is_contiguous() for v in values), len(values), min(sizes), max(sizes)):
    means = {k: v.mean() for k, v in losses.items()}
    loss = sum([means[k] * scales[k] for k in losses])
    return loss, {f'loss/{k}': mean.detach() for k, mean in means.items()}
  weights = tuple(float(np.float32(scales[k])) for k in losses)
  total, stats = _FusedTotal.apply(weights, *values)
  return total, {f'loss/{k}': stats[index, 0] for index, k in enumerate(losses)}
