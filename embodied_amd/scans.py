"""Return scans on device (float32): GAE (ppo/agent.py:188-201), lambda-return
(dreamerv3/agent.py:482-490, over flags and over float continuation
probabilities) and the Director critic target (director/agent.py:430-445), each
one kernel launch; the PPO targets (ppo/agent.py:188-210: GAE with both return
normalisers) and DreamerV3's imagination targets (dreamerv3/agent.py:397-419:
lambda-return, weight and three return normalisers) as one launch each.

Inputs are torch CUDA tensors; bool flags may be torch.bool or uint8.
"""
import collections
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import api, fast


def _stream(t):
  return _lib.raw_stream(t.device)


_ROUNDED = {}


def _round32(x):
  """x rounded to float32 (what the float32 reference computes with), as a
  Python float; the handful of hyper-parameter values is remembered."""
  try:
    return _ROUNDED[x]
  except KeyError:
    if len(_ROUNDED) > 1024:
      _ROUNDED.clear()
    value = _ROUNDED[x] = float(np.float32(x))
    return value


# A tensor OBJECT that passed `_f32` / `_flag` for a device keeps a mark (the
# replay hands out the same output tensors again once nobody holds them, a
# critic's value buffer is often one tensor): the next call recognises it with
# one attribute read instead of four calls into torch.  dtype, device and
# strides of a tensor do not change behind its back (short of resize_ / set_).
_F32_OK, _FLAG_OK = {}, {}


def _mark(table, device):
  mark = table.get(device)
  if mark is None:
    mark = table[device] = (device,)
  return mark


def _f32(x, device):
  if type(x) is torch.Tensor:
    mark = _mark(_F32_OK, device)
    if getattr(x, '_emb_f32', None) is mark:
      return x
    if x.dtype == torch.float32 and x.device == device and x.is_contiguous():
      x._emb_f32 = mark
      return x
  if torch.is_tensor(x) and x.dtype == torch.float32 and x.device == device and x.is_contiguous():
    return x
  if not torch.is_tensor(x):
    x = torch.as_tensor(np.asarray(x))
  return x.to(device=device, dtype=torch.float32).contiguous()


def _flag(x, device):
  """bool / uint8 flags as a contiguous 1-byte tensor on `device` (the kernels
  read the bytes; torch.bool is one byte per element)."""
  if type(x) is torch.Tensor:
    mark = _mark(_FLAG_OK, device)
    if getattr(x, '_emb_flag', None) is mark:
      return x
    if (x.device == device and x.is_contiguous()
        and (x.dtype == torch.bool or x.dtype == torch.uint8)):
      x._emb_flag = mark
      return x
  if (torch.is_tensor(x) and x.device == device and x.is_contiguous()
      and (x.dtype == torch.bool or x.dtype == torch.uint8)):
    return x
  if not torch.is_tensor(x):
    x = torch.as_tensor(np.asarray(x))
  if x.dtype != torch.bool and x.dtype != torch.uint8:
    x = x != 0
  return x.to(device).contiguous()


def _device(*xs):
  for x in xs:
    if torch.is_tensor(x) and x.is_cuda:
      return x.device
  raise RuntimeError(
      'embodied_amd.scans run as HIP kernels: pass CUDA tensors (no CPU fallback)')


def _pair(B, n, dev):
  """Two fresh (B, n) float32 results out of one (2, B, n) allocation (`out=`
  is the form without an allocation)."""
  return _lib.empty((2, B, n), torch.float32, dev).unbind(0)


def gae(rew, val, last, term, hor=200, lam=0.8, out=None):
  """adv_t = delta_t + live_t*cont_t*adv_{t+1}; tar = adv + val[:, :-1].
  rew, val (B,T) f32; last, term (B,T) bool -> adv, tar (B,T-1).
  `out=(adv, tar)`: write into the caller's contiguous float32 (B,T-1) tensors."""
  dev = _device(rew, val, last, term)
  rew, val = _f32(rew, dev), _f32(val, dev)
  last, term = _flag(last, dev), _flag(term, dev)
  B, T = rew.shape
  assert val.shape == last.shape == term.shape == (B, T)
  if out is not None:
    adv, tar = out
    for result in (adv, tar):
      # (a tensor object that passed for this shape and device keeps a mark, like
      # the inputs: an agent hands the same few result tensors in again)
      if result.__dict__.get('_emb_gae_out') == (B, T, dev):
        continue
      if (result.dtype != torch.float32 or tuple(result.shape) != (B, T - 1) or result.device != dev
          or not result.is_contiguous()):
        raise ValueError(f'gae(out=): needs contiguous float32 {(B, T - 1)} tensors on {dev}')
      result._emb_gae_out = (B, T, dev)
  elif B * T <= 1 << 20:
    adv, tar = _pair(B, T - 1, dev)                         # one allocation, two views
  else:       # bandwidth-bound sizes: two write streams a power-of-two-ish distance apart
    adv = _lib.empty((B, T - 1), torch.float32, dev)        # collide on HBM channels (-19 %)
    tar = _lib.empty((B, T - 1), torch.float32, dev)
  if B == 0 or T < 2:
    return adv, tar                   # nothing to scan: (B, 0) results
  fast.emb_scan_gae(
      rew.data_ptr(), val.data_ptr(), last.data_ptr(), term.data_ptr(), B, T,
      _round32(1 - 1 / hor), _round32(lam), adv.data_ptr(),
      tar.data_ptr(), _stream(rew))
  return adv, tar


class PpoTargets(collections.namedtuple('PpoTargets', 'adv tar tar_normed adv_normed')):
  """What the top of ppo_loss hands on: adv, tar (B,T-1), the clipped normalised
  target padded to (B,T), the normalised advantage (B,T-1)."""


# B * T up to which `ppo_targets(fused=None)` takes the one-workgroup kernel:
# the largest size of profiles/ppo_targets_bench.txt at which it still beat the
# composed path (16 384 values: 19.8 us against 35.3 at (1024, 16), 17.5 against
# 41.1 at (16, 1024); 7.0 against 40.1 at PPO's (16, 64)).  The next measured size,
# (4096, 64), loses 272 us to 132: between the two nothing was measured.
PPO_TARGETS_FUSED_MAX = 16384


def ppo_targets_launches():
  """Kernel launches `emb_ppo_targets` has issued in this process."""
  return _lib.launches('ppo_targets')


def _ppo_targets_path(fused, valnorm, advnorm, B, T):
  """True: the kernel, False: the composed path (`ppo_targets` says when)."""
  meanstd = valnorm.impl == 'meanstd' and advnorm.impl == 'meanstd'
  if fused and not meanstd:
    raise ValueError(
        f"ppo_targets(fused=True): the kernel runs 'meanstd' normalisers, got valnorm "
        f"'{valnorm.impl}' and advnorm '{advnorm.impl}' (fused=None or False composes them)")
  if fused is None:
    return meanstd and B * T <= PPO_TARGETS_FUSED_MAX
  return bool(fused)


def ppo_targets(rew, pred, last, term, valnorm, advnorm, hor=200, lam=0.8, tarclip=10.0,
                update=True, out=None, fused=None):
  """The top of ppo_loss (ppo/agent.py:188-210): val = pred * vscale + voffset
  with valnorm's statistics before the step, GAE, `valnorm(tar, update)`, the
  target normalised, clipped to +-tarclip (None / 0: no clip) and padded with a
  zero column, `advnorm(adv, update)`, the advantage normalised.
  rew, pred (B,T) f32; last, term (B,T) bool; valnorm, advnorm: `DeviceNormalize`
  -> PpoTargets(adv, tar (B,T-1), tar_normed (B,T), adv_normed (B,T-1)).

  Afterwards both normalisers hold what `valnorm.stats()`, `valnorm(tar)` and
  `advnorm(adv)` would have left.  Two paths compute it:
    composed  torch's multiply-add, `gae`, `valnorm.normalize`, torch's clip and
              pad, `advnorm.normalize`: every impl, every size.  The definition.
    fused     ONE launch of one workgroup (`emb_ppo_targets`): both impls 'meanstd'.
  `fused=None` takes the kernel where it is the faster one (both 'meanstd',
  B * T <= PPO_TARGETS_FUSED_MAX), True / False force a path (True raises unless
  both are 'meanstd').  `out=(adv, tar, tar_normed, adv_normed)`: the caller's
  contiguous float32 tensors; without it one allocation holds all four."""
  dev = _device(rew, pred, last, term)
  rew, pred = _f32(rew, dev), _f32(pred, dev)
  last, term = _flag(last, dev), _flag(term, dev)
  B, T = rew.shape
  assert pred.shape == last.shape == term.shape == (B, T)
  fused = _ppo_targets_path(fused, valnorm, advnorm, B, T)
  n = max(T - 1, 0)
  shapes = ((B, n), (B, n), (B, T), (B, n))
  if out is not None:
    results = tuple(out)
    if len(results) != 4:
      raise ValueError('ppo_targets(out=): needs (adv, tar, tar_normed, adv_normed)')
    for result, shape in zip(results, shapes):
      if torch.is_tensor(result) and result.__dict__.get('_emb_ppo_out') == (shape, dev):
        continue          # (marked like gae's: an agent hands the same result tensors in again)
      if (not torch.is_tensor(result) or result.dtype != torch.float32 or tuple(result.shape) != shape
          or result.device != dev or not result.is_contiguous()):
        raise ValueError(
            f'ppo_targets(out=): needs contiguous float32 tensors of shapes {shapes} on {dev}')
      result._emb_ppo_out = (shape, dev)
  else:
    # one allocation; every part starts on a 16-byte boundary (the kernel's wide path)
    sizes = [(rows * cols + 3) // 4 * 4 for rows, cols in shapes]
    flat = _lib.empty((sum(sizes),), torch.float32, dev)
    results, start = [], 0
    for size, (rows, cols) in zip(sizes, shapes):
      results.append(flat[start:start + rows * cols].view(rows, cols))
      start += size
    results = tuple(results)
  adv, tar, tar_normed, adv_normed = results
  if B == 0 or T < 2:
    tar_normed.zero_()
    return PpoTargets(adv, tar, tar_normed, adv_normed)
  if fused:
    vconfig, vstate = valnorm.fused(dev)
    aconfig, astate = advnorm.fused(dev)
    fast.emb_ppo_targets(
        vconfig, aconfig, rew.data_ptr(), pred.data_ptr(), last.data_ptr(), term.data_ptr(), B, T,
        _round32(1 - 1 / hor), _round32(lam), _round32(tarclip) if tarclip else 0.0, int(bool(update)),
        adv.data_ptr(), tar.data_ptr(), tar_normed.data_ptr(), adv_normed.data_ptr(), vstate, astate,
        _stream(rew))
    return PpoTargets(adv, tar, tar_normed, adv_normed)
  voffset, vscale = valnorm.latest()
  val = pred * vscale + voffset
  gae(rew, val, last, term, hor, lam, out=(adv, tar))
  normed = tar_normed[:, :-1]
  normed.copy_(valnorm.normalize(tar, update=update))
  if tarclip:
    normed.clamp_(-tarclip, tarclip)
  tar_normed[:, -1].zero_()
  advnorm.normalize(adv, out=adv_normed, update=update)
  return PpoTargets(adv, tar, tar_normed, adv_normed)


def lambda_return(last, term, rew, val, boot, disc, lam):
  """ret_t = interm_t + live_t*cont_t*ret_{t+1}, seeded with boot[:, -1].
  All (B,T) -> (B,T-1).  `val` is only shape-checked, as in the reference.
  `last` and `term` are flags only (anything not zero is set); float
  continuation probabilities (imag_loss's term = 1 - con) go to `lambda_return_cont`."""
  dev = _device(rew, boot, last, term)
  rew, boot = _f32(rew, dev), _f32(boot, dev)
  last, term = _flag(last, dev), _flag(term, dev)
  B, T = rew.shape
  assert boot.shape == last.shape == term.shape == (B, T)
  assert val is None or tuple(val.shape) == (B, T)
  ret = _lib.empty((B, T - 1), torch.float32, dev)
  if B == 0 or T < 2:
    return ret
  fast.emb_scan_lambda(
      last.data_ptr(), term.data_ptr(), rew.data_ptr(), boot.data_ptr(), B, T,
      _round32(disc), _round32(lam), ret.data_ptr(),
      _stream(rew))
  return ret


def lambda_return_cont(rew, con, boot, disc, lam, out=None):
  """The lambda-return as imag_loss calls it (dreamerv3/agent.py:401-405): last = 0
  and term = 1 - con with `con` the continue head's float probability, so
  live_t = (1 - (1 - con_t)) * disc and cont_t = lam; seeded with boot[:, -1].
  rew, con, boot (B,T) f32 -> ret (B,T-1).  `out=ret`: write into the caller's
  contiguous float32 (B,T-1) tensor."""
  dev = _device(rew, con, boot)
  rew, con, boot = _f32(rew, dev), _f32(con, dev), _f32(boot, dev)
  B, T = rew.shape
  assert con.shape == boot.shape == (B, T)
  if out is not None:
    ret = out
    if not (torch.is_tensor(ret) and ret.__dict__.get('_emb_cont_out') == (B, T, dev)):
      if (not torch.is_tensor(ret) or ret.dtype != torch.float32 or tuple(ret.shape) != (B, max(T - 1, 0))
          or ret.device != dev or not ret.is_contiguous()):
        raise ValueError(f'lambda_return_cont(out=): needs a contiguous float32 {(B, T - 1)} tensor on {dev}')
      ret._emb_cont_out = (B, T, dev)
  else:
    ret = _lib.empty((B, max(T - 1, 0)), torch.float32, dev)
  if B == 0 or T < 2:
    return ret                        # nothing to scan: a (B, 0) result
  fast.emb_scan_lambda_cont(
      rew.data_ptr(), con.data_ptr(), boot.data_ptr(), B, T, _round32(disc), _round32(lam), ret.data_ptr(),
      _stream(rew))
  return ret


class DreamerTargets(collections.namedtuple('DreamerTargets', 'ret weight adv adv_normed tar_padded')):
  """What the top of imag_loss hands on: ret (N,T-1), weight (N,T), adv and
  adv_normed (N,T-1), the normalised target padded to (N,T)."""


# N * (T-1) up to which `dreamer_targets(fused=None)` takes the one-workgroup
# kernel.  16 384 is structural: the returns' sort keys in one workgroup's LDS
# (csrc/normalize.h kNormLdsMax).  The kernel beat the composed path at every
# size of profiles/dreamer_targets_bench.txt up to it, every round of one below
# every round of the other: 39.9 us against 158.2 at (1024, 16), 43.1 against
# 164.8 at (1024, 17) = 16 384 returns, 11.4 against 179.1 at (16, 16), 52.6
# against 7 094 at (16, 1024).  So the constant stays at the limit.
DREAMER_TARGETS_FUSED_MAX = 16384


def dreamer_targets_launches():
  """Kernel launches `emb_dreamer_targets` has issued in this process."""
  return _lib.launches('dreamer_targets')


def _dreamer_targets_path(fused, retnorm, valnorm, advnorm, N, T):
  """True: the kernel, False: the composed path (`dreamer_targets` says when)."""
  impls = (retnorm.impl == 'perc' and valnorm.impl in ('meanstd', 'none')
           and advnorm.impl in ('meanstd', 'none'))
  size = N * max(T - 1, 0) <= 16384            # one workgroup's LDS, whatever the crossover
  if fused and not impls:
    raise ValueError(
        f"dreamer_targets(fused=True): the kernel runs a 'perc' retnorm with 'meanstd' or 'none' valnorm and "
        f"advnorm, got '{retnorm.impl}', '{valnorm.impl}' and '{advnorm.impl}' (fused=None or False composes them)")
  if fused and not size:
    raise ValueError(
        f'dreamer_targets(fused=True): {N} x {T - 1} = {N * (T - 1)} returns, the kernel keeps at most 16384 '
        f'in one workgroup (fused=None or False composes them)')
  if fused is None:
    return impls and N * max(T - 1, 0) <= min(DREAMER_TARGETS_FUSED_MAX, 16384)
  return bool(fused)


_DISC = {}


def _disc_tensor(disc, dev):
  """`disc` as a 0-d float32 tensor on `dev`: torch divides by a tensor, but
  multiplies by the reciprocal of a Python number (one more rounding)."""
  key = (disc, dev)
  tensor = _DISC.get(key)
  if tensor is None:
    if len(_DISC) > 64:
      _DISC.clear()
    tensor = _DISC[key] = torch.tensor(disc, dtype=torch.float32, device=dev)
  return tensor


def _cumprod_rows(x):
  """cumprod(x, 1) with the products taken left to right, one float32 rounding
  each -- numpy.cumprod's order, which torch.cumprod's parallel scan does not
  promise: T-1 dependent column multiplies."""
  out = torch.empty_like(x)
  if x.shape[1]:
    out[:, 0].copy_(x[:, 0])
  for t in range(1, x.shape[1]):
    torch.mul(out[:, t - 1], x[:, t], out=out[:, t])
  return out


def dreamer_targets(rew, con, pred, retnorm, valnorm, advnorm, contdisc=True, horizon=333, lam=0.95,
                    update=True, out=None, fused=None):
  """The top of imag_loss (dreamerv3/agent.py:397-419): tarval = pred * vscale +
  voffset with valnorm's statistics before the step, weight = cumprod(disc * con)
  / disc, the lambda-return with term = 1 - con, `retnorm(ret, update)`,
  adv = (ret - tarval[:, :-1]) / rscale, `advnorm(adv, update)`, the advantage
  normalised, `valnorm(ret, update)`, the return normalised and padded with a
  zero column.  disc = 1 with `contdisc`, else 1 - 1 / horizon.
  rew, con, pred (N,T) f32 -- `con` the continue head's probability, `pred` the
  prediction that serves as the target value (`slowvalue.pred()` with slowtar,
  else `value.pred()`); retnorm, valnorm, advnorm: `DeviceNormalize`
  -> DreamerTargets(ret (N,T-1), weight (N,T), adv, adv_normed (N,T-1), tar_padded (N,T)).

  Afterwards the three normalisers hold what `retnorm(ret)`, `advnorm(adv)` and
  `valnorm(ret)` would have left.  Two paths compute it:
    composed  torch's multiply-add, column multiplies for the weight,
              `lambda_return_cont`, `retnorm.normalize(ret, sub=tarval[:, :-1])`,
              `advnorm.normalize`, `valnorm.normalize`, torch's pad: every impl,
              every size.  The definition.
    fused     ONE launch of one workgroup (`emb_dreamer_targets`): retnorm 'perc',
              valnorm and advnorm 'meanstd' or 'none', N * (T-1) <= 16 384.
  `fused=None` takes the kernel where the impls fit and
  N * (T-1) <= DREAMER_TARGETS_FUSED_MAX, True / False force a path (True raises
  where the impls or the size do not fit, and says which).
  `out=(ret, weight, adv, adv_normed, tar_padded)`: the caller's contiguous
  float32 tensors; without it one allocation holds all five."""
  dev = _device(rew, con, pred)
  rew, con, pred = _f32(rew, dev), _f32(con, dev), _f32(pred, dev)
  N, T = rew.shape
  assert con.shape == pred.shape == (N, T)
  fused = _dreamer_targets_path(fused, retnorm, valnorm, advnorm, N, T)
  n = max(T - 1, 0)
  shapes = ((N, n), (N, T), (N, n), (N, n), (N, T))
  if out is not None:
    results = tuple(out)
    if len(results) != 5:
      raise ValueError('dreamer_targets(out=): needs (ret, weight, adv, adv_normed, tar_padded)')
    for result, shape in zip(results, shapes):
      if torch.is_tensor(result) and result.__dict__.get('_emb_dreamer_out') == (shape, dev):
        continue          # (marked like gae's: an agent hands the same result tensors in again)
      if (not torch.is_tensor(result) or result.dtype != torch.float32 or tuple(result.shape) != shape
          or result.device != dev or not result.is_contiguous()):
        raise ValueError(
            f'dreamer_targets(out=): needs contiguous float32 tensors of shapes {shapes} on {dev}')
      result._emb_dreamer_out = (shape, dev)
  else:
    # one allocation; every part starts on a 16-byte boundary (the kernel's wide path)
    sizes = [(rows * cols + 3) // 4 * 4 for rows, cols in shapes]
    flat = _lib.empty((sum(sizes),), torch.float32, dev)
    results, start = [], 0
    for size, (rows, cols) in zip(sizes, shapes):
      results.append(flat[start:start + rows * cols].view(rows, cols))
      start += size
    results = tuple(results)
  ret, weight, adv, adv_normed, tar_padded = results
  disc = 1.0 if contdisc else _round32(1 - 1 / horizon)
  if N == 0 or T < 2:
    if N and T:           # one column: nothing to scan, the weight is its first factor
      weight.copy_(con if disc == 1.0 else (con * disc) / _disc_tensor(disc, dev))
    tar_padded.zero_()
    return DreamerTargets(ret, weight, adv, adv_normed, tar_padded)
  if fused:
    rconfig, rstate = retnorm.fused(dev)
    vconfig, vstate = valnorm.fused(dev)
    aconfig, astate = advnorm.fused(dev)
    fast.emb_dreamer_targets(
        rconfig, vconfig, aconfig, rew.data_ptr(), con.data_ptr(), pred.data_ptr(), N, T, disc, _round32(lam),
        int(bool(update)), ret.data_ptr(), weight.data_ptr(), adv.data_ptr(), adv_normed.data_ptr(),
        tar_padded.data_ptr(), rstate, vstate, astate, _stream(rew))
    return DreamerTargets(ret, weight, adv, adv_normed, tar_padded)
  voffset, vscale = valnorm.latest()
  tarval = pred * vscale + voffset
  if disc == 1.0:         # (x * 1 and x / 1 are x)
    weight.copy_(_cumprod_rows(con))
  else:
    torch.div(_cumprod_rows(con * disc), _disc_tensor(disc, dev), out=weight)
  lambda_return_cont(rew, con, tarval, disc, lam, out=ret)
  retnorm.normalize(ret, sub=tarval[:, :-1].contiguous(), out=adv, update=update)
  advnorm.normalize(adv, out=adv_normed, update=update)
  tar_padded[:, :-1].copy_(valnorm.normalize(ret, update=update))
  tar_padded[:, -1].zero_()
  return DreamerTargets(ret, weight, adv, adv_normed, tar_padded)


# The largest array (elements) up to which `imag_metrics(fused=None)` takes the
# kernel.  An entry is reduced by ONE workgroup, so a large array could lose to
# torch's many; at every shape of profiles/stat_metrics_bench.txt the fused median
# is below the composed one -- (16, 16) 26.1 us against 210.3, (1024, 16) 22.6
# against 187.7, (1024, 17) 20.9 against 137.3, and (4096, 16), past what
# `dreamer_targets` fuses, 24.4 against 204.4 (31 device operations composed, 1
# fused; the fused figure is the host's enqueue time at all but the last) -- so
# the constant stays at what the kernel indexes.  Nothing larger was measured.
IMAG_METRICS_FUSED_MAX = 2 ** 31 - 1
IMAG_METRICS = ('adv', 'adv_std', 'adv_mag', 'rew', 'con', 'ret', 'val', 'tar', 'weight', 'slowval',
                'ret_min', 'ret_max', 'ret_rate')


def _imag_metrics_path(fused, float32, views, largest):
  """True: the kernel, False: the composed path (`imag_metrics` says when).
  `float32`: every input is a float32 CUDA tensor; `views`: every one is a matrix
  view `emb_stat_rows` takes; `largest`: the elements of the largest of them."""
  from . import outs
  fits = outs._fused_path(
      'imag_metrics', fused,
      (float32, 'the kernel reads float32 CUDA tensors'),
      (views, 'the kernel reads arrays that are contiguous, or 2-D with unit column stride'),
      (largest <= 2 ** 31 - 1, f'an array of {largest} elements, the kernel indexes at most 2^31 - 1'))
  if fused is None:
    return fits and largest <= IMAG_METRICS_FUSED_MAX
  return fits


_STAT_PAIRS, _IMAG_PLANS = {}, {}


def _constant_pair(offset, scale, dev):
  """(offset, scale) as a float32 pair on `dev`, uploaded once per value."""
  key = (offset, scale, dev)
  pair = _STAT_PAIRS.get(key)
  if pair is None:
    if len(_STAT_PAIRS) > 256:
      _STAT_PAIRS.clear()
    pair = _STAT_PAIRS[key] = torch.tensor([offset, scale], dtype=torch.float32, device=dev)
  return pair


def _device_pair(offset, scale, dev):
  """The (offset, scale) of an affine entry: None for the constants (0, 1), else a
  float32 tensor on `dev` that holds the two side by side -- two 0-d views of
  neighbouring words (a clone of `DeviceNormalize`'s state words 3-4) as they
  are, anything else packed by one torch op."""
  if torch.is_tensor(offset) or torch.is_tensor(scale):
    if (torch.is_tensor(offset) and torch.is_tensor(scale) and offset.device == dev and scale.device == dev
        and offset.dtype == scale.dtype == torch.float32 and offset.numel() == scale.numel() == 1
        and scale.data_ptr() == offset.data_ptr() + 4):
      return torch.as_strided(offset, (2,), (1,))
    parts = [torch.as_tensor(v, dtype=torch.float32, device=dev).reshape(()) for v in (offset, scale)]
    return torch.stack(parts)
  offset, scale = float(offset), float(scale)
  if offset == 0.0 and scale == 1.0:
    return None
  return _constant_pair(offset, scale, dev)


def imag_metrics(targets, rew, con, val_pred, slow_pred, retnorm, vstats=None, ents=None, entlimits=None,
                 fused=None):
  """The metrics of imag_loss (dreamerv3/agent.py:424-442) -> {name: 0-d float32}:
  adv, adv_std (population), adv_mag; rew, con, weight; ret, ret_min, ret_max and
  ret_rate of ret_normed = (ret - roffset) / rscale; val and slowval, the means of
  pred * vscale + voffset; tar, the mean of `tar_padded[:, :-1]`; and per action
  key `ent/{k}`, the mean of `ents[k][:, :-1]`, with `rand/{k}` =
  (ent - minent) / (maxent - minent) where `entlimits` has the key.

  targets   the `DreamerTargets` of the same train step
  rew, con, val_pred, slow_pred  (N, T): `value.pred()` and `slowvalue.pred()`
  retnorm   the `DeviceNormalize` that `dreamer_targets` just stepped: its
            (offset, scale) is what `retnorm(ret, update)` returned, read from the
            state words ON THE DEVICE; 'none' is the constants (0, 1)
  vstats    valnorm's (voffset, vscale) from BEFORE the step (agent.py:397), as
            floats or 0-d device tensors; None is (0, 1), the shipped
            `valnorm: none`.  `dreamer_targets` overwrites a 'meanstd' valnorm's
            words in place: a caller with one must CLONE `valnorm.latest()`
            before calling `dreamer_targets`, and pass the clones
  ents      {key: (N, T) float32 entropy}; the `[:, :-1]` is taken by stride
  entlimits {key: (minent, maxent)}

  T < 2 or N = 0 raises ValueError (the reference would take means of nothing).
  Two paths compute it:
    composed  torch ops, one by one as the reference writes them: every dtype,
              every layout.  The definition.
    fused     ONE launch of `emb_stat_rows` for up to 48 entries (8 arrays, one
              more per key and one more per key with limits; more keys: further
              launches); float32 inputs.  `rand/{k}` is the mean of
              (ent - minent) / (maxent - minent), a second entry over the same
              array, so it costs no launch.
  `fused=None` takes the kernel where it fits and no array is larger than
  IMAG_METRICS_FUSED_MAX; True / False force a path (True raises where it does
  not fit, and says why).  The fused results are 0-d VIEWS of one result buffer
  per argument structure: valid in stream order until the next call with the same
  structure, which overwrites them in place (clone them to keep a value)."""
  ret, weight, adv, tar_padded = targets.ret, targets.weight, targets.adv, targets.tar_padded
  if rew.dim() != 2:
    raise ValueError(f'imag_metrics: rew must be (N, T), got {tuple(rew.shape)}')
  N, T = rew.shape
  if N == 0 or T < 2:
    raise ValueError(f'imag_metrics: (N, T) = ({N}, {T}), needs N >= 1 and T >= 2 (means of empty arrays otherwise)')
  ents = dict(ents or {})
  entlimits = dict(entlimits or {})
  if not set(entlimits) <= set(ents):
    raise ValueError(f'imag_metrics: entlimits for {sorted(set(entlimits) - set(ents))}, which `ents` does not have')
  wide, short = (rew, con, val_pred, slow_pred, weight, tar_padded, *ents.values()), (ret, adv)
  if any(tuple(x.shape) != (N, T) for x in wide) or any(tuple(x.shape) != (N, T - 1) for x in short):
    raise ValueError(f'imag_metrics: needs ({N}, {T}) arrays and ({N}, {T - 1}) returns and advantages')
  from . import ops
  arrays = wide + short
  float32 = all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in arrays)
  views = all(ops.stat_view(x) is not None for x in arrays)
  voffset, vscale = (0.0, 1.0) if vstats is None else vstats
  if not _imag_metrics_path(fused, float32, views, N * T):
    roffset, rscale = retnorm.latest()
    ret_normed = (ret - roffset) / rscale
    val, slowval = val_pred * vscale + voffset, slow_pred * vscale + voffset
    metrics = {
        'adv': adv.mean(), 'adv_std': adv.std(correction=0), 'adv_mag': adv.abs().mean(),
        'rew': rew.mean(), 'con': con.mean(), 'ret': ret_normed.mean(), 'val': val.mean(),
        'tar': tar_padded[:, :-1].mean(), 'weight': weight.mean(), 'slowval': slowval.mean(),
        'ret_min': ret_normed.min(), 'ret_max': ret_normed.max(),
        # (a count over n as a true division: torch's mean multiplies by a rounded 1 / n)
        'ret_rate': (ret_normed.abs() >= 1.0).sum().to(torch.float32) / _disc_tensor(float(ret.numel()), ret.device)}
    for k, ent in ents.items():
      metrics[f'ent/{k}'] = ent[:, :-1].mean()
      if k in entlimits:
        lo, hi = entlimits[k]
        metrics[f'rand/{k}'] = (metrics[f'ent/{k}'] - lo) / (hi - lo)
    return {k: v if v.dtype == torch.float32 else v.to(torch.float32) for k, v in metrics.items()}
  dev = rew.device
  if retnorm.impl == 'none':
    rpair = None
  else:
    retnorm.latest()                          # words 3-4 hold (offset, scale) of the present statistics
    rpair = retnorm._state(dev)[3:]
  vpair = _device_pair(voffset, vscale, dev)
  sub, mul = _lib.STAT_SUB_DIV, _lib.STAT_MUL_ADD
  items = [(adv, 0, None), (rew, 0, None), (con, 0, None), (ret, sub if rpair is not None else 0, rpair),
           (val_pred, mul if vpair is not None else 0, vpair), (slow_pred, mul if vpair is not None else 0, vpair),
           (tar_padded[:, :-1], 0, None), (weight, 0, None)]
  names = {'adv': (0, 0), 'adv_std': (0, 1), 'adv_mag': (0, 2), 'rew': (1, 0), 'con': (2, 0), 'ret': (3, 0),
           'val': (4, 0), 'tar': (6, 0), 'weight': (7, 0), 'slowval': (5, 0), 'ret_min': (3, 3), 'ret_max': (3, 4),
           'ret_rate': (3, 5)}
  for k, ent in ents.items():
    names[f'ent/{k}'] = (len(items), 0)
    items.append((ent[:, :-1], 0, None))
    if k in entlimits:
      lo, hi = (float(v) for v in entlimits[k])
      names[f'rand/{k}'] = (len(items), 0)
      items.append((ent[:, :-1], sub, _constant_pair(lo, hi - lo, dev)))
  key = (dev, tuple(names))
  plan = _IMAG_PLANS.get(key)
  if plan is None:
    if len(_IMAG_PLANS) > 64:
      _IMAG_PLANS.clear()
    out = torch.empty((len(items), _lib.STAT_VALUES), dtype=torch.float32, device=dev)
    plan = _IMAG_PLANS[key] = ((_lib.StatEntry * len(items))(), out, {k: out[e, c] for k, (e, c) in names.items()})
  table, out, results = plan
  for entry, (x, mode, pair) in zip(table, items):
    entry.rows, entry.cols, entry.stride = ops.stat_view(x)
    entry.x, entry.mode, entry.affine = x.data_ptr(), mode, None if pair is None else pair.data_ptr()
  fast.emb_stat_rows(table, len(items), out.data_ptr(), None, _stream(rew))
  return dict(results)


_MULTI = {}


def lambda_returns(problems, out=None):
  """Several `lambda_return` problems of one train step in ONE launch:
  `problems` = [(last, term, rew, val, boot, disc, lam), ...] (the arguments of
  `lambda_return`), result = [ret, ...].  DreamerV3 computes the replay returns
  (B, T) and the imagined returns (B*K, H+1) in the same train step
  (dreamerv3/agent.py:401-405, 464-466); at those sizes each scan is launch
  latency, so one launch costs half of two.  `out=[ret, ...]`: the caller's
  contiguous float32 (B, T-1) tensors."""
  import ctypes as C
  prepared, shapes = [], []
  for last, term, rew, val, boot, disc, lam in problems:
    dev = _device(rew, boot, last, term)
    rew, boot = _f32(rew, dev), _f32(boot, dev)
    last, term = _flag(last, dev), _flag(term, dev)
    B, T = rew.shape
    assert boot.shape == last.shape == term.shape == (B, T)
    assert val is None or tuple(val.shape) == (B, T)
    prepared.append((last, term, rew, boot, dev))
    shapes.append((B, T, _round32(disc), _round32(lam)))
  key = tuple(shapes)
  table = _MULTI.get(key)
  if table is None:
    if len(_MULTI) > 64:
      _MULTI.clear()
    table = _MULTI[key] = (_lib.LambdaProblem * len(shapes))()
    for entry, (B, T, disc, lam) in zip(table, shapes):
      entry.B, entry.T, entry.disc, entry.lam = B, T, disc, lam
  rets = []
  for i, ((last, term, rew, boot, dev), (B, T, _, _)) in enumerate(zip(prepared, shapes)):
    if out is not None:
      ret = out[i]
      if (ret.dtype != torch.float32 or tuple(ret.shape) != (B, T - 1) or ret.device != dev
          or not ret.is_contiguous()):
        raise ValueError(f'lambda_returns(out=): needs contiguous float32 {(B, T - 1)} tensors on {dev}')
    else:
      ret = _lib.empty((B, T - 1), torch.float32, dev)
    entry = table[i]
    entry.last, entry.term, entry.rew = last.data_ptr(), term.data_ptr(), rew.data_ptr()
    entry.boot, entry.ret = boot.data_ptr(), ret.data_ptr()
    rets.append(ret)
  if prepared:
    fast.emb_scan_lambda_multi(len(prepared), table, _stream(prepared[0][2]))
  return rets


def director_score(rew, cont, value, horizon=333, lam=0.95):
  """Time-major: rew (T-1,B), cont, value (T,B) -> ret (T-1,B)."""
  dev = _device(rew, cont, value)
  rew, cont, value = _f32(rew, dev), _f32(cont, dev), _f32(value, dev)
  T, B = value.shape
  assert cont.shape == (T, B) and rew.shape == (T - 1, B)
  ret = _lib.empty((T - 1, B), torch.float32, dev)
  if B == 0 or T < 2:
    return ret
  api.emb_scan_director(
      rew.data_ptr(), cont.data_ptr(), value.data_ptr(), T, B,
      _round32(1 - 1 / horizon), _round32(lam),
      ret.data_ptr(), _stream(rew))
  return ret


def split_traj(x, k, is_reward=False):
  """Director worker windows (director/hierarchy.py:224-238): time-major
  (T,B,...) -> (k, (T/k)*B, ...) views/reshapes; reward keys shift by one."""
  if is_reward:
    x = torch.cat([0 * x[:1], x], 0)
  x = x.reshape((x.shape[0] // k, k) + tuple(x.shape[1:]))
  x = x.transpose(0, 1)
  x = x.reshape((x.shape[0], -1) + tuple(x.shape[3:]))
  return x[1:] if is_reward else x


def abstract_traj(x, cont, k, kind='first'):
  """Director manager steps (director/hierarchy.py:240-256), time-major.
  kind 'reward': x (T-1,B) -> cumprod(cont)-weighted window means (T/k-1,B);
  'cont': x = cont (T,B) -> window products (T/k,B) — both one kernel
  (`emb_abstract_traj`); anything else: first step of every window (a view)."""
  if kind in ('reward', 'cont'):
    if not (torch.is_tensor(cont) and cont.is_cuda and cont.dim() == 2):
      raise RuntimeError(
          'abstract_traj reward/cont windows run as a HIP kernel: `cont` must be a (T, B) CUDA '
          'tensor (no CPU fallback)')
    dev = cont.device
    c = _f32(cont, dev)
    T, B = c.shape
    assert T % k == 0, (T, k)
    if kind == 'reward':
      r = _f32(x, dev)
      assert r.shape == (T - 1, B), (r.shape, c.shape)
      out = torch.empty((T // k - 1, B), dtype=torch.float32, device=dev)
      api.emb_abstract_traj(r.data_ptr(), c.data_ptr(), T, B, k, out.data_ptr(), None, _stream(c))
    else:
      out = torch.empty((T // k, B), dtype=torch.float32, device=dev)
      api.emb_abstract_traj(None, c.data_ptr(), T, B, k, None, out.data_ptr(), _stream(c))
    return out
  return x.reshape((x.shape[0] // k, k) + tuple(x.shape[1:]))[:, 0]   # first step of each window
