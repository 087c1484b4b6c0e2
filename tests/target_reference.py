"""Plain float64 statements of what the target kernels compute: the running
return normaliser (embodied/jax/utils.py:44-91), the top of imag_loss
(dreamerv3/agent.py:397-419) with its lambda-return (:482-490) and the top of
ppo_loss (ppo/agent.py:188-210).  numpy only: no torch, no GPU.

The hyper-parameters are rounded to float32 first (rate, limit, disc, lam,
1 - 1 / hor, tarclip), because that is what the kernels receive; everything
after that is float64.  tests/test_target_reference_host.py ties these
definitions to the fixtures made by executing the reference's own functions.
The recurrences are vectorised over rows and loop over t only.
"""
import numpy as np

f32, f64 = np.float32, np.float64


def _r32(x):
  return f64(f32(x))


class Normalize64:
  """embodied/jax/utils.py:16-91: 'none' / 'meanstd' / 'perc', the debias
  correction and the limit.  Only `rate` and `limit` are rounded to float32."""

  def __init__(self, impl, rate=0.01, limit=1e-8, perclo=5.0, perchi=95.0, debias=True):
    assert impl in ('none', 'meanstd', 'perc'), impl
    self.impl, self.rate, self.limit = impl, _r32(rate), _r32(limit)
    self.perclo, self.perchi, self.debias = perclo, perchi, debias
    self.var = {k: f64(0) for k in ('corr', 'mean', 'sqrs', 'lo', 'hi')}

  def _update(self, name, x):                       # utils.py:90-91
    self.var[name] = (1 - self.rate) * self.var[name] + self.rate * f64(x)

  def update(self, x):                              # utils.py:44-57
    x = np.asarray(x, f64)
    if self.impl == 'meanstd':
      self._update('mean', x.mean())
      self._update('sqrs', np.square(x).mean())
    elif self.impl == 'perc':
      self._update('lo', np.percentile(x, self.perclo))     # linear interpolation
      self._update('hi', np.percentile(x, self.perchi))
    if self.debias and self.impl != 'none':
      self._update('corr', 1.0)

  def stats(self):                                  # utils.py:59-74
    if self.impl == 'none':
      return f64(0), f64(1)
    corr = f64(1)
    if self.debias:
      corr = corr / np.maximum(self.rate, self.var['corr'])
    if self.impl == 'meanstd':
      mean = self.var['mean'] * corr
      std = np.sqrt(np.maximum(0.0, self.var['sqrs'] * corr - mean ** 2))
      return mean, np.maximum(self.limit, std)
    lo, hi = self.var['lo'] * corr, self.var['hi'] * corr
    return lo, np.maximum(self.limit, hi - lo)

  def __call__(self, x, update):                    # utils.py:39-42
    if update:
      self.update(x)
    return self.stats()

  def words(self):
    """The three running statistics in the order of the device state's words."""
    first, second = ('lo', 'hi') if self.impl == 'perc' else ('mean', 'sqrs')
    return np.array([self.var[first], self.var[second], self.var['corr']], f64)


def lambda_cont64(rew, con, boot, disc, lam):
  """dreamerv3/agent.py:401-405,482-490 in float64: last = 0, term = 1 - con."""
  rew, con, boot = (np.asarray(x, np.float64) for x in (rew, con, boot))
  live = (1 - (1 - con))[:, 1:] * disc
  interm = rew[:, 1:] + (1 - lam) * live * boot[:, 1:]
  rets = [boot[:, -1]]
  for t in reversed(range(live.shape[1])):
    rets.append(interm[:, t] + live[:, t] * lam * rets[-1])
  return np.stack(list(reversed(rets))[:-1], 1)


def weight32(con, disc):
  """agent.py:402 as numpy computes it from float32 inputs: float32 products
  taken left to right, one rounding each.  The kernel promises this order, so
  the weight is held bit for bit."""
  return np.cumprod(f32(disc) * np.asarray(con, f32), 1, dtype=f32) / f32(disc)


def dreamer_targets64(rew, con, pred, retnorm, valnorm, advnorm, disc, lam, update):
  """dreamerv3/agent.py:397-419 with `pred` the prediction that serves as the
  target value.  The three `Normalize64` take their step (with `update`).
  -> dict(ret, weight, adv, adv_normed, tar_padded, stats) with stats =
  (roffset, rscale, aoffset, ascale, voffset, vscale) as the calls returned them."""
  rew, con, pred = (np.asarray(x, f64) for x in (rew, con, pred))
  disc, lam = _r32(disc), _r32(lam)
  voffset, vscale = valnorm.stats()                 # BEFORE the step
  tarval = pred * vscale + voffset
  weight = np.cumprod(disc * con, 1) / disc
  ret = lambda_cont64(rew, con, tarval, disc, lam)
  roffset, rscale = retnorm(ret, update)            # AFTER the step
  adv = (ret - tarval[:, :-1]) / rscale
  aoffset, ascale = advnorm(adv, update)
  adv_normed = (adv - aoffset) / ascale
  voffset, vscale = valnorm(ret, update)
  tar_normed = (ret - voffset) / vscale
  tar_padded = np.concatenate([tar_normed, np.zeros_like(tar_normed[:, -1:])], 1)
  stats = np.array([roffset, rscale, aoffset, ascale, voffset, vscale], f64)
  return dict(ret=ret, weight=weight, adv=adv, adv_normed=adv_normed, tar_padded=tar_padded, stats=stats)


def ppo_targets64(rew, pred, last, term, valnorm, advnorm, hor, lam, tarclip, update):
  """ppo/agent.py:188-210.  -> dict(adv, tar, tar_normed, adv_normed, unclipped,
  stats): tar_normed clipped to +-tarclip (None / 0: no clip) and padded with a
  zero column, `unclipped` the same before the clip, stats = (voffset, vscale,
  aoffset, ascale) as the calls returned them."""
  rew, pred = np.asarray(rew, f64), np.asarray(pred, f64)
  last, term = np.asarray(last) != 0, np.asarray(term) != 0
  lam = _r32(lam)
  voffset, vscale = valnorm.stats()                 # BEFORE the step
  val = pred * vscale + voffset
  live = (~term).astype(f64)[:, 1:] * _r32(1 - 1 / hor)
  cont = (~last & ~term).astype(f64)[:, 1:] * lam
  delta = rew[:, 1:] + live * val[:, 1:] - val[:, :-1]
  advs = [np.zeros(len(rew), f64)]
  for t in reversed(range(delta.shape[1])):
    advs.append(delta[:, t] + live[:, t] * cont[:, t] * advs[-1])
  adv = np.stack(list(reversed(advs))[:-1], 1)
  tar = adv + val[:, :-1]
  voffset, vscale = valnorm(tar, update)
  unclipped = (tar - voffset) / vscale
  tar_normed = np.clip(unclipped, -_r32(tarclip), _r32(tarclip)) if tarclip else unclipped
  pad = np.zeros_like(tar_normed[:, :1])
  aoffset, ascale = advnorm(adv, update)
  adv_normed = (adv - aoffset) / ascale
  stats = np.array([voffset, vscale, aoffset, ascale], f64)
  return dict(adv=adv, tar=tar, tar_normed=np.concatenate([tar_normed, pad], 1), adv_normed=adv_normed,
              unclipped=np.concatenate([unclipped, pad], 1), stats=stats)
