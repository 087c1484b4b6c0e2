"""Case tables and plain restatements for the device metrics: `emb_stat_rows`,
`scans.imag_metrics` (dreamerv3/agent.py:424-442) and `outs.total_loss`
(dreamerv3/agent.py:239-240).

Shared by `tools/gen_imag_metrics_golden.py` (which feeds the seeded inputs to
the reference's own `imag_loss`), by the host tests (which hold the float64
restatement against what the reference returned) and by the GPU tests and
tools.  numpy only: nothing here needs the library or a GPU.
"""
import numpy as np

from tests import dreamer_target_cases as dcases
from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)

f32, f64 = np.float32, np.float64

BAR = 1e-5                                   # the project's bar; what it multiplies is said per check
COLUMNS = ('mean', 'std', 'absmean', 'min', 'max', 'rate')
NONE, MUL_ADD, SUB_DIV = 0, 1, 2             # EMB_STAT_*

# ------------------------------------------------------------- restatements --


def affine32(x, mode=NONE, offset=0.0, scale=1.0):
  """x' of an entry: float32 operations, one rounding each, in the order written."""
  x = np.asarray(x, f32)
  offset, scale = f32(offset), f32(scale)
  if mode == MUL_ADD:
    return (x * scale).astype(f32) + offset
  if mode == SUB_DIV:
    with np.errstate(all='ignore'):
      return ((x - offset).astype(f32) / scale).astype(f32)
  return x


def exact32(xp):
  """(min, max, rate) of x' as float32: what the kernel returns bit for bit.  min
  and max return a NaN that is there; a NaN never counts toward the rate."""
  xp = np.asarray(xp, f32).reshape(-1)
  with np.errstate(invalid='ignore'):
    count = int((np.abs(xp) >= f32(1.0)).sum())
  return f32(np.min(xp)), f32(np.max(xp)), f32(count) / f32(xp.size)


def stats64(xp):
  """The six statistics of x' (float32 values) in float64: mean, population std
  (two passes, as numpy's), mean |x'|, then `exact32`."""
  flat = np.asarray(xp, f32).reshape(-1).astype(f64)
  with np.errstate(all='ignore'):
    mean, std, absmean = flat.mean(), flat.std(), np.abs(flat).mean()
  lo, hi, rate = exact32(xp)
  return np.array([mean, std, absmean, lo, hi, rate], f64)


def stats32(xp):
  """The float32 definition: numpy's float32 mean (pairwise sums) and std."""
  flat = np.asarray(xp, f32).reshape(-1)
  return np.array([flat.mean(dtype=f32), flat.std(dtype=f32), np.abs(flat).mean(dtype=f32), *exact32(xp)], f64)


def moment_bar(xp):
  """What mean, std and absmean of an entry are held to: BAR * mean |x'| in float64."""
  return BAR * float(np.abs(np.asarray(xp, f32).astype(f64)).mean())


def imag_metrics64(rew, con, val_pred, slow_pred, ret, adv, weight, tar_padded, rstats, vstats, ents, entlimits):
  """dreamerv3/agent.py:424-442 restated: every array is what the float32
  reference holds at that line, `rstats` = (roffset, rscale) as retnorm returned
  them, `vstats` = (voffset, vscale) from before the step (agent.py:397); the
  elementwise maps are float32 (`affine32`), the reductions float64.
  -> ({name: value}, {name: bar})."""
  ret_normed = affine32(ret, SUB_DIV, *rstats)
  val, slowval = affine32(val_pred, MUL_ADD, *vstats), affine32(slow_pred, MUL_ADD, *vstats)
  tar_normed = np.asarray(tar_padded, f32)[:, :-1]
  means = dict(adv=adv, rew=rew, con=con, ret=ret_normed, val=val, tar=tar_normed, weight=weight, slowval=slowval)
  got, bars = {}, {}
  for name, array in means.items():
    got[name], bars[name] = stats64(array)[0], moment_bar(array)
  got['adv_std'], got['adv_mag'] = stats64(adv)[1:3]
  bars['adv_std'] = bars['adv_mag'] = moment_bar(adv)
  got['ret_min'], got['ret_max'], got['ret_rate'] = exact32(ret_normed)
  bars['ret_min'] = bars['ret_max'] = bars['ret_rate'] = 0.0
  for k, ent in ents.items():
    kept = np.asarray(ent, f32)[:, :-1]
    got[f'ent/{k}'], bars[f'ent/{k}'] = stats64(kept)[0], moment_bar(kept)
    if k in entlimits:
      lo, hi = entlimits[k]
      got[f'rand/{k}'] = (got[f'ent/{k}'] - lo) / (hi - lo)
      # the fused path takes the mean of (ent - lo) / (hi - lo): the bar of that entry
      bars[f'rand/{k}'] = moment_bar(affine32(kept, SUB_DIV, lo, hi - lo))
  return got, bars


def total_loss64(losses, scales):
  """dreamerv3/agent.py:239-240 restated in float64 over the float32 losses and
  the float32 scales -> (total, {k: mean}, bar, {k: gradient value}): the bar is
  BAR * sum |scale_k| * mean |v_k|, the gradient of the total to every element of
  losses[k] is scale_k / n_k."""
  means = {k: np.asarray(v, f32).reshape(-1).astype(f64).mean() for k, v in losses.items()}
  total = sum(means[k] * f64(f32(scales[k])) for k in losses)
  bar = BAR * sum(abs(f64(f32(scales[k]))) * np.abs(np.asarray(v, f32).astype(f64)).mean() for k, v in losses.items())
  grads = {k: f64(f32(scales[k])) / np.asarray(v).size for k, v in losses.items()}
  return total, means, bar, grads


def total_loss32(losses, scales):
  """The float32 definition of the same lines: numpy's float32 means, the products
  added left to right from 0."""
  total = f32(0)
  for k, v in losses.items():
    total = f32(total + f32(np.asarray(v, f32).mean(dtype=f32) * f32(scales[k])))
  return total


# ------------------------------------------------------ emb_stat_rows cases --

THREADS, VECTOR = 1024, 4                    # kStatThreads, kStatVector: the GPU test reads them from stat_rows.h
MAX_ENTRIES = 48                             # kStatMaxEntries
# one element, both sides of a wave, of four waves, of the workgroup, and one
# element past a full pass of the workgroup's 16-byte loads
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, THREADS * VECTOR + 1)
# (rows, cols, buffer cols): a view that drops the last column, one row, and a
# view of more elements than the workgroup has threads
VIEWS = ((3, 5, 6), (1, 37, 37), (70, 15, 16))
OFFSETS = (1, 2, 3)                          # floats past a 16-byte boundary
OFFSET_COUNT = 259
LAUNCH_COUNTS = (1, 2, MAX_ENTRIES, MAX_ENTRIES + 1)
AFFINE = {NONE: (0.0, 1.0), MUL_ADD: (0.375, 1.75), SUB_DIV: (-0.125, 0.75)}


def stat_data(tag, n, seed=0):
  """n float32 values ~ 2 N(0, 1) + 0.25: mean |x| about 1.6, a std far above 0.1
  of the mean (the condition under which a std is held to a bar that is relative
  to mean |x'|; the host test checks it for every entry)."""
  rng = np.random.default_rng([seed, n, *(ord(c) for c in tag)])
  return (2 * rng.standard_normal(n) + 0.25).astype(f32)


def edge_data(n, mode, seed=0):
  """`stat_data` with elements whose x' is exactly +-1.0 and others whose |x'| is
  the float32 just below 1.0, for the entry's affine map: -> (x, exactly one,
  just below).  The preimages are searched among the neighbours of the real
  preimage, so x' is what `affine32` gives, not what algebra promises.  Arrays
  of fewer than 64 elements stay as they are (eight planted values would be the
  array)."""
  x = stat_data('edge', n, seed)
  offset, scale = AFFINE[mode]
  one, below = f32(1.0), np.nextafter(f32(1.0), f32(0.0))

  def preimage(target):
    guess = f32(target)
    if mode == MUL_ADD:
      guess = f32((f64(target) - offset) / scale)
    elif mode == SUB_DIV:
      guess = f32(f64(target) * scale + offset)
    cand = guess
    for _ in range(8):
      cand = np.nextafter(cand, f32(-np.inf))
    for _ in range(17):
      if affine32(np.array([cand], f32), mode, offset, scale)[0] == f32(target):
        return cand
      cand = np.nextafter(cand, f32(np.inf))
    return None

  hits = {name: [v for v in (preimage(s * t) for s in (1, -1)) if v is not None]
          for name, t in (('one', one), ('below', below))}
  slots = np.random.default_rng([seed, n, 99]).permutation(n)
  placed = {'one': 0, 'below': 0}
  cursor = 0
  for name in ('one', 'below'):
    for value in hits[name]:
      for _ in range(2):                       # each value twice, in arrays of a wave and more
        if n >= 64:
          x[slots[cursor]] = value
          cursor += 1
          placed[name] += 1
  return x, placed['one'], placed['below']


# ---------------------------------------------------------- imag_loss cases --

STEPS = dcases.STEPS
PARAMS, NORM = dcases.PARAMS, dcases.NORM
KEYS = ('move', 'arm')                       # a discrete and a continuous action key
ENTLIMITS = {'move': (0.0, 1.6094379124341003), 'arm': (-3.5, 4.25)}          # (minent, maxent)
# (source, Case): rows of tests/dreamer_target_cases.py by index -- the shipped
# normalisers on a small batch, all three normalisers, a tiny odd shape, T = 2,
# many rows with disc = 1 - 1 / horizon -- and the workload's (1024, 16), which
# that table does not have (source None: seeded here, the same distributions).
IMAG_CASES = tuple((i, dcases.CASES[i]) for i in (0, 1, 2, 3, 5)) + (
    (None, dcases.Case((1024, 16), ('perc', {}), ('none', {}), ('none', {}), True, True, False)),)
METRICS = ('adv', 'adv_std', 'adv_mag', 'rew', 'con', 'ret', 'val', 'tar', 'weight', 'slowval',
           'ret_min', 'ret_max', 'ret_rate', 'ent/move', 'rand/move', 'ent/arm', 'rand/arm')


def imag_tag(case):
  source, c = IMAG_CASES[case]
  return f'i{case}_{c.shape[0]}x{c.shape[1]}_{c.retnorm[0]}_{c.valnorm[0]}_{c.advnorm[0]}'


def imag_inputs(case, step):
  """rew, con, pred, slow as tests/dreamer_target_cases.py makes them, and the
  entropies of the two action keys: `move` ~ U[0.2, 1.5) and `arm` ~ 1.5 N(0, 1) +
  0.5 (a continuous head's entropy may be negative), float32."""
  source, c = IMAG_CASES[case]
  if source is not None:
    inp = dict(dcases.inputs(source, step))
  else:
    rng = np.random.default_rng([1000 + case, step, *c.shape])
    rew, pred, slow = (rng.standard_normal(c.shape).astype(f32) for _ in range(3))
    con = np.minimum((0.9 + 0.1 * rng.random(c.shape)).astype(f32), np.nextafter(f32(1), f32(0)))
    pick = rng.random(c.shape)
    con[pick < 0.03] = 0.0
    con[pick > 0.97] = 1.0
    inp = dict(rew=rew, con=con, pred=pred, slow=slow)
  rng = np.random.default_rng([7, case, step, *c.shape])
  inp['ent_move'] = (0.2 + 1.3 * rng.random(c.shape)).astype(f32)
  inp['ent_arm'] = (1.5 * rng.standard_normal(c.shape) + 0.5).astype(f32)
  return inp


def target_pred(case, inp):
  """The prediction that serves as the target value (dreamerv3/agent.py:400)."""
  return inp['slow'] if IMAG_CASES[case][1].slowtar else inp['pred']


# --------------------------------------------------------- total_loss cases --

LOSS_SHAPES = ((16, 64), (1,), (3, 5, 7))
LOSS_COUNTS = (1, 3, 10)


def loss_inputs(count, seed=0):
  """`count` float32 losses of the shapes above in turn, named as Agent.loss's, with
  scales of both signs and sizes -> (losses, scales), dicts in the same order."""
  names = ('dyn', 'rep', 'image', 'rew', 'con', 'policy', 'value', 'repval', 'extra', 'aux')
  rng = np.random.default_rng([seed, count])
  losses, scales = {}, {}
  for index in range(count):
    shape = LOSS_SHAPES[index % len(LOSS_SHAPES)]
    losses[names[index]] = (rng.standard_normal(shape) * (1 + index) + 0.5).astype(f32)
    scales[names[index]] = (1.0, 0.1, 0.3, -0.5, 1.0, 1.0, 1.0, 0.3, 2.5, 1e-3)[index]
  return losses, scales
