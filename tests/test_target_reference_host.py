"""tests/target_reference.py, the float64 statement the target sweeps hold the
kernels to (tests/test_gpu_target_sweeps.py), checked without a GPU:

  * against the fixtures made by executing the reference's own `imag_loss`,
    `ppo_loss`, `lambda_return` and `Normalize` (tests/golden/dreamer_targets.npz,
    ppo_targets.npz): every case, step, field and carried statistic.  This ties
    the float64 definitions to the real ones;
  * against a float32 composition in the reference's operation order
    (oracle/np_oracle.py's `Normalize`, `lambda_return` and `gae`) at every shape
    and step of the sweep, with the sweep's own inputs.  This is the condition
    under which the sweep's 1e-5 bar is fair: float32 arithmetic alone stays
    inside it, and no swept shape divides rounding noise by a scale near `limit`;
  * the sweep's lists against the kernels' constants they are derived from.

CPU only."""
import pathlib

import numpy as np
import pytest

from oracle import np_oracle
from tests import dreamer_target_cases as dreamer_cases
from tests import ppo_target_cases as ppo_cases
from tests import target_reference as ref
from tests import target_sweep_cases as sweep

GOLDEN = pathlib.Path(__file__).parent / 'golden'
# the project's stated float tolerance, as tests/test_gpu_dreamer_targets.py
RTOL = ATOL = 1e-5
f32 = np.float32


def _worst(got, want):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))) if want.size else 0.0


def _note(worst, key, got, want):
  worst[key] = max(worst.get(key, 0.0), _worst(got, want))


def _report(title, worst):
  print(f'{title}: worst |got - want| / (atol + rtol |want|) = ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))
  assert max(worst.values()) <= 1.0, (title, worst)


# ---------------------------------------------------------------- fixtures --

def test_float64_definitions_against_the_dreamer_fixture():
  keys = dict(ret='ret', weight='weight', adv='adv', adv_normed='advnormed', tar_padded='tarpadded', stats='stats')
  with np.load(GOLDEN / 'dreamer_targets.npz') as f:
    for case, c in enumerate(dreamer_cases.CASES):
      name = dreamer_cases.tag(case)
      norms = [ref.Normalize64(impl, **{**dreamer_cases.NORM, **fields}) for impl, fields in
               (c.retnorm, c.valnorm, c.advnorm)]
      disc = 1 if c.contdisc else 1 - 1 / dreamer_cases.PARAMS['horizon']
      worst = {}
      for step in range(dreamer_cases.STEPS):
        inp = dreamer_cases.inputs(case, step)
        assert np.array_equal(dreamer_cases.digest(inp), f[f'in_{name}'][step])
        got = ref.dreamer_targets64(inp['rew'], inp['con'], dreamer_cases.target_pred(case, inp), *norms, disc,
                                    dreamer_cases.PARAMS['lam'], True)
        for key, stored in keys.items():
          _note(worst, key, got[key], f[f'{stored}_{name}'][step])
        assert np.array_equal(ref.weight32(inp['con'], disc).view(np.uint32),
                              f[f'weight_{name}'][step].view(np.uint32)), (name, step)
        assert not got['tar_padded'][:, -1].any()
      _report(name, worst)


def test_float64_definitions_against_the_ppo_fixture():
  keys = dict(adv='adv', tar='tar', tar_normed='tarnormed', adv_normed='advnormed', stats='stats')
  with np.load(GOLDEN / 'ppo_targets.npz') as f:
    for case, ((B, T), tarclip) in enumerate(ppo_cases.CASES):
      name = ppo_cases.tag(case)
      valnorm, advnorm = (ref.Normalize64('meanstd', **ppo_cases.NORM) for _ in range(2))
      worst = {}
      for step in range(ppo_cases.STEPS):
        inp = ppo_cases.inputs(case, step)
        assert np.array_equal(ppo_cases.digest(inp), f[f'in_{name}'][step])
        got = ref.ppo_targets64(inp['rew'], inp['pred'], inp['last'], inp['term'], valnorm, advnorm,
                                ppo_cases.PARAMS['hor'], ppo_cases.PARAMS['lam'], tarclip, True)
        for key, stored in keys.items():
          _note(worst, key, got[key], f[f'{stored}_{name}'][step])
        assert not got['tar_normed'][:, -1].any()
      _report(name, worst)


def test_lambda_cont64_is_the_fixture_s_lambda_return():
  """The cases that run without a valnorm: boot is the prediction itself."""
  with np.load(GOLDEN / 'dreamer_targets.npz') as f:
    worst = {}
    for case in dreamer_cases.NONE_VALNORM_CASES:
      c = dreamer_cases.CASES[case]
      disc = float(f32(1 if c.contdisc else 1 - 1 / dreamer_cases.PARAMS['horizon']))
      for step in range(dreamer_cases.STEPS):
        inp = dreamer_cases.inputs(case, step)
        got = ref.lambda_cont64(inp['rew'], inp['con'], dreamer_cases.target_pred(case, inp), disc,
                                float(f32(dreamer_cases.PARAMS['lam'])))
        _note(worst, dreamer_cases.tag(case), got, f[f'ret_{dreamer_cases.tag(case)}'][step])
    _report('lambda_cont64', worst)


# ------------------------------------------------------ the sweep's lists --

def test_sweep_lists_follow_the_kernels_constants():
  root = pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc'
  ladder = 'n <= 16 ? 4 : n <= 32 ? 8 : n <= 64 ? 16 : n <= 128 ? 32 : 64'
  for source in ('scans.hip', 'ppo_targets.hip', 'dreamer_targets.hip'):
    assert ladder in (root / source).read_text(), source
  header = (root / 'normalize.h').read_text()
  assert f'kNormLdsMax = {sweep.LDS_MAX}' in header and f'kNormThreads = {sweep.THREADS}' in header
  assert sorted(sweep.LENGTHS) == list(sweep.WIDTHS)
  for W in sweep.WIDTHS:
    lengths = sweep.LENGTHS[W]
    assert all(sweep.width(n) == W for n in lengths), W
    assert any(n % 4 == 2 for n in lengths), W                   # a last lane with two steps
    assert sweep.off16_shape(W) in sweep.shapes(W) and sweep.clip_shape(W) in sweep.shapes(W)
    assert max(sweep.rows(W)) == sweep.THREADS // W + 1           # a second sweep of the rows
    assert all(N * (T - 1) <= sweep.LDS_MAX for N, T in sweep.shapes(W))
    if W == 4:
      continue
    first = 2 * W + 1                                             # the ladder's first n of this width
    assert {first, first + 1, first + 2, 4 * W - 1, 4 * W} <= set(lengths), W
    assert {n % 4 for n in lengths} == {0, 1, 2, 3}, W
    assert sweep.width(first - 1) == W // 2
    assert sweep.rows(W)[:2] == (1, 3)
  assert max(sweep.LENGTHS[32]) == 128 and sweep.width(129) == 64
  assert {255, 256, 257, 258, 511, 512, 513} <= set(sweep.LENGTHS[64])   # both sides of the pieces' ends
  assert max(N * (T - 1) for N, T in sweep.shapes(64)) == 17 * 513
  # lambda_return_cont: every T of test_scans_at_every_row_length, the long-row kernel's 2nd and 3rd piece
  assert set(range(2, 71)) | {126, 127, 128, 129, 130, 131, 254, 255, 256, 257, 258, 259, 300} <= set(sweep.CONT_LENGTHS)
  assert {1025, 1026, 2049, 2050} <= set(sweep.CONT_LENGTHS)
  assert sweep.CONT_MANY_ROWS == 8192 + 1 and {15, 16, 17} <= set(sweep.CONT_MANY_LENGTHS)
  assert 'n <= 16 && B <= 8192' in (root / 'scans.hip').read_text()


# -------------------------------- float32 arithmetic alone, at every shape --

def _oracle_norms(specs):
  return [np_oracle.Normalize(impl, **{**sweep.NORM, **fields}) for impl, fields in specs]


def _norms64(specs):
  return [ref.Normalize64(impl, **{**sweep.NORM, **fields}) for impl, fields in specs]


def _dreamer32(rew, con, pred, retnorm, valnorm, advnorm, disc, lam, update):
  """dreamerv3/agent.py:397-419 in float32, one operation after the other."""
  voffset, vscale = valnorm.stats()
  tarval = pred * vscale + voffset
  ret = np_oracle.lambda_return(np.zeros_like(con), f32(1) - con, rew, tarval, disc, lam)
  if update:
    retnorm.update([ret])
  roffset, rscale = retnorm.stats()
  adv = (ret - tarval[:, :-1]) / rscale
  if update:
    advnorm.update([adv])
  aoffset, ascale = advnorm.stats()
  adv_normed = (adv - aoffset) / ascale
  if update:
    valnorm.update([ret])
  voffset, vscale = valnorm.stats()
  tar_normed = (ret - voffset) / vscale
  out = dict(ret=ret, adv=adv, adv_normed=adv_normed,
             tar_padded=np.concatenate([tar_normed, 0 * tar_normed[:, -1:]], 1),
             stats=np.array([roffset, rscale, aoffset, ascale, voffset, vscale], np.float64))
  assert all(v.dtype == f32 for k, v in out.items() if k != 'stats')
  return out


def _ppo32(rew, pred, last, term, valnorm, advnorm, hor, lam, tarclip, update):
  """ppo/agent.py:188-210 in float32, one operation after the other."""
  voffset, vscale = valnorm.stats()
  val = pred * vscale + voffset
  adv, tar = np_oracle.gae(rew, val, last, term, hor, lam)
  if update:
    valnorm.update([tar])
  voffset, vscale = valnorm.stats()
  tar_normed = (tar - voffset) / vscale
  if tarclip:
    tar_normed = np.clip(tar_normed, -f32(tarclip), f32(tarclip))
  if update:
    advnorm.update([adv])
  aoffset, ascale = advnorm.stats()
  out = dict(adv=adv, tar=tar, tar_normed=np.concatenate([tar_normed, 0 * tar_normed[:, :1]], 1),
             adv_normed=(adv - aoffset) / ascale, stats=np.array([voffset, vscale, aoffset, ascale], np.float64))
  assert all(v.dtype == f32 for k, v in out.items() if k != 'stats')
  return out


@pytest.mark.parametrize('W', sweep.WIDTHS)
def test_float32_stays_inside_the_bar_at_every_dreamer_shape(W):
  worst, least = {}, {}
  for index, (N, T) in enumerate(sweep.shapes(W)):
    specs, contdisc = sweep.dreamer_settings(index)
    disc = sweep.dreamer_disc(contdisc)
    norms32, norms64 = _oracle_norms(specs), _norms64(specs)
    for step, update in enumerate(sweep.UPDATES):
      rew, con, pred = sweep.dreamer_inputs(N, T, step)
      got = _dreamer32(rew, con, pred, *norms32, disc, sweep.DREAMER['lam'], update)
      want = ref.dreamer_targets64(rew, con, pred, *norms64, disc, sweep.DREAMER['lam'], update)
      for key, values in got.items():
        _note(worst, key, values, want[key])
      # no swept case is rounding noise divided by `limit` (the (1, 2) caveat of the older tests)
      for name, scale in zip(('rscale', 'ascale', 'vscale'), want['stats'][1::2]):
        least[name] = min(least.get(name, np.inf), scale)
        assert scale > 1e-3, (N, T, step, name, scale)
  print(f'W = {W}: least ' + ', '.join(f'{k} {v:.4f}' for k, v in least.items()))
  _report(f'dreamer W = {W}, float32 against float64', worst)


@pytest.mark.parametrize('W', sweep.WIDTHS)
def test_float32_stays_inside_the_bar_at_every_ppo_shape(W):
  worst, least = {}, {}
  for B, T in sweep.shapes(W):
    tarclip = 2.0 if (B, T) == sweep.clip_shape(W) else 10.0
    norms32, norms64 = _oracle_norms(sweep.ALL3[1:]), _norms64(sweep.ALL3[1:])
    for step, update in enumerate(sweep.UPDATES):
      inp = sweep.ppo_inputs(B, T, step)
      got = _ppo32(*inp, *norms32, sweep.PPO['hor'], sweep.PPO['lam'], tarclip, update)
      want = ref.ppo_targets64(*inp, *norms64, sweep.PPO['hor'], sweep.PPO['lam'], tarclip, update)
      for key, values in got.items():
        _note(worst, key, values, want[key])
      for name, scale in zip(('vscale', 'ascale'), want['stats'][1::2]):
        least[name] = min(least.get(name, np.inf), scale)
        assert scale > 1e-3, (B, T, step, name, scale)
      if tarclip == 2.0:                                  # the clip bites
        assert (np.abs(want['unclipped'][:, :-1]) > 2.0).mean() >= 0.01, (B, T, step)
  print(f'W = {W}: least ' + ', '.join(f'{k} {v:.4f}' for k, v in least.items()))
  _report(f'ppo W = {W}, float32 against float64', worst)


@pytest.mark.parametrize('n_rows', [*sweep.CONT_ROWS, sweep.CONT_MANY_ROWS])
def test_float32_stays_inside_the_bar_at_every_cont_shape(n_rows):
  worst = {}
  for N, T in sweep.cont_shapes(n_rows):
    rew, con, pred = sweep.dreamer_inputs(N, T, sweep.CONT_SEED)
    for disc in sweep.CONT_DISCS:
      got = np_oracle.lambda_return(np.zeros_like(con), f32(1) - con, rew, pred, disc, sweep.CONT_LAM)
      _note(worst, f'disc {disc:.4f}', got, ref.lambda_cont64(rew, con, pred, disc, float(f32(sweep.CONT_LAM))))
  _report(f'lambda_return_cont, {n_rows} rows, float32 against float64', worst)
