"""The three newest users of `scan_piece4<W>` (csrc/scan_segment.h) at every
segment width: `scans.lambda_return_cont` (ContLambdaOp through launch_scan),
`scans.dreamer_targets` (dreamer_targets_kernel<W>) and `scans.ppo_targets`
(ppo_targets_kernel<W>), the fused launch and the composed path each, held to
the plain float64 statement of the operation in tests/target_reference.py at
the project's 1e-5 bar.

tests/target_sweep_cases.py derives the shapes from the kernels' constants:
every width at its first row length, with a last lane of 1, 2, 3 and 4 steps,
at n = 4 W (where the Dreamer kernel's weight phase has a second piece of one
column), with one row, three, and one more than a workgroup has segments (a
second sweep of the rows, all segments but one dead); for W = 64 both sides of
the piece boundaries.  tests/test_target_reference_host.py shows without a GPU
that float32 arithmetic alone stays inside the bar at every one of these shapes
(worst 0.12 of it), and that none of them divides rounding noise by a scale
near `limit`.  Need a GPU."""
import numpy as np
import pytest
import torch

from embodied_amd import DeviceNormalize
from embodied_amd.scans import dreamer_targets, lambda_return_cont, ppo_targets
from tests import target_reference as ref
from tests import target_sweep_cases as sweep

pytestmark = pytest.mark.gpu
# the project's stated float tolerance, as tests/test_gpu_dreamer_targets.py
RTOL = ATOL = 1e-5
DREAMER_FIELDS = ('ret', 'weight', 'adv', 'adv_normed', 'tar_padded')
PPO_FIELDS = ('adv', 'tar', 'tar_normed', 'adv_normed')


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _cuda(array, misalign=False):
  """`array` on the device; with `misalign` one element (one float, one byte)
  past a 16-byte boundary."""
  t = torch.from_numpy(np.ascontiguousarray(array)).cuda()
  if misalign:
    padded = torch.empty(t.numel() + 1, dtype=t.dtype, device='cuda')
    padded[1:].copy_(t.reshape(-1))
    t = padded[1:].view(array.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == t.element_size()
  return t


def _outs(shapes, misalign):
  if not misalign:
    return None
  outs = []
  for rows, cols in shapes:
    padded = torch.empty(rows * cols + 1, dtype=torch.float32, device='cuda')
    outs.append(padded[1:].view(rows, cols))
    assert outs[-1].data_ptr() % 16 == 4
  return tuple(outs)


def _norms(specs):
  return [DeviceNormalize(impl, **{**sweep.NORM, **fields}) for impl, fields in specs]


def _state(norm):
  """All five state words as host uint32 (bit patterns); 'none' has none."""
  if norm.impl == 'none':
    return np.zeros(5, np.uint32)
  return norm._state().cpu().numpy().view(np.uint32).copy()


def _pair(norm):
  return [0.0, 1.0] if norm.impl == 'none' else [float(v) for v in norm._stats]


def _bits(a):
  return np.ascontiguousarray(a).view(np.uint32)


def _hold(worst, where, key, got, want):
  """got against the float64 `want` at the bar; the worst ratio per key is kept."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (where, key, got.shape, want.shape)
  ratio = float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))) if want.size else 0.0
  worst[key] = max(worst.get(key, 0.0), ratio)
  assert ratio <= 1.0, (*where, key, f'|got - want| / (atol + rtol |want|) = {ratio:.4f}')


def _report(title, worst):
  print(f'{title}: worst |got - want| / (atol + rtol |want|) = ' + ', '.join(f'{k} {v:.4f}' for k, v in worst.items()))


def _paths(W, shape):
  """(name, fused, misalign): both paths, and the fused kernel once per width
  with every tensor one element past a 16-byte boundary."""
  paths = [('fused', True, False), ('composed', False, False)]
  if shape == sweep.off16_shape(W):
    paths.append(('fused off16', True, True))
  return paths


@pytest.mark.parametrize('W', sweep.WIDTHS)
def test_dreamer_targets_every_width(W):
  """Three calls with carried state (update, update, no update) per shape and
  path: the five outputs and the three normalisers' (offset, scale) against
  `dreamer_targets64`, the weight against `weight32` bit for bit, the padded
  column +0.0, the state words untouched by the call that does not update."""
  worst = {}
  for index, (N, T) in enumerate(sweep.shapes(W)):
    specs, contdisc = sweep.dreamer_settings(index)
    disc = sweep.dreamer_disc(contdisc)
    norms64 = [ref.Normalize64(impl, **{**sweep.NORM, **fields}) for impl, fields in specs]
    steps = []                               # the reference once, shared by the paths
    for step, update in enumerate(sweep.UPDATES):
      inp = sweep.dreamer_inputs(N, T, step)
      steps.append((inp, ref.dreamer_targets64(*inp, *norms64, disc, sweep.DREAMER['lam'], update),
                    ref.weight32(inp[1], disc)))
    shapes = ((N, T - 1), (N, T), (N, T - 1), (N, T - 1), (N, T))
    for path, fused, misalign in _paths(W, (N, T)):
      retnorm, valnorm, advnorm = norms = _norms(specs)
      for step, ((inp, want, weight), update) in enumerate(zip(steps, sweep.UPDATES)):
        where = (f'W={W}', (N, T), path, f'step {step}')
        before = None if update else [_state(norm) for norm in norms]
        got = dreamer_targets(*(_cuda(x, misalign) for x in inp), *norms, contdisc=contdisc, update=update,
                              out=_outs(shapes, misalign), fused=fused, **sweep.DREAMER)
        host = {k: getattr(got, k).cpu().numpy() for k in DREAMER_FIELDS}
        for key in DREAMER_FIELDS:
          _hold(worst, where, key, host[key], want[key])
        _hold(worst, where, 'stats', _pair(retnorm) + _pair(advnorm) + _pair(valnorm), want['stats'])
        differ = _bits(host['weight']) != _bits(weight)
        assert not differ.any(), (*where, 'weight', int(differ.sum()), np.argwhere(differ)[:4].tolist())
        assert not _bits(host['tar_padded'][:, -1]).any(), (*where, 'the padded column is not +0.0')
        if not update:
          for norm, b in zip(norms, before):
            assert np.array_equal(b, _state(norm)), (*where, norm.impl, b, _state(norm))
  _report(f'dreamer_targets W = {W}, {len(sweep.shapes(W))} shapes, fused and composed', worst)


@pytest.mark.parametrize('W', sweep.WIDTHS)
def test_ppo_targets_every_width(W):
  """The same for the PPO targets against `ppo_targets64`; at one shape per
  width `tarclip` = 2 bites, and the cells it clips are exactly +-2."""
  worst = {}
  for B, T in sweep.shapes(W):
    tarclip = 2.0 if (B, T) == sweep.clip_shape(W) else 10.0
    norms64 = [ref.Normalize64('meanstd', **sweep.NORM) for _ in range(2)]
    steps = []
    for step, update in enumerate(sweep.UPDATES):
      inp = sweep.ppo_inputs(B, T, step)
      steps.append((inp, ref.ppo_targets64(*inp, *norms64, sweep.PPO['hor'], sweep.PPO['lam'], tarclip, update)))
    shapes = ((B, T - 1), (B, T - 1), (B, T), (B, T - 1))
    for path, fused, misalign in _paths(W, (B, T)):
      valnorm, advnorm = norms = _norms(sweep.ALL3[1:])
      for step, ((inp, want), update) in enumerate(zip(steps, sweep.UPDATES)):
        where = (f'W={W}', (B, T), path, f'step {step}')
        before = None if update else [_state(norm) for norm in norms]
        got = ppo_targets(*(_cuda(x, misalign) for x in inp), valnorm, advnorm, tarclip=tarclip, update=update,
                          out=_outs(shapes, misalign), fused=fused, **sweep.PPO)
        host = {k: getattr(got, k).cpu().numpy() for k in PPO_FIELDS}
        for key in PPO_FIELDS:
          _hold(worst, where, key, host[key], want[key])
        _hold(worst, where, 'stats', _pair(valnorm) + _pair(advnorm), want['stats'])
        assert not _bits(host['tar_normed'][:, -1]).any(), (*where, 'the padded column is not +0.0')
        if tarclip == 2.0:
          # cells the definition clips by more than the bar: exactly +-2, nothing beyond
          beyond = np.abs(want['unclipped']) > 2.0 * (1 + RTOL) + ATOL
          assert beyond.mean() >= 0.01, (*where, 'the clip does not bite')
          assert np.array_equal(host['tar_normed'][beyond], np.sign(want['unclipped'][beyond]).astype(np.float32) * 2)
          assert np.abs(host['tar_normed']).max() == np.float32(2.0), where
        if not update:
          for norm, b in zip(norms, before):
            assert np.array_equal(b, _state(norm)), (*where, b, _state(norm))
  _report(f'ppo_targets W = {W}, {len(sweep.shapes(W))} shapes, fused and composed', worst)


@pytest.mark.parametrize('n_rows', [*sweep.CONT_ROWS, sweep.CONT_MANY_ROWS])
def test_lambda_return_cont_every_row_length(n_rows):
  """ContLambdaOp through every kernel of launch_scan: one step per lane
  (n <= 16), four steps per lane at every width (8193 rows: W = 4), the long-row
  kernel up to its third piece; both discounts; `out=` leaves the same bits."""
  worst = {}
  for N, T in sweep.cont_shapes(n_rows):
    arrays = sweep.dreamer_inputs(N, T, sweep.CONT_SEED)
    rew, con, pred = (_cuda(x) for x in arrays)
    for disc in sweep.CONT_DISCS:
      ret = lambda_return_cont(rew, con, pred, disc, sweep.CONT_LAM)
      assert ret.shape == (N, T - 1)
      want = ref.lambda_cont64(*arrays, disc, float(np.float32(sweep.CONT_LAM)))
      _hold(worst, ((N, T),), f'disc {disc:.4f}', ret.cpu().numpy(), want)
      out = torch.empty(N, T - 1, device='cuda')
      assert lambda_return_cont(rew, con, pred, disc, sweep.CONT_LAM, out=out) is out
      assert np.array_equal(_bits(out.cpu().numpy()), _bits(ret.cpu().numpy())), (N, T, disc)
  _report(f'lambda_return_cont, {n_rows} rows, {len(sweep.cont_shapes(n_rows))} lengths', worst)
