"""`emb_stat_rows` / `ops.stat_rows`, `scans.imag_metrics` and `outs.total_loss` on
the GPU (csrc/stat_rows.hip), against the restatements of
tests/stat_metric_cases.py: mean, std and mean |x'| at the project's 1e-5 bar
times mean |x'|; min, max and rate bit for bit against the float32 restatement.
tests/test_stat_metrics_host.py shows without a GPU that float32 sums alone stay
far inside those bars at every shape used here.  Need a GPU."""
import pathlib
import re

import numpy as np
import pytest
import torch

from embodied_amd import DeviceNormalize, _lib, ops, outs, scans
from tests import stat_metric_cases as cases

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
MODES = {cases.NONE: None, cases.MUL_ADD: 'mul_add', cases.SUB_DIV: 'sub_div'}
GRAD_RTOL = 4 * 2.0 ** -24       # against float64: (g * scale) / n is two float32 roundings, g * scale * (1 / n) three
PAIR_RTOL = 8 * 2.0 ** -24       # fused against composed: the roundings of both


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _bits(a):
  return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _cuda(array, offset=0):
  """`array` on the device, its first element `offset` floats past a 16-byte boundary."""
  array = np.ascontiguousarray(array, np.float32)
  buffer = torch.zeros(array.size + offset + 4, dtype=torch.float32, device='cuda')
  view = buffer[offset:offset + array.size]
  view.copy_(torch.from_numpy(array.reshape(-1)))
  assert view.data_ptr() % 16 == 4 * offset
  return view.view(array.shape)


def _entry(x, mode, pairs):
  return x if mode == cases.NONE else (x, MODES[mode], pairs[mode])


def _pairs():
  return {mode: torch.tensor(pair, dtype=torch.float32, device='cuda') for mode, pair in cases.AFFINE.items()}


def _hold(where, row, xp):
  """One row of `stat_rows` against the restatements of x' (a host array)."""
  row = np.asarray(row, np.float32)
  want, bar = cases.stats64(xp), cases.moment_bar(xp)
  for index, column in enumerate(cases.COLUMNS[:3]):
    if xp.size == 1 and column == 'std':
      assert row[index] == 0.0, (where, 'the std of one element', row[index])
      continue
    share = abs(float(row[index]) - want[index]) / bar
    print(f'{where} {column}: got {row[index]!r}, float64 {want[index]!r}, share of the bar {share:.4f}')
    assert share <= 1.0, (where, column, float(row[index]), want[index], share)
  exact = np.array(cases.exact32(xp), np.float32)
  assert np.array_equal(_bits(row[3:]), _bits(exact)), (where, 'min, max, rate', row[3:], exact)


def test_constants_come_from_the_header():
  text = (ROOT / 'embodied_amd' / 'csrc' / 'stat_rows.h').read_text()
  constant = lambda name: int(re.search(r'constexpr\s+\w+\s+%s\s*=\s*(\d+)' % name, text).group(1))
  assert cases.COUNTS[-1] == constant('kStatThreads') * constant('kStatVector') + 1
  assert cases.MAX_ENTRIES == _lib.STAT_MAX_ENTRIES and 'kStatMaxEntries = EMB_STAT_MAX_ENTRIES' in text


@pytest.mark.parametrize('mode', sorted(cases.AFFINE))
def test_every_element_count(mode):
  """One launch over every count, aligned: elements at exactly |x'| = 1.0 count,
  the float32 just below does not."""
  pairs, offset_scale = _pairs(), cases.AFFINE[mode]
  host = [cases.edge_data(n, mode) for n in cases.COUNTS]
  before = ops.stat_rows_launches()
  out = ops.stat_rows([_entry(_cuda(x), mode, pairs) for x, _, _ in host])
  assert ops.stat_rows_launches() == before + 1
  got = out.cpu().numpy()
  assert got.shape == (len(cases.COUNTS), 6) and got.dtype == np.float32
  for row, (x, ones, below), n in zip(got, host, cases.COUNTS):
    xp = cases.affine32(x, mode, *offset_scale)
    _hold(f'mode {mode} n {n}', row, xp)
    count = int((np.abs(xp) >= 1).sum())
    assert round(float(row[5]) * n) == count and abs(float(row[5]) * n - count) < 1e-3, (n, row[5], count)   # the count is exact
    if n >= 64:
      assert ones >= 2 and below >= 2 and (np.abs(xp) == 1.0).sum() >= ones


def test_matrix_views_and_odd_offsets():
  pairs = _pairs()
  entries, host = [], []
  for index, (rows, cols, width) in enumerate(cases.VIEWS):
    full = cases.stat_data('view', rows * width).reshape(rows, width)
    mode = sorted(cases.AFFINE)[index % 3]
    entries.append(_entry(_cuda(full)[:, :cols], mode, pairs))
    host.append((f'view {rows}x{cols} of {width}', cases.affine32(full[:, :cols], mode, *cases.AFFINE[mode])))
  for offset in cases.OFFSETS:
    x = cases.stat_data('offset', cases.OFFSET_COUNT + offset)[offset:]
    mode = sorted(cases.AFFINE)[offset % 3]
    entries.append(_entry(_cuda(x, offset), mode, pairs))
    host.append((f'offset {offset}', cases.affine32(x, mode, *cases.AFFINE[mode])))
  # a view whose rows start off 16 bytes, and one row of a wider buffer
  full = cases.stat_data('view', 70 * 16 + 1)
  entries.append(_cuda(full, 1)[1:].view(70, 16)[:, :15])
  host.append(('view 70x15 of 16, off 8 bytes', full[1:].reshape(70, 16)[:, :15]))
  before = ops.stat_rows_launches()
  got = ops.stat_rows(entries).cpu().numpy()
  assert ops.stat_rows_launches() == before + 1
  for row, (where, xp) in zip(got, host):
    _hold(where, row, xp)


@pytest.mark.parametrize('count', cases.LAUNCH_COUNTS)
def test_launch_counts(count):
  host = [cases.stat_data('launch', 33 + index, seed=count) for index in range(count)]
  before = ops.stat_rows_launches()
  got = ops.stat_rows([_cuda(x) for x in host]).cpu().numpy()
  assert ops.stat_rows_launches() - before == -(-count // _lib.STAT_MAX_ENTRIES)
  assert got.shape == (count, 6)
  for index, (row, x) in enumerate(zip(got, host)):
    _hold(f'{count} entries, entry {index}', row, x)


@pytest.mark.parametrize('special', [np.nan, np.inf, -np.inf])
def test_nan_and_infinity_stay_in_their_row(special):
  pairs = _pairs()
  modes = (cases.NONE, cases.SUB_DIV, cases.MUL_ADD, cases.NONE, cases.NONE)
  offsets = (0, 0, 0, 1, 0)
  host = [cases.stat_data('special', 300 + index) for index in range(5)]

  def run(arrays):
    entries = [_entry(_cuda(x, o), m, pairs) for x, m, o in zip(arrays, modes, offsets)]
    return ops.stat_rows(entries).cpu().numpy()

  clean = run(host)
  for target, position in ((1, 130), (3, 299)):          # a 16-byte load's lane, and a 4-byte load's last element
    dirty = [x.copy() for x in host]
    dirty[target][position] = special
    got = run(dirty)
    xp = cases.affine32(dirty[target], modes[target], *cases.AFFINE[modes[target]])
    want = cases.stats64(xp).astype(np.float32)
    assert np.array_equal(got[target], want, equal_nan=True), (special, target, got[target], want)
    assert np.isnan(want[1]) and (np.isnan(special) or abs(want[0]) == np.inf)
    others = [k for k in range(5) if k != target]
    assert np.array_equal(_bits(got[others]), _bits(clean[others])), (special, target)
    assert not np.array_equal(_bits(got[target]), _bits(clean[target]))


def test_same_bits_run_to_run_and_nothing_written_beside_out():
  pairs = _pairs()
  entries = [_entry(_cuda(cases.stat_data('again', 500 + 37 * index), index % 4), sorted(cases.AFFINE)[index % 3], pairs)
             for index in range(7)]
  spare = 16
  buffer = torch.full((spare + 7 * 6 + spare,), 7.0, dtype=torch.float32, device='cuda')
  out = buffer[spare:spare + 42].view(7, 6)
  assert ops.stat_rows(entries, out=out) is out
  first = buffer.cpu().numpy().copy()
  buffer[spare:spare + 42].fill_(7.0)
  ops.stat_rows(entries, out=out)
  second = buffer.cpu().numpy()
  assert np.array_equal(_bits(first), _bits(second))
  assert (first[:spare] == 7.0).all() and (first[-spare:] == 7.0).all()
  assert not (first[spare:-spare] == 7.0).all()
  fresh = ops.stat_rows(entries).cpu().numpy()
  assert np.array_equal(_bits(fresh), _bits(first[spare:-spare].reshape(7, 6)))


# ------------------------------------------------------------ imag_metrics --

@pytest.fixture(scope='module')
def golden():
  with np.load(ROOT / 'tests' / 'golden' / 'imag_metrics.npz') as f:
    return {key: f[key] for key in f.files}


@pytest.mark.parametrize('case', range(len(cases.IMAG_CASES)))
def test_imag_metrics_over_the_fixture(case, golden):
  """Fused and composed over STEPS train steps with carried normaliser state.
  Against the float64 restatement over the arrays `dreamer_targets` left on the
  device: moments at the bar, min / max / rate bit for bit (fused; the composed
  path divides as torch does, the same bits here).  Against what the reference's
  own imag_loss returned: the reference's arrays differ from the device's by what
  tests/test_gpu_dreamer_targets.py allows, 1e-5 (1 + |x|) per element, and so do
  roffset and rscale: three such terms on top of the bar."""
  source, c = cases.IMAG_CASES[case]
  name = cases.imag_tag(case)
  for path, fused in (('fused', True), ('composed', False)):
    retnorm, valnorm, advnorm = (DeviceNormalize(impl, **{**cases.NORM, **fields})
                                 for impl, fields in (c.retnorm, c.valnorm, c.advnorm))
    for step in range(cases.STEPS):
      inp = cases.imag_inputs(case, step)
      dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
      vstats = None if valnorm.impl == 'none' else tuple(v.clone() for v in valnorm.latest())    # BEFORE the step
      targets = scans.dreamer_targets(dev['rew'], dev['con'], torch.from_numpy(cases.target_pred(case, inp)).cuda(),
                                      retnorm, valnorm, advnorm, contdisc=c.contdisc, update=True, **cases.PARAMS)
      ents = {k: dev[f'ent_{k}'] for k in cases.KEYS}
      before = ops.stat_rows_launches()
      got = scans.imag_metrics(targets, dev['rew'], dev['con'], dev['pred'], dev['slow'], retnorm, vstats, ents,
                               cases.ENTLIMITS, fused=fused)
      assert ops.stat_rows_launches() - before == (1 if fused else 0), path
      assert list(got) == list(cases.METRICS)
      assert all(v.dtype == torch.float32 and v.dim() == 0 for v in got.values())
      got = {k: v.cpu().numpy() for k, v in got.items()}
      rstats = [float(v) for v in retnorm._stats]
      vhost = (0.0, 1.0) if vstats is None else [float(v) for v in vstats]
      ret = targets.ret.cpu().numpy()
      want, bars = cases.imag_metrics64(
          inp['rew'], inp['con'], inp['pred'], inp['slow'], ret, targets.adv.cpu().numpy(),
          targets.weight.cpu().numpy(), targets.tar_padded.cpu().numpy(), rstats, vhost,
          {k: inp[f'ent_{k}'] for k in cases.KEYS}, cases.ENTLIMITS)
      theirs = dict(zip(cases.METRICS, golden[f'metrics_{name}'][step]))
      ret_normed = cases.affine32(ret, cases.SUB_DIV, *rstats)
      for metric in cases.METRICS:
        where = (name, path, f'step {step}', metric)
        if bars[metric] == 0.0:
          assert np.array_equal(_bits(got[metric]), _bits(want[metric])), (*where, got[metric], want[metric])
        else:
          share = abs(float(got[metric]) - want[metric]) / bars[metric]
          print(*where, f'got {got[metric]!r}, float64 {want[metric]!r}, share of the bar {share:.4f}')
          assert share <= 1.0, (*where, float(got[metric]), want[metric], share)
        # the reference's own value
        if metric == 'ret_rate':
          near = int((np.abs(np.abs(ret_normed.astype(np.float64)) - 1.0) <= 3e-5 * 2).sum())
          assert abs(float(got[metric]) - float(theirs[metric])) * ret.size <= near + 1e-3, (*where, theirs[metric], near)
        elif metric in ('ret_min', 'ret_max'):
          assert abs(float(got[metric]) - float(theirs[metric])) <= 3e-5 * (1 + abs(float(theirs[metric]))), where
        else:
          scale = bars[metric] / cases.BAR                       # mean |x'|
          assert abs(float(got[metric]) - float(theirs[metric])) <= bars[metric] + 3e-5 * (1 + scale), (
              *where, float(got[metric]), float(theirs[metric]))


def test_imag_metrics_takes_views_and_constants():
  """`fused=None` on float32 inputs takes the kernel; a strided input stays one
  launch; float vstats go in as a constant pair; the results are views of one
  buffer that the next call overwrites."""
  inp = cases.imag_inputs(0, 0)
  dev = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
  norms = [DeviceNormalize(impl, **cases.NORM) for impl in ('perc', 'none', 'none')]
  targets = scans.dreamer_targets(dev['rew'], dev['con'], dev['slow'], *norms)
  wide = torch.from_numpy(np.concatenate([inp['rew'], inp['rew']], 1)).cuda()[:, :inp['rew'].shape[1]]
  assert not wide.is_contiguous()
  before = ops.stat_rows_launches()
  got = scans.imag_metrics(targets, wide, dev['con'], dev['pred'], dev['slow'], norms[0], vstats=(0.25, 1.5))
  assert ops.stat_rows_launches() == before + (1 if scans._imag_metrics_path(None, True, True, wide.numel()) else 0)
  same = scans.imag_metrics(targets, wide, dev['con'], dev['pred'], dev['slow'], norms[0], vstats=(0.25, 1.5), fused=True)
  other = scans.imag_metrics(targets, wide, dev['con'], dev['pred'], dev['slow'], norms[0], vstats=(0.25, 1.5), fused=False)
  assert same['val'].data_ptr() == scans.imag_metrics(
      targets, wide, dev['con'], dev['pred'], dev['slow'], norms[0], vstats=(0.25, 1.5), fused=True)['val'].data_ptr()
  val = cases.affine32(inp['pred'], cases.MUL_ADD, 0.25, 1.5)
  for result in (got, same, other):
    assert abs(float(result['val']) - cases.stats64(val)[0]) <= cases.moment_bar(val)
    assert abs(float(result['rew']) - cases.stats64(inp['rew'])[0]) <= cases.moment_bar(inp['rew'])
  with pytest.raises(ValueError, match=r'fused=True\): the kernel reads float32'):
    scans.imag_metrics(targets, wide.double(), dev['con'], dev['pred'], dev['slow'], norms[0], fused=True)


# -------------------------------------------------------------- total_loss --

def _total(losses, scales, fused, gradient=None):
  tensors = {k: torch.from_numpy(v).cuda().requires_grad_() for k, v in losses.items()}
  before = outs.stat_rows_launches()
  loss, metrics = outs.total_loss(tensors, scales, fused=fused)
  forward = outs.stat_rows_launches() - before
  loss.backward(gradient=None if gradient is None else torch.tensor(gradient, device='cuda'))
  backward = outs.stat_rows_launches() - before - forward
  return (loss.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in metrics.items()},
          {k: v.grad.cpu().numpy() for k, v in tensors.items()}, (forward, backward))


@pytest.mark.parametrize('count', cases.LOSS_COUNTS)
def test_total_loss_forward_and_gradients(count):
  losses, scales = cases.loss_inputs(count)
  total, means, bar, grads = cases.total_loss64(losses, scales)
  for gradient in (None, 0.37):
    fused = _total(losses, scales, True, gradient)
    composed = _total(losses, scales, False, gradient)
    assert fused[3] == (1, 1) and composed[3] == (0, 0)
    for path, (loss, metrics, got, _) in (('fused', fused), ('composed', composed)):
      share = abs(float(loss) - total) / bar
      print(f'total_loss K = {count} {path}: got {loss!r}, float64 {total!r}, share of the bar {share:.4f}')
      assert loss.dtype == np.float32 and loss.shape == () and share <= 1.0, (path, float(loss), total, share)
      assert list(metrics) == [f'loss/{k}' for k in losses]
      for k, v in losses.items():
        assert abs(float(metrics[f'loss/{k}']) - means[k]) <= cases.moment_bar(v), (path, k)
        g = np.float32(1.0 if gradient is None else gradient)
        np.testing.assert_allclose(got[k], np.full(v.shape, float(g) * grads[k]), rtol=GRAD_RTOL, atol=0, err_msg=f'{path} {k}')
        assert got[k].shape == v.shape and len(np.unique(got[k])) == 1
    for k in losses:                                            # torch autograd of the composed path
      np.testing.assert_allclose(fused[2][k], composed[2][k], rtol=PAIR_RTOL, atol=0, err_msg=k)
  again = _total(losses, scales, True)
  assert np.array_equal(_bits(again[0]), _bits(_total(losses, scales, True)[0]))
  default = _total(losses, scales, None)
  assert default[3] == ((1, 1) if outs._total_loss_path(None, True, True, count, 1, 1024) else (0, 0))


@pytest.mark.parametrize('count', [3, 10])
def test_total_loss_nan_stays_in_its_key(count):
  losses, scales = cases.loss_inputs(count)
  clean = _total(losses, scales, True)
  dirty = {k: v.copy() for k, v in losses.items()}
  bad = list(losses)[1]
  dirty[bad].reshape(-1)[0] = np.nan
  loss, metrics, grads, _ = _total(dirty, scales, True)
  assert np.isnan(loss) and np.isnan(metrics[f'loss/{bad}'])
  for k in losses:
    if k != bad:
      assert np.array_equal(_bits(metrics[f'loss/{k}']), _bits(clean[1][f'loss/{k}'])), k
      assert np.array_equal(_bits(grads[k]), _bits(clean[2][k])), k
  assert np.isfinite(grads[bad]).all()                         # d total / d v is scale / n whatever v holds


def test_total_loss_leaves_what_the_kernels_do_not_take_to_torch():
  losses, scales = cases.loss_inputs(3)
  tensors = {k: torch.from_numpy(v).cuda() for k, v in losses.items()}
  first = list(tensors)[0]
  tensors[first] = torch.from_numpy(np.concatenate([losses[first]] * 2, 1)).cuda()[:, ::2]
  before = outs.stat_rows_launches()
  loss, _ = outs.total_loss(tensors, scales)
  assert outs.stat_rows_launches() == before and loss.dim() == 0
  with pytest.raises(ValueError, match=r'fused=True\): the kernels read and write contiguous'):
    outs.total_loss(tensors, scales, fused=True)
  only = {first: torch.from_numpy(losses[first]).cuda().requires_grad_(False)}
  loss, metrics = outs.total_loss(only, {first: scales[first]}, fused=True)       # nothing asks for a gradient
  assert not loss.requires_grad and abs(float(loss) - float(metrics[f'loss/{first}']) * scales[first]) < 1e-6
