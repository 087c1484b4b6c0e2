"""`DeviceNormalize` from `GRID_MIN` values on: the chain of launches over many
workgroups (csrc/normalize_grid.hip) against numpy on the sorted input, bit for
bit where the kernel selects, and to one float32 rounding where it sums.  Sizes
are taken relative to `GRID_MIN` and to the tile.  Need a GPU."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from embodied_amd import DeviceNormalize
from embodied_amd import normalize as normlib

pytestmark = pytest.mark.gpu
GRID_MIN = getattr(normlib, 'GRID_MIN', 131072)      # (missing on the parent: test_the_path_is_taken says so)
# the threshold, one past it, a ragged last tile that is no multiple of 4, the capped grid
SIZES = [GRID_MIN, GRID_MIN + 1, GRID_MIN + 4099, 4096 * 256 + 3]
RAGGED = GRID_MIN + 4099


def _cuda(array, offset=0):
  """On the device, `offset` floats past a 16-byte boundary."""
  padded = torch.from_numpy(np.concatenate([np.zeros(offset, np.float32), array])).cuda()
  assert padded.data_ptr() % 16 == 0
  return padded[offset:]


def _boundary(low, high):
  """RAGGED values whose order statistics k and k + 1 of the 5th percentile are
  `low` and `high`: values below 1 before them, values above 3 behind."""
  gen = np.random.default_rng(5)
  k = int(0.05 * (RAGGED - 1))
  x = np.concatenate([gen.uniform(-10, 1, k), [low, high], gen.uniform(3, 10, RAGGED - k - 2)]).astype(np.float32)
  assert np.sort(x)[k] == np.float32(low) and np.sort(x)[k + 1] == np.float32(high)
  return gen.permutation(x)


def _bits(value):
  return np.uint32(value).view(np.float32)


INPUTS = {
    # 1.9999999 | 2.0: the keys differ in their top 11 bits
    'first digit': lambda: _boundary(np.nextafter(np.float32(2), np.float32(0)), 2.0),
    # the same top digit, bit 10 of the key differs
    'second digit': lambda: _boundary(_bits(0x40000000 + (1 << 10) - 1), _bits(0x40000000 + (1 << 10))),
    'all equal': lambda: np.full(RAGGED, -7.25, np.float32),
    'four values': lambda: np.random.default_rng(4).integers(-2, 2, RAGGED).astype(np.float32) * 0.5,
    'signed zeros': lambda: np.where(np.arange(RAGGED) % 3 == 0, -0.0, 0.0).astype(np.float32),
}
for n in SIZES:
  def _normal(n=n):
    gen = np.random.default_rng(n)
    x = (gen.standard_normal(n) * 30).astype(np.float32)
    x[::7] *= -1
    return gen.permutation(x)
  INPUTS[f'normal {n}'] = _normal


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('name', list(INPUTS))
def test_exact_selection(name, offset):
  """lo and hi after one update with rate 1 and no debiasing are the batch's
  percentiles: numpy's linear method restated in the kernel's float32 on the
  sorted input (position and weight from the float64 position, as norm_rank)."""
  x = INPUTS[name]()
  ordered, n = x[np.lexsort((~np.signbit(x), x))], len(x)       # np.sort with -0.0 below +0.0, the kernel's order
  device_x = _cuda(x, offset)
  for percs in ((5.0, 95.0), (0.0, 100.0), (37.3, 62.1)):
    norm = DeviceNormalize('perc', rate=1.0, debias=False, perclo=percs[0], perchi=percs[1])
    norm.update(device_x)
    state = norm.state_dict()
    for word, q in zip(('lo', 'hi'), percs):
      pos = q / 100 * (n - 1)
      k = int(np.floor(pos))
      a, b, frac = ordered[k], ordered[min(k + 1, n - 1)], np.float32(pos - k)
      want = a if frac == 0 or a.view(np.uint32) == b.view(np.uint32) else np.float32(a + np.float32(np.float32(b - a) * frac))
      want = np.float32(0) + want          # the EMA step from a zero state: 0 * 0 + 1 * value (-0.0 becomes +0.0)
      got = state[word].cpu().numpy()
      assert got.view(np.uint32) == want.view(np.uint32), (name, q, got, want)


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_mean_std(n, offset):
  """One float32 rounding of a float64 sum, and the same bits from run to run."""
  x = INPUTS[f'normal {n}']() + np.float32(3)
  device_x = _cuda(x, offset)
  runs = []
  for _ in range(2):
    norm = DeviceNormalize('meanstd', rate=1.0, debias=False)
    norm.update(device_x)
    runs.append(torch.stack([norm.state_dict()[k] for k in ('mean', 'sqrs')]).cpu().numpy())
  want = [np.mean(x, dtype=np.float64), np.mean(np.square(x), dtype=np.float64)]      # (squares in float32)
  print(f'n={n}: got {runs[0]} want {want}')
  np.testing.assert_allclose(runs[0], want, rtol=2.0 ** -23, atol=0)
  assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


@pytest.mark.parametrize('impl', ['meanstd', 'perc'])
@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_normalize_is_the_same_divide(n, offset, impl):
  x0 = INPUTS[f'normal {n}']()
  x, sub = _cuda(x0, offset), _cuda(x0 * np.float32(0.25) + np.float32(1), offset)
  norm = DeviceNormalize(impl)
  norm.update(x * 0.5)
  got = norm.normalize(x, sub=sub)
  offset_, scale = (v.clone() for v in norm.latest())
  torch.testing.assert_close(got, (x - sub) / scale, rtol=1e-6, atol=0)
  out = torch.empty_like(x)
  assert norm.normalize(x, out=out) is out
  offset_, scale = (v.clone() for v in norm.latest())
  torch.testing.assert_close(out, (x - offset_) / scale, rtol=1e-6, atol=0)
  # without an update the running statistics keep their bits ...
  before = {k: v.cpu().numpy().view(np.uint32) for k, v in norm.state_dict().items()}
  got = norm.normalize(x, update=False)
  torch.testing.assert_close(got, (x - offset_) / scale, rtol=1e-6, atol=0)
  after = {k: v.cpu().numpy().view(np.uint32) for k, v in norm.state_dict().items()}
  assert before == after
  # ... and in place, with an update
  want_stats = DeviceNormalize(impl)
  want_stats.load_state_dict(norm.state_dict())
  offset_, scale = (v.clone() for v in want_stats(x))
  want = (x - offset_) / scale
  assert norm.normalize(x, out=x) is x
  torch.testing.assert_close(x, want, rtol=1e-6, atol=0)


def test_the_path_is_taken():
  """From GRID_MIN values on a perc update is more than one launch, below it
  exactly one; torch dispatches no operator in either."""
  seen = []

  class Ops(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
      seen.append(str(func))
      return func(*args, **(kwargs or {}))

  assert normlib.GRID_MIN == GRID_MIN
  norm = DeviceNormalize('perc')
  for n, chain in ((GRID_MIN, True), (15360, False)):
    x = _cuda(INPUTS[f'normal {GRID_MIN}']()[:n])
    norm.update(x)
    before = normlib.launches()
    with Ops():
      norm.update(x)
    moved = normlib.launches() - before
    assert (1 < moved <= 4) if chain else moved == 1, (n, moved)
    assert seen == [], seen


def test_a_captured_chain_replays_to_the_eager_bits():
  """On a stream that already has its scratch block the chain itself is
  captured; every replay leaves the bits of the eager call on the same input."""
  x = _cuda(INPUTS[f'normal {RAGGED}']())
  stream = torch.cuda.Stream()
  norm = DeviceNormalize('perc', rate=1.0, debias=False)
  out = torch.empty_like(x)
  with torch.cuda.stream(stream):
    norm.normalize(x, out=out)
  stream.synchronize()
  graph, before = torch.cuda.CUDAGraph(), normlib.launches()
  with torch.cuda.graph(graph, stream=stream):
    norm.normalize(x, out=out)
  assert normlib.launches() - before == 6          # the clearing kernel in place of the memset
  for scale in (1.0, -2.0, 0.5):
    x.copy_(_cuda(INPUTS[f'normal {RAGGED}']() * np.float32(scale)))
    graph.replay()
    torch.cuda.synchronize()
    got = (norm.state_dict()['lo'].clone(), norm.state_dict()['hi'].clone(), out.clone())
    eager = DeviceNormalize('perc', rate=1.0, debias=False)
    want_out = eager.normalize(x)
    assert torch.equal(got[0], eager.state_dict()['lo']) and torch.equal(got[1], eager.state_dict()['hi'])
    assert torch.equal(got[2], want_out)
