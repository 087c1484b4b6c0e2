"""`DeviceNormalize`: the return normaliser (embodied/jax/utils.py:16-91) as one
HIP launch per call (emb_normalize, csrc/normalize.hip).  Against the fixture
made by executing the reference's class (tests/golden/normalize.npz), against
numpy's percentiles and means on edge inputs, and against
`distributed.Normalize` across a checkpoint.  Need a GPU."""
import pathlib

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from embodied_amd import DeviceNormalize          # every test here fails without the feature
from embodied_amd import normalize as normlib
from oracle import gen_normalize_golden as gen    # CASES, STEPS, inputs: no reference tree needed

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'normalize.npz'
# the project's stated float tolerance, as tests/test_normalize_golden.py
RTOL = ATOL = 1e-5


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _cuda(array):
  return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def _pair(stats):
  return np.array([float(v) for v in stats], np.float64)


def _words(norm):
  """The running statistics as host float32 (state_dict order)."""
  return {k: v.cpu().numpy() for k, v in norm.state_dict().items()}


def _bits(norm):
  return {k: v.view(np.uint32) for k, v in _words(norm).items()}


@pytest.mark.parametrize('case', range(len(gen.CASES)))
def test_golden_parity(case):
  impl, fields = gen.CASES[case]
  with np.load(GOLDEN) as f:
    want = f[f'case{case}']
  norm = DeviceNormalize(impl, **fields)
  rows = [_pair(norm.stats())]
  for step in range(gen.STEPS):
    rows.append(_pair(norm(_cuda(gen.inputs(case, step)), update=True)))
  got = np.stack(rows)
  print(f'case {case}: worst |got - want| / (atol + rtol |want|) = '
        f'{np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want))):.4f}')
  np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def _selected(x, perclo, perchi):
  """(lo, hi) that one update with rate 1 and no debiasing leaves in the state:
  exactly the batch's two percentiles."""
  norm = DeviceNormalize('perc', rate=1.0, debias=False, perclo=perclo, perchi=perchi)
  norm.update(x if torch.is_tensor(x) else _cuda(x))
  words = _words(norm)
  return words['lo'], words['hi']


@pytest.mark.parametrize('n, perclo, perchi', [
    (101, 5.0, 95.0), (101, 0.0, 100.0), (16384, 0.0, 100.0), (16384, 100.0, 0.0), (11, 50.0, 20.0),
    (20001, 5.0, 95.0), (20001, 0.0, 100.0)])
def test_exact_selection(n, perclo, perchi):
  """Where q/100 * (n-1) is an integer the percentile is an element of the
  input: bit-equal to the sorted array's."""
  gen_ = np.random.default_rng([n, int(perclo)])
  x = (gen_.standard_normal(n) * 30).astype(np.float32)
  x[::7] *= -1
  gen_.shuffle(x)
  ordered = np.sort(x)
  for q in (perclo, perchi):
    assert q / 100 * (n - 1) == int(q / 100 * (n - 1))
  lo, hi = _selected(x, perclo, perchi)
  assert lo.view(np.uint32) == ordered[int(perclo / 100 * (n - 1))].view(np.uint32)
  assert hi.view(np.uint32) == ordered[int(perchi / 100 * (n - 1))].view(np.uint32)


def _edge_inputs():
  gen_ = np.random.default_rng(7)
  zeros = np.zeros(4099, np.float32)
  zeros[::2] = -0.0
  zeros[::5] = gen_.standard_normal(len(zeros[::5])).astype(np.float32) * 1e-3
  return {
      'ties': gen_.integers(0, 4, 5000).astype(np.float32) - 1,
      'few distinct, large': gen_.integers(-2, 3, 70001).astype(np.float32) * 0.5,
      'negative zero': zeros,
      'all equal': np.full(3000, 2.5, np.float32),
      'all equal, large': np.full(40000, -7.25, np.float32),
      'n = 1': np.array([-3.75], np.float32),
      'n = 2': np.array([4.0, -1.0], np.float32),
      'n = 16384': gen_.standard_normal(16384).astype(np.float32),
      'n = 16385': gen_.standard_normal(16385).astype(np.float32) * 3 + 1,
      'n = 1M + 3': gen_.standard_normal((1 << 20) + 3).astype(np.float32) * 100 - 20,
  }


@pytest.mark.parametrize('name', list(_edge_inputs()))
@pytest.mark.parametrize('offset', [0, 1])
def test_ties_and_edge_values(name, offset):
  """Both paths (keys in LDS up to 16384 values, re-read from global memory
  beyond), 16-byte aligned input and input that starts one float later."""
  x = _edge_inputs()[name]
  padded = _cuda(np.concatenate([np.zeros(offset, np.float32), x]))
  device_x = padded[offset:]
  assert device_x.is_contiguous() and device_x.data_ptr() % 16 == 4 * offset
  for perclo, perchi in ((5.0, 95.0), (37.3, 62.1), (0.0, 100.0)):
    lo, hi = _selected(device_x, perclo, perchi)
    want = np.percentile(x.astype(np.float32), [perclo, perchi])
    print(f'{name} q=({perclo}, {perchi}): got ({lo}, {hi}) want {want}')
    np.testing.assert_allclose([lo, hi], want, rtol=RTOL, atol=ATOL)
  norm = DeviceNormalize('meanstd', rate=1.0, debias=False)
  norm.update(device_x)
  words = _words(norm)
  want = [np.mean(x, dtype=np.float64), np.mean(np.square(x), dtype=np.float64)]
  print(f'{name} means: got ({words["mean"]}, {words["sqrs"]}) want {want}')
  np.testing.assert_allclose([words['mean'], words['sqrs']], want, rtol=RTOL, atol=ATOL)


def test_percentiles_of_values_twenty_decades_apart():
  """Neighbouring order statistics may differ by many times their own size
  here, so the weight matters to its last bits.  numpy places the percentile of
  float32 data with float32 arithmetic (q / 100 * (n - 1) rounded to float32: a
  weight off by up to 4e-6 at n = 97); the kernel's position is computed in
  double, so the yardstick is numpy's percentile of the same values as float64.
  Its distance: float32 rounding of the weight, the product and the sum, 3 * 2^-24
  of the larger neighbour -- inside 1e-5 of the result unless the result is a
  near-cancellation, hence atol on the scale of the neighbours."""
  gen_ = np.random.default_rng(11)
  for n in (97, 3000, 20000):
    x = (gen_.standard_normal(n) * 10.0 ** gen_.integers(-10, 10, n)).astype(np.float32)
    ordered = np.sort(x)
    for perclo, perchi in ((5.0, 95.0), (37.3, 62.1)):
      lo, hi = _selected(x, perclo, perchi)
      for got, q in ((lo, perclo), (hi, perchi)):
        k = int(q / 100 * (n - 1))
        want = np.percentile(x.astype(np.float64), q)
        atol = ATOL * max(abs(float(ordered[k])), abs(float(ordered[min(k + 1, n - 1)])))
        print(f'n={n} q={q}: got {got} want {want}')
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=atol)


@pytest.mark.parametrize('impl', ['meanstd', 'perc'])
def test_update_false_leaves_the_state_alone(impl):
  norm = DeviceNormalize(impl)
  gen_ = np.random.default_rng(3)
  for _ in range(3):
    norm.update(_cuda(gen_.standard_normal((16, 64)).astype(np.float32)))
  before, stats = _bits(norm), _pair(norm.stats())
  other = _cuda(gen_.standard_normal((1024, 15)).astype(np.float32) * 50 + 9)
  assert np.array_equal(_pair(norm(other, update=False)), stats)
  norm.normalize(other, update=False)
  norm.normalize(other, sub=other * 0.5, update=False)
  assert np.array_equal(_pair(norm.stats()), stats)
  after = _bits(norm)
  assert before.keys() == after.keys() and all(before[k] == after[k] for k in before), (before, after)


@pytest.mark.parametrize('impl', ['meanstd', 'perc'])
@pytest.mark.parametrize('shape', [(16, 64), (1024, 15), (16, 64, 16), (70001,), (7,)])
def test_normalize_is_the_same_divide(impl, shape):
  """One float32 subtract and divide against torch's, from the returned stats."""
  gen_ = np.random.default_rng(len(shape))
  norm = DeviceNormalize(impl)
  x = _cuda(gen_.standard_normal(shape).astype(np.float32) * 20 + 3)
  sub = _cuda(gen_.standard_normal(shape).astype(np.float32))
  norm.update(x * 0.5)
  # against the stats of the same launch (update=True) ...
  got = norm.normalize(x, sub=sub)
  offset, scale = (v.clone() for v in norm.stats())
  torch.testing.assert_close(got, (x - sub) / scale, rtol=1e-6, atol=0)
  got = norm.normalize(x)
  offset, scale = (v.clone() for v in norm.stats())
  torch.testing.assert_close(got, (x - offset) / scale, rtol=1e-6, atol=0)
  # ... into the caller's tensor, without an update, and in place
  out = torch.empty_like(x)
  assert norm.normalize(x, out=out, update=False) is out
  torch.testing.assert_close(out, (x - offset) / scale, rtol=1e-6, atol=0)
  want = (x - sub) / scale
  assert norm.normalize(x, sub=sub, out=x, update=False) is x
  torch.testing.assert_close(x, want, rtol=1e-6, atol=0)
  # other dtypes / strides are converted first
  turned = norm.normalize(want.to(torch.float64).transpose(0, -1), update=False)
  torch.testing.assert_close(turned, (want.transpose(0, -1) - offset) / scale, rtol=1e-6, atol=0)


@pytest.mark.parametrize('impl, fields', [('meanstd', {}), ('perc', {}), ('meanstd', {'debias': False, 'rate': 0.1})])
def test_checkpoint_interop(impl, fields):
  from embodied_amd import distributed as D
  case = 1
  device = DeviceNormalize(impl, **fields)
  for step in range(10):
    device.update(_cuda(gen.inputs(case, step)))
  torch_norm = D.Normalize(impl, **fields)
  torch_norm.state = dict(device.state_dict())               # DeviceNormalize -> distributed.Normalize
  for step in range(10, 15):
    x = _cuda(gen.inputs(case, step))
    np.testing.assert_allclose(_pair(device(x)), _pair(torch_norm(x)), rtol=RTOL, atol=ATOL)
  back = DeviceNormalize(impl, **fields)
  back.load_state_dict(torch_norm.state)                     # ... and back
  np.testing.assert_allclose(_pair(back.stats()), _pair(torch_norm.stats()), rtol=RTOL, atol=ATOL)
  for step in range(15, 20):
    x = _cuda(gen.inputs(case, step))
    np.testing.assert_allclose(_pair(back(x)), _pair(torch_norm(x)), rtol=RTOL, atol=ATOL)
  # host numbers (a checkpoint read from disk), loaded before the first call
  cold = DeviceNormalize(impl, **fields)
  cold.load_state_dict({k: float(v) for k, v in torch_norm.state.items()})
  x = _cuda(gen.inputs(case, 20))
  np.testing.assert_allclose(_pair(cold(x)), _pair(torch_norm(x)), rtol=RTOL, atol=ATOL)


class _Ops(TorchDispatchMode):
  """Every operator torch dispatches while the mode is on."""

  def __init__(self):
    super().__init__()
    self.seen = []

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    self.seen.append(str(func))
    return func(*args, **(kwargs or {}))


@pytest.mark.parametrize('impl', ['meanstd', 'perc'])
def test_one_launch_and_no_allocation_per_call(impl):
  """A steady-state call is one kernel launch: the library's launch counter
  moves by one and torch dispatches no operator at all (so it launches and
  allocates nothing).  Allocated memory does not grow over 100 calls."""
  norm = DeviceNormalize(impl)
  x = _cuda(np.random.default_rng(0).standard_normal((1024, 15)).astype(np.float32))
  sub, out = x * 0.25, torch.empty_like(x)
  norm(x)
  torch.cuda.synchronize()
  for call in (lambda: norm(x), lambda: norm(x, update=False), lambda: norm.update(x), norm.stats,
               lambda: norm.normalize(x, sub=sub, out=out)):
    before = normlib.launches()
    with _Ops() as ops:
      call()
    assert normlib.launches() - before == 1
    assert ops.seen == [], ops.seen
  allocated = torch.cuda.memory_allocated()
  for _ in range(100):
    offset, scale = norm(x)
    norm.normalize(x, sub=sub, out=out)
  torch.cuda.synchronize()
  assert torch.cuda.memory_allocated() == allocated
  assert offset.shape == () and offset.dtype == torch.float32 and offset.is_cuda


@pytest.mark.parametrize('impl', ['meanstd', 'perc'])
def test_profiler_counts_one_kernel_per_call(impl):
  """The same count from outside the library: the device-side events of a
  torch.profiler window over 10 calls are 10 kernels, all of them this one."""
  from torch.profiler import ProfilerActivity, profile
  norm = DeviceNormalize(impl)
  x = _cuda(np.random.default_rng(1).standard_normal((1024, 15)).astype(np.float32))
  sub, out = x * 0.25, torch.empty_like(x)
  norm(x)
  with profile(activities=[ProfilerActivity.CUDA]):      # the tracer's own first-use work stays out of the count
    norm(x)
    torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CUDA]) as prof:
    for _ in range(5):
      norm(x)
      norm.normalize(x, sub=sub, out=out)
    torch.cuda.synchronize()
  names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
  print(names)
  assert len(names) == 10 and all('normalize_kernel' in name for name in names), names
