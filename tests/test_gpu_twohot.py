"""`embodied_amd.outs.TwoHot`: the symexp_twohot head (embodied/jax/outs.py:273-330)
on the kernels of csrc/twohot.hip and as composed torch ops, against the float64
run of the reference's own class (tests/golden/twohot.npz) and, for the shapes
the fixture does not hold, against `tests.twohot_cases.reference64` (which the
host test holds against that fixture).  Need a GPU.

Bars: loss within the project's RTOL = ATOL = 1e-5 of float64; pred within
1e-5 * (1 + sum |p_i b_i|), the same tolerance on the sum's condition scale (the
bins reach +-4.85e8 and cancel).  The reference's own float32 run stays inside
both (worst 0.03 and 0.04 of the bars, tests/test_twohot_host.py), so they leave
room for another reduction order and nothing more.  Measured worst ratios of
the kernels: profiles/twohot_accuracy.txt."""
import pathlib

import numpy as np
import pytest
import torch

from embodied_amd.outs import TwoHot, symexp_twohot_bins, twohot_launches   # every test here fails without the feature
from tests import twohot_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'twohot.npz'
RTOL = ATOL = 1e-5
EPS32 = float(np.finfo(np.float32).eps)
PATHS = pytest.mark.parametrize('fused', [True, False], ids=['fused', 'composed'])


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def _cuda(array):
  return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def _loss_ratio(got, want):
  """Worst |got - want| / (ATOL + RTOL |want|); NaN where and only where `want` is."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert np.array_equal(np.isnan(got), np.isnan(want)), (np.isnan(got).sum(), np.isnan(want).sum())
  ok = ~np.isnan(want)
  return float(np.max(np.abs(got - want)[ok] / (ATOL + RTOL * np.abs(want[ok])), initial=0.0))


def _pred_ratio(got, ref):
  return float(np.max(np.abs(np.asarray(got, np.float64) - ref['pred']) / (1e-5 * (1 + ref['scale'])), initial=0.0))


_SHAPED = {}


def _shaped(n, rows, lead=None):
  """Seeded inputs of another shape and their float64 values, computed once."""
  key = (n, rows, lead)
  if key not in _SHAPED:
    rng = np.random.default_rng([n, rows])
    bins = symexp_twohot_bins(n)
    logits = np.concatenate([cases.logits_of(kind, -(-rows // 4), n, rng) for kind in cases.KINDS])[:rows]
    logits = logits[rng.permutation(rows)]
    targets = [cases.targets_of(rows, bins, rng, special=False) for _ in range(2)]
    gout = rng.standard_normal(rows).astype(np.float32)
    ref = cases.reference64(logits, bins, targets)
    for a in (logits, gout, *targets):
      a.setflags(write=False)
    _SHAPED[key] = dict(bins=bins, logits=logits, targets=targets, gout=gout, ref=ref)
  return _SHAPED[key]


@PATHS
@pytest.mark.parametrize('case', range(len(cases.CASES)), ids=cases.tag)
def test_golden_parity(golden, case, fused):
  c, name = cases.CASES[case], cases.tag(case)
  bins = golden[f'bins_{c.n}']
  inp = cases.inputs(case, bins)
  assert np.array_equal(golden[f'in_{name}'], cases.digest(inp))
  ref = cases.reference64(inp['logits'], bins, [])            # the scale of pred's bar only
  head = TwoHot(_cuda(inp['logits']), bins, fused=fused)
  assert head.fused is fused
  pred = head.pred()
  losses = [head.loss(_cuda(inp[f'target{k}'])) for k in range(cases.TARGETS)]
  assert pred.dtype == torch.float32 and pred.shape == (c.rows,)
  ratio = np.max(np.abs(pred.cpu().numpy().astype(np.float64) - golden[f'pred64_{name}']) / (1e-5 * (1 + ref['scale'])))
  worst = max(_loss_ratio(loss.cpu().numpy(), golden[f'loss64_{name}'][k]) for k, loss in enumerate(losses))
  print(f'{name} fused={fused}: pred {ratio:.3g} of its bar, loss {worst:.3g}')
  assert ratio <= 1.0 and worst <= 1.0
  last = losses[0][-1].item()                                   # the NaN target
  assert np.isnan(last) if c.n > 1 else last == 0.0
  assert torch.isfinite(losses[0][-3:-1]).all()                 # +-inf land on the outer bins


@pytest.mark.parametrize('n', [255, 256])
def test_zero_logits_predict_exactly_zero(n):
  head = TwoHot(torch.zeros(67, n, device='cuda'), symexp_twohot_bins(n), fused=True)
  pred = head.pred().cpu().numpy()
  assert pred.shape == (67,) and not pred.any(), pred[np.nonzero(pred)][:4]
  # and with any constant: the probabilities are equal, whatever they are
  head = TwoHot(torch.full((5, n), -3.25, device='cuda'), symexp_twohot_bins(n), fused=True)
  assert not head.pred().cpu().numpy().any()


@pytest.mark.parametrize('n', [255, 256, 2])
def test_target_on_a_bin_reads_that_logit(n):
  d = _shaped(n, 64)
  rng = np.random.default_rng(n)
  index = rng.integers(0, n, 64)
  index[:2] = (0, n - 1)
  if n == 256:
    index[index == 127] = 128          # of the two zero bins a target of 0 finds the upper one (bins <= t)
  head = TwoHot(_cuda(d['logits']), d['bins'], fused=True)
  loss = head.loss(_cuda(d['bins'][index])).cpu().numpy()
  lse = head._stats()[0].cpu().numpy()
  want = -(d['logits'][np.arange(64), index] - lse)
  ulp = np.spacing(np.abs(want).astype(np.float32))
  assert np.all(np.abs(loss - want) <= ulp), np.max(np.abs(loss - want) / ulp)
  assert _loss_ratio(lse, d['ref']['lse']) <= 1.0


@pytest.mark.parametrize('rows', [1, 3, 5, 1025])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 255, 256, 1024])
def test_shapes(n, rows):
  """Fewer rows than waves in a workgroup, not a multiple of it, many workgroups;
  every row width the kernels are instantiated for, full and partial last lanes."""
  d = _shaped(n, rows)
  coefs = (1.0, 0.7)
  logits = _cuda(d['logits']).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=True)
  pred = head.pred()
  loss = head.loss_sum([_cuda(t) for t in d['targets']], coefs)
  loss.backward(_cuda(d['gout']))
  ref = d['ref']
  want = sum(c * l for c, l in zip(coefs, ref['loss']))
  ratios = (_pred_ratio(pred.cpu().numpy(), ref), _loss_ratio(loss.detach().cpu().numpy(), want),
            _loss_ratio(logits.grad.cpu().numpy(), cases.grad64(ref, coefs, d['gout'])))
  print(f'{rows}x{n}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g}, grad {ratios[2]:.3g} of their bars')
  assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_second_sweep_of_the_capped_grid(kind):
  """The stats and grad kernels cover 8192 rows with one sweep of their capped
  grid (csrc/twohot.hip: kMaxBlocks workgroups of kWaves rows): row 8192 is the
  first of the grid stride's second iteration.  (The loss kernel's grid covers
  131 072 rows before it strides: its stride loop is NOT exercised by any test.)"""
  rows = 8193
  d = _shaped(255, rows)
  values = d['logits'] if kind == 'f32' else cases.bf16_round(d['logits'])
  key = ('sweep', kind)
  if key not in _SHAPED:
    _SHAPED[key] = cases.reference64(values, d['bins'], d['targets'])
  ref, coefs = _SHAPED[key], (1.0, 0.7)
  logits = _cuda(values).to(torch.float32 if kind == 'f32' else torch.bfloat16).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=True)
  pred = head.pred()
  loss = head.loss_sum([_cuda(t) for t in d['targets']], coefs)
  loss.backward(_cuda(d['gout']))
  want = cases.grad64(ref, coefs, d['gout'])
  grad = logits.grad.float().cpu().numpy().astype(np.float64)
  bar = 1e-5 + 1e-5 * np.abs(want) if kind == 'f32' else 2.0 ** -8 * np.abs(want) + 1e-5
  tail = slice(8192 - 4, rows)                                    # the seam between the sweeps, by itself too
  ratios = (_pred_ratio(pred.cpu().numpy(), ref),
            _loss_ratio(loss.detach().cpu().numpy(), sum(c * l for c, l in zip(coefs, ref['loss']))),
            float(np.max(np.abs(grad - want) / bar)), float(np.max((np.abs(grad - want) / bar)[tail])))
  print(f'{rows}x255 {kind}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g}, grad {ratios[2]:.3g} of their bars')
  assert max(ratios) <= 1.0, ratios
  assert np.abs(grad[-1]).max() > 0 and torch.isfinite(pred[-1]) and torch.isfinite(loss[-1])


def test_leading_shape_and_strided_logits():
  d = _shaped(255, 63)
  base = _cuda(d['logits'])
  wide = torch.zeros(7, 9, 300, device='cuda')
  wide[..., :255] = base.view(7, 9, 255)
  for logits in (base.view(7, 9, 255), wide[..., :255]):          # contiguous, and rows 300 floats apart
    logits = logits.detach().requires_grad_()
    head = TwoHot(logits, d['bins'])
    assert head.fused is True                                       # fused=None takes the kernels where they fit
    assert head.pred().shape == (7, 9)
    loss = head.loss(_cuda(d['targets'][0]).view(7, 9))
    assert loss.shape == (7, 9) and loss.dtype == torch.float32
    loss.backward(_cuda(d['gout']).view(7, 9))
    assert logits.grad.shape == (7, 9, 255)
    assert _pred_ratio(head.pred().reshape(-1).cpu().numpy(), d['ref']) <= 1.0
    assert _loss_ratio(loss.detach().reshape(-1).cpu().numpy(), d['ref']['loss'][0]) <= 1.0
    assert _loss_ratio(logits.grad.reshape(63, 255).cpu().numpy(), cases.grad64(d['ref'], (1.0,), d['gout'])) <= 1.0
  with pytest.raises(ValueError, match='target of shape'):
    head.loss(_cuda(d['targets'][0]))


def test_gradient_against_closed_form_and_composed_autograd():
  d = _shaped(255, 130)
  coefs = (1.0, 0.7)
  grads = {}
  for fused in (True, False):
    logits = _cuda(d['logits']).requires_grad_()
    head = TwoHot(logits, d['bins'], fused=fused)
    head.loss_sum([_cuda(t) for t in d['targets']], coefs).sum().backward()
    grads[fused] = logits.grad.cpu().numpy()
    assert logits.grad.dtype == torch.float32
  want = cases.grad64(d['ref'], coefs, np.ones(130))
  ratios = _loss_ratio(grads[True], want), _loss_ratio(grads[False], want), _loss_ratio(grads[True], grads[False])
  print(f'grad: fused {ratios[0]:.3g}, composed {ratios[1]:.3g} of the bar against float64; fused against composed {ratios[2]:.3g}')
  assert max(ratios) <= 1.0, ratios
  # softmax sums to 1 and so does every two-hot target
  sums = np.abs(grads[True].astype(np.float64).sum(-1))
  assert np.all(sums <= 255 * EPS32 * sum(abs(c) for c in coefs)), sums.max()
  # a grad_output that differs from row to row
  logits = _cuda(d['logits']).requires_grad_()
  TwoHot(logits, d['bins'], fused=True).loss_sum([_cuda(t) for t in d['targets']], coefs).backward(_cuda(d['gout']))
  assert _loss_ratio(logits.grad.cpu().numpy(), cases.grad64(d['ref'], coefs, d['gout'])) <= 1.0
  assert not np.array_equal(logits.grad.cpu().numpy(), grads[True])


def test_nan_target_gradient_is_nan_in_its_row_only():
  d = _shaped(63, 5)
  target = d['targets'][0].copy()
  target[2] = np.nan
  for fused in (True, False):
    logits = _cuda(d['logits']).requires_grad_()
    loss = TwoHot(logits, d['bins'], fused=fused).loss(_cuda(target))
    loss.sum().backward()
    bad = torch.isnan(logits.grad).all(-1).cpu().numpy()
    assert np.array_equal(bad, np.arange(5) == 2) and not torch.isnan(logits.grad[[0, 1, 3, 4]]).any()
    assert np.array_equal(torch.isnan(loss).cpu().numpy(), np.arange(5) == 2)


@pytest.mark.parametrize('n,rows', [(255, 130), (256, 5), (64, 33), (1024, 3)])
def test_bfloat16(n, rows):
  """bfloat16 logits against float64 over the bf16-rounded values: loss and pred
  at the float32 bars (the arithmetic is float32), the gradient within one
  bfloat16 rounding of them, 2^-8 |want| + 1e-5."""
  d = _shaped(n, rows)
  rounded = cases.bf16_round(d['logits'])
  ref = cases.reference64(rounded, d['bins'], d['targets'])
  coefs = (1.0, 0.7)
  want_loss = sum(c * l for c, l in zip(coefs, ref['loss']))
  want_grad = cases.grad64(ref, coefs, d['gout'])
  for fused in (True, False):
    logits = _cuda(rounded).to(torch.bfloat16).requires_grad_()
    assert np.array_equal(logits.detach().float().cpu().numpy(), rounded)
    head = TwoHot(logits, d['bins'], fused=fused)
    pred, loss = head.pred(), head.loss_sum([_cuda(t) for t in d['targets']], coefs)
    assert pred.dtype == loss.dtype == torch.float32
    loss.backward(_cuda(d['gout']))
    assert logits.grad.dtype == torch.bfloat16
    grad = logits.grad.float().cpu().numpy().astype(np.float64)
    ratios = (_pred_ratio(pred.cpu().numpy(), ref), _loss_ratio(loss.detach().cpu().numpy(), want_loss),
              float(np.max(np.abs(grad - want_grad) / (2.0 ** -8 * np.abs(want_grad) + 1e-5))))
    print(f'bf16 {rows}x{n} fused={fused}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g}, grad {ratios[2]:.3g} of their bars')
    assert max(ratios) <= 1.0, ratios


def test_no_rows():
  before = twohot_launches()
  for fused in (True, None, False):
    logits = torch.zeros(0, 255, device='cuda', requires_grad=True)
    head = TwoHot(logits, symexp_twohot_bins(255), fused=fused)
    pred, loss = head.pred(), head.loss(torch.zeros(0, device='cuda'))
    assert pred.shape == loss.shape == (0,) and pred.dtype == loss.dtype == torch.float32
    loss.sum().backward()
    assert logits.grad.shape == (0, 255)
    head = TwoHot(torch.zeros(4, 0, 64, device='cuda'), symexp_twohot_bins(64), fused=fused)
    assert head.pred().shape == (4, 0) and head.loss(torch.zeros(4, 0, device='cuda')).shape == (4, 0)
  assert twohot_launches() == before


def test_launch_counts():
  d = _shaped(255, 130)
  logits = _cuda(d['logits']).requires_grad_()
  targets = [_cuda(t) for t in d['targets']]
  torch.cuda.synchronize()
  before = twohot_launches()
  head = TwoHot(logits, d['bins'], fused=True)
  assert twohot_launches() == before                     # the constructor launches nothing
  pred = head.pred()
  assert twohot_launches() == before + 1
  loss = head.loss_sum(targets, (1.0, 0.7))
  assert twohot_launches() == before + 2
  loss.sum().backward()
  assert twohot_launches() == before + 3                 # pred, the loss of two targets, the gradient
  first = [t.clone() for t in (pred, loss.detach(), logits.grad)]
  again = head.pred()
  assert twohot_launches() == before + 3 and again.data_ptr() == pred.data_ptr()
  head.loss(targets[0])                                  # lse is kept too: the loss launch alone
  assert twohot_launches() == before + 4
  other = TwoHot(logits, d['bins'], fused=True)          # loss first: stats ride along, pred is then free
  other.loss(targets[0])
  assert twohot_launches() == before + 6
  other.pred()
  assert twohot_launches() == before + 6
  composed = TwoHot(logits, d['bins'], fused=False)
  composed.pred(), composed.loss(targets[0]).sum().backward()
  assert twohot_launches() == before + 6                 # the composed path launches none of the kernels
  # the same bits run to run: no atomics, no order left to the scheduler
  logits.grad = None
  head = TwoHot(logits, d['bins'], fused=True)
  loss2 = head.loss_sum(targets, (1.0, 0.7))
  loss2.sum().backward()
  assert torch.equal(head.pred(), first[0]) and torch.equal(loss2.detach(), first[1])
  assert torch.equal(logits.grad, first[2])


def test_more_bins_than_the_kernels_take():
  d = _shaped(1025, 3)
  with pytest.raises(ValueError, match=r'fused=True.*1025 bins.*at most 1024'):
    TwoHot(_cuda(d['logits']), d['bins'], fused=True)
  before = twohot_launches()
  logits = _cuda(d['logits']).requires_grad_()
  head = TwoHot(logits, d['bins'])
  assert head.fused is False
  pred, loss = head.pred(), head.loss_sum([_cuda(t) for t in d['targets']], (1.0, 0.7))
  loss.backward(_cuda(d['gout']))
  assert twohot_launches() == before
  ref = d['ref']
  assert _pred_ratio(pred.cpu().numpy(), ref) <= 1.0
  assert _loss_ratio(loss.detach().cpu().numpy(), ref['loss'][0] + 0.7 * ref['loss'][1]) <= 1.0
  assert _loss_ratio(logits.grad.cpu().numpy(), cases.grad64(ref, (1.0, 0.7), d['gout'])) <= 1.0
  with pytest.raises(ValueError, match='5 targets'):
    head.loss_sum([_cuda(d['targets'][0])] * 5, [1.0] * 5)
