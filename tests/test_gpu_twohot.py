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
the kernels: profiles/twohot_accuracy.txt.

Sums of three and four targets with coefficients of both signs are held to the
same 1e-5 on their own condition scale, 1 + sum_k |c_k| |loss_k| (the gradient:
1 + sum_k |c_k| (p_i + twohot_k,i), times |gout|): `_sum_bars`.

Non-finite logits: the composed path is the definition, -(twohot * log_pred)
summed over the whole row, so a -inf logit under a zero weight makes the loss
NaN; the fused loss reads the row's two logits at `below` and `above` alone and
is `reference64`'s `loss2` there (the TwoHot docstring)."""
import pathlib
import re

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
  131 072 rows before it strides: `test_loss_rows_beyond_one_sweep`.)"""
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


# ---- three and four targets, the loss kernel's stride, other bins, non-finite
# logits, autograd use: what the tests above never reach

COEFS4 = (1.0, 0.7, -0.25, 0.0)
BF16_GRAD = 2.0 ** -8


def _tensor(values, kind):
  return _cuda(values).to(torch.float32 if kind == 'f32' else torch.bfloat16)


def _match(got, want, bar):
  """Worst |got - want| / bar over the finite part of `want`; NaN, +inf and -inf
  exactly where `want` has them."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  bar = np.broadcast_to(np.asarray(bar, np.float64), want.shape)
  assert got.shape == want.shape, (got.shape, want.shape)
  for name, test in (('NaN', np.isnan), ('+inf', np.isposinf), ('-inf', np.isneginf)):
    assert np.array_equal(test(got), test(want)), (name, np.argwhere(test(got) != test(want))[:8].tolist())
  ok = np.isfinite(want)
  assert np.all(bar[ok] > 0)
  return float(np.max(np.abs(got[ok] - want[ok]) / bar[ok], initial=0.0))


def _sum_bars(ref, coefs, gout, picks=None):
  """float64 (loss, its bar, gradient, its bar) of sum_k coefs[k] * loss_{picks[k]}."""
  picks = range(len(coefs)) if picks is None else picks
  loss = sum(c * ref['loss'][k] for c, k in zip(coefs, picks))
  loss_bar = 1e-5 * (1 + sum(abs(c) * np.abs(ref['loss'][k]) for c, k in zip(coefs, picks)))
  hot = sum(c * ref['twohot'][k] for c, k in zip(coefs, picks))
  g = np.asarray(gout, np.float64)[..., None]
  grad = g * (sum(coefs) * ref['probs'] - hot)
  scale = sum(abs(c) * (ref['probs'] + ref['twohot'][k]) for c, k in zip(coefs, picks))
  return loss, loss_bar, grad, 1e-5 * (1 + scale) * np.abs(g)


def _multi(n, rows, kind):
  """`_shaped` with four target sets, over float32 or bfloat16-rounded logits."""
  key = ('multi', n, rows, kind)
  if key not in _SHAPED:
    rng = np.random.default_rng([n, rows, 4])
    bins = symexp_twohot_bins(n)
    logits = np.concatenate([cases.logits_of(k, -(-rows // 4), n, rng) for k in cases.KINDS])[:rows]
    logits = logits[rng.permutation(rows)]
    if kind == 'bf16':
      logits = cases.bf16_round(logits)
    targets = [cases.targets_of(rows, bins, rng, special=False) for _ in range(4)]
    gout = rng.standard_normal(rows).astype(np.float32)
    ref = cases.reference64(logits, bins, targets)
    for a in (logits, gout, *targets):
      a.setflags(write=False)
    _SHAPED[key] = dict(bins=bins, logits=logits, targets=targets, gout=gout, ref=ref)
  return _SHAPED[key]


def _run_sum(d, kind, fused, targets, coefs, gout=None):
  """(loss, grad) as float64 numpy of `loss_sum(targets, coefs)` and its backward."""
  logits = _tensor(d['logits'], kind).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=fused)
  loss = head.loss_sum([_cuda(t) for t in targets], coefs)
  loss.backward(_cuda(d['gout'] if gout is None else gout))
  assert loss.dtype == torch.float32 and logits.grad.dtype == logits.dtype
  return loss.detach().cpu().numpy().astype(np.float64), logits.grad.float().cpu().numpy().astype(np.float64)


@PATHS
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('rows,n', [(5, 63), (67, 255), (1025, 2)])
@pytest.mark.parametrize('k', [3, 4])
def test_three_and_four_targets(k, rows, n, kind, fused):
  """Slots 2 and 3 of the launch: fewer rows than a workgroup's lanes / 4, a row
  count that leaves a wave's last rows partial, many workgroups.  Coefficients
  (1, 0.7, -0.25, 0)[:k]; bars on the sums' condition scales (`_sum_bars`).  The
  composed formula restated in float32 numpy over these seeds
  (`tests.twohot_cases.composed32`, held to the same bars by the host test)
  reaches at worst 0.054 of the loss bar and 0.048 of the gradient bar."""
  d = _multi(n, rows, kind)
  ref, coefs = d['ref'], COEFS4[:k]
  extra = (lambda want: BF16_GRAD * np.abs(want) + 1e-5) if kind == 'bf16' else (lambda want: 0.0)

  def check(picks, cs, what):
    want_loss, loss_bar, want_grad, grad_bar = _sum_bars(ref, cs, d['gout'], picks)
    loss, grad = _run_sum(d, kind, fused, [d['targets'][i] for i in picks], cs)
    ratios = _match(loss, want_loss, loss_bar), _match(grad, want_grad, grad_bar + extra(want_grad))
    print(f'{what} k={len(cs)} {rows}x{n} {kind} fused={fused}: loss {ratios[0]:.3g}, grad {ratios[1]:.3g} of their bars')
    assert max(ratios) <= 1.0, (what, ratios)
    return loss, grad

  loss, grad = check(tuple(range(k)), coefs, 'sum')
  if k < 4:
    # a NaN target in slot 2, row 1: that row and no other, loss and gradient
    bad = [t.copy() for t in d['targets'][:k]]
    bad[2][1] = np.nan
    nan_loss, nan_grad = _run_sum(d, kind, fused, bad, coefs)
    only = np.arange(rows) == 1
    assert np.array_equal(np.isnan(nan_loss), only) and np.array_equal(np.isnan(nan_grad), np.broadcast_to(only[:, None], (rows, n)))
    assert np.array_equal(nan_loss[~only], loss[~only]) and np.array_equal(nan_grad[~only], grad[~only])
    return
  # the slots: every pairing of the (target, coefficient) pairs follows its own float64 value ...
  for perm in ((3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1)):
    check(perm, tuple(coefs[i] for i in perm), f'permuted {perm}')
  # ... and the coefficients stay with their slots, not their targets
  swapped, _ = check((1, 0, 2, 3), coefs, 'targets 0 and 1 swapped')
  gap = np.abs(swapped - loss) / _sum_bars(ref, coefs, d['gout'])[1]
  assert np.mean(gap > 100) > 0.2, np.mean(gap > 100)           # (n = 2: half the targets share their weights)
  if not fused:
    return
  logits = _tensor(d['logits'], kind).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=True)
  targets = [_cuda(t) for t in d['targets']]
  head.pred()
  before = twohot_launches()
  total = head.loss_sum(targets, coefs)
  total.backward(_cuda(d['gout']))
  assert twohot_launches() == before + 2                       # four targets: one launch forward, one backward
  # a zero coefficient with a finite target adds exactly nothing
  assert np.array_equal(total.detach().cpu().numpy().astype(np.float64), loss)
  three = logits.detach().clone().requires_grad_()
  less = TwoHot(three, d['bins'], fused=True).loss_sum(targets[:3], coefs[:3])
  less.backward(_cuda(d['gout']))
  assert torch.equal(less, total.detach()) and torch.equal(three.grad, logits.grad)
  # the documented order of addition, ((t0 + t1) + t2) + t3, to the bit
  t = [head.loss(target).detach() for target in targets]
  ones = head.loss_sum(targets, (1.0, 1.0, 1.0, 1.0)).detach()
  assert torch.equal(ones, ((t[0] + t[1]) + t[2]) + t[3])
  if rows >= 67:    # and the terms differ enough in magnitude for another order to show
    assert not torch.equal(ones, ((t[0] + t[1]) + t[3]) + t[2])
    assert not torch.equal(ones, t[0] + (t[1] + (t[2] + t[3])))


def _kernel_constants():
  text = (pathlib.Path(__file__).resolve().parent.parent / 'embodied_amd' / 'csrc' / 'twohot.hip').read_text()
  return {name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1)) for name in ('kWave', 'kWaves', 'kMaxBlocks')}


@pytest.mark.parametrize('n,kind', [(3, 'f32'), (2, 'bf16')])
def test_loss_rows_beyond_one_sweep(n, kind):
  """The loss kernel gives TWOHOT_MAX_TARGETS = 4 lanes to a row: its capped grid
  of kMaxBlocks workgroups of kWave * kWaves lanes (csrc/twohot.hip, read here)
  covers 2048 * 256 / 4 = 131 072 rows in one sweep, so row 131 072 is the first
  one of the stride loop's second iteration (and the 17th sweep of the stats and
  grad kernels)."""
  from embodied_amd.outs import TWOHOT_MAX_TARGETS
  k = _kernel_constants()
  sweep = k['kMaxBlocks'] * k['kWave'] * k['kWaves'] // TWOHOT_MAX_TARGETS
  assert sweep == 131072, k
  rows = sweep + 1
  d = _shaped(n, rows)
  values = d['logits'] if kind == 'f32' else cases.bf16_round(d['logits'])
  key = ('stride', n, kind)
  if key not in _SHAPED:
    _SHAPED[key] = cases.reference64(values, d['bins'], d['targets'])
  ref, coefs = _SHAPED[key], (1.0, 0.7)
  logits = _tensor(values, kind).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=True)
  pred = head.pred()
  loss = head.loss_sum([_cuda(t) for t in d['targets']], coefs)
  loss.backward(_cuda(d['gout']))
  want_loss = sum(c * l for c, l in zip(coefs, ref['loss']))
  want = cases.grad64(ref, coefs, d['gout'])
  grad = logits.grad.float().cpu().numpy().astype(np.float64)
  got_loss = loss.detach().cpu().numpy()
  bar = 1e-5 + 1e-5 * np.abs(want) if kind == 'f32' else BF16_GRAD * np.abs(want) + 1e-5
  seam = slice(sweep - 4, rows)                                   # rows 131 068 .. 131 072, by themselves too
  ratios = (_pred_ratio(pred.cpu().numpy(), ref), _loss_ratio(got_loss, want_loss),
            _loss_ratio(got_loss[seam], want_loss[seam]), float(np.max(np.abs(grad - want) / bar)),
            float(np.max((np.abs(grad - want) / bar)[seam])))
  print(f'{rows}x{n} {kind}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g} (seam {ratios[2]:.3g}), '
        f'grad {ratios[3]:.3g} (seam {ratios[4]:.3g}) of their bars')
  assert max(ratios) <= 1.0, ratios
  assert np.isfinite(got_loss[-1]) and got_loss[-1] != 0 and np.abs(want_loss[-1]) > 1e-3
  assert np.abs(want_loss[seam]).min() > 1e-3                     # no row of the seam would pass as an unwritten zero


def _custom(binkind, n):
  key = ('custom', binkind, n)
  if key not in _SHAPED:
    rows = 37
    rng = np.random.default_rng([n, rows, ('asym', 'ties', 'symexp').index(binkind)])
    bins = cases.edge_bins(binkind, n, symexp_twohot_bins)
    logits = np.concatenate([cases.logits_of(k, -(-rows // 4), n, rng) for k in cases.KINDS])[:rows]
    logits = logits[rng.permutation(rows)]
    targets = [cases.edge_targets(rows, bins, rng, zeros=binkind == 'symexp' and i == 0) for i in range(2)]
    # and a target between every neighbouring pair (equal neighbours: inside the run), rows at a time
    frac = rng.uniform(0.05, 0.95, n - 1)
    between = (bins[:-1].astype(np.float64) + frac * (bins[1:].astype(np.float64) - bins[:-1])).astype(np.float32)
    between = np.resize(between, -(-(n - 1) // rows) * rows).reshape(-1, rows)
    gout = rng.standard_normal(rows).astype(np.float32)
    _SHAPED[key] = dict(bins=bins, logits=logits, targets=targets, gout=gout, between=between,
                        ref=cases.reference64(logits, bins, targets),
                        between_loss=np.stack(cases.reference64(logits, bins, between)['loss']))
  return _SHAPED[key]


@PATHS
@pytest.mark.parametrize('n', [6, 7, 64, 255, 1024])
@pytest.mark.parametrize('binkind', ['asym', 'ties', 'symexp'])
def test_custom_bins(binkind, n, fused):
  """Bins that are not antisymmetric (pred's mirrored pairs do not cancel, the
  odd n's middle bin is not 0), runs of equal neighbours and equal outer bins,
  the symexp set: targets on a bin, between EVERY neighbouring pair, beyond
  both ends, inside a run of ties (`cases.edge_targets`).  `reference64` is held
  against the reference's class on these bin sets by the host test."""
  d = _custom(binkind, n)
  ref, coefs = d['ref'], (1.0, 0.7)
  assert binkind == 'symexp' or not np.array_equal(d['bins'], -d['bins'][::-1])
  logits = _cuda(d['logits']).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=fused)
  pred = head.pred()
  loss = head.loss_sum([_cuda(t) for t in d['targets']], coefs)
  loss.backward(_cuda(d['gout']))
  between = np.stack([head.loss(_cuda(t)).detach().cpu().numpy() for t in d['between']])
  ratios = (_pred_ratio(pred.cpu().numpy(), ref),
            _loss_ratio(loss.detach().cpu().numpy(), sum(c * l for c, l in zip(coefs, ref['loss']))),
            _loss_ratio(logits.grad.cpu().numpy(), cases.grad64(ref, coefs, d['gout'])),
            _loss_ratio(between, d['between_loss']))
  print(f'{binkind}{n} fused={fused}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g}, grad {ratios[2]:.3g}, '
        f'between every pair {ratios[3]:.3g} of their bars')
  assert max(ratios) <= 1.0, ratios
  if binkind == 'symexp' and n % 2 == 0 and fused:
    # 0.0 and -0.0 against the bins' own 0.0, -0.0: both zeros count as <= t, the upper one is `below`
    assert d['bins'][n // 2 - 1] == 0 and d['bins'][n // 2] == 0 and np.signbit(d['bins'][n // 2])
    lse = head._stats()[0].cpu().numpy()
    want = -(d['logits'][:, n // 2] - lse)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    for zero in (0.0, -0.0):
      got = head.loss(_cuda(np.full(37, zero, np.float32))).detach().cpu().numpy()
      assert np.all(np.abs(got - want) <= ulp), (zero, np.max(np.abs(got - want) / ulp))


def _nonfinite(n, kind):
  key = ('nonfinite', n, kind)
  if key not in _SHAPED:
    rows = len(cases.EDGE_KINDS)
    rng = np.random.default_rng([n, rows, 9])
    bins = symexp_twohot_bins(n)
    pair = rng.integers(0, n - 1, rows)
    mid = (bins[pair].astype(np.float64) + rng.uniform(0.2, 0.8, rows) * (bins[pair + 1].astype(np.float64) - bins[pair]))
    # between a pair (both weights positive), and on that pair's lower bin (the upper one's weight is 0)
    targets = [mid.astype(np.float32), bins[pair].copy()]
    logits = cases.edge_logits('edge', rows, bins, targets[0], rng)
    if kind == 'bf16':
      logits = cases.bf16_round(logits)
    gout = rng.standard_normal(rows).astype(np.float32)
    _SHAPED[key] = dict(bins=bins, logits=logits, targets=targets, gout=gout, ref=cases.reference64(logits, bins, targets))
  return _SHAPED[key]


def _grad_bar(want, kind):
  return 1e-5 + 1e-5 * np.abs(want) if kind == 'f32' else BF16_GRAD * np.abs(want) + 1e-5


@PATHS
@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('n', [63, 255])
def test_nonfinite_logits(n, kind, fused):
  """Rows of `cases.EDGE_KINDS`: one -inf logit in the first target's `below`
  bin, in its `above` bin, elsewhere; all -inf; one +inf; one NaN; |x| up to 1e4;
  N(0,1).  NaN, +inf and -inf exactly where float64 has them, the rest within
  the bars.  The loss of a row with a -inf logit is where the paths differ BY
  DESIGN: composed is the definition (`loss`: NaN unless the -inf bin
  carries weight), fused reads two logits (`loss2`: a -inf elsewhere is not seen)."""
  d = _nonfinite(n, kind)
  ref, coefs = d['ref'], (1.0, 0.7)
  want_loss = ref['loss2'] if fused else ref['loss']
  kinds = list(cases.EDGE_KINDS)
  elsewhere = kinds.index('ninf_else')
  assert np.isnan(ref['loss'][0][elsewhere]) and np.isfinite(ref['loss2'][0][elsewhere])
  assert np.isposinf(ref['loss'][0][kinds.index('ninf_below')]) and np.isposinf(ref['loss2'][0][kinds.index('ninf_below')])
  assert np.isnan(ref['loss2'][1][kinds.index('ninf_above')])     # 0 * -inf inside the two bins: NaN on both paths
  want_grad = cases.grad64(ref, coefs, d['gout'])
  assert np.isnan(want_grad[[kinds.index(k) for k in ('all_ninf', 'pinf', 'nan')]]).all()
  assert np.isfinite(np.delete(want_grad, [kinds.index(k) for k in ('all_ninf', 'pinf', 'nan')], 0)).all()

  def run(values):
    logits = _tensor(values['logits'], kind).requires_grad_()
    head = TwoHot(logits, d['bins'], fused=fused)
    out = dict(pred=head.pred(), loss0=head.loss(_cuda(values['targets'][0])).detach(),
               loss1=head.loss(_cuda(values['targets'][1])).detach())
    if fused:
      out['lse'] = head._stats()[0]
    head.loss_sum([_cuda(t) for t in values['targets']], coefs).backward(_cuda(values['gout']))
    out['grad'] = logits.grad
    return out

  got = run(d)
  np64 = lambda t: t.float().cpu().numpy().astype(np.float64)
  ratios = dict(pred=_match(np64(got['pred']), ref['pred'], 1e-5 * (1 + np.nan_to_num(ref['scale']))),
                loss0=_match(np64(got['loss0']), want_loss[0], ATOL + RTOL * np.abs(np.nan_to_num(want_loss[0], posinf=0))),
                loss1=_match(np64(got['loss1']), want_loss[1], ATOL + RTOL * np.abs(np.nan_to_num(want_loss[1], posinf=0))),
                grad=_match(np64(got['grad']), want_grad, _grad_bar(np.nan_to_num(want_grad), kind)))
  if fused:
    ratios['lse'] = _match(np64(got['lse']), ref['lse'], ATOL + RTOL * np.abs(np.nan_to_num(ref['lse'])))
  print(f'non-finite 8x{n} {kind} fused={fused}: ' + ', '.join(f'{k} {v:.3g}' for k, v in ratios.items()) + ' of their bars')
  assert max(ratios.values()) <= 1.0, ratios
  if fused:
    # the finite rows stand between poisoned ones in the same wave (loss) and the
    # same workgroup (stats, grad): the same bits as when they run alone
    clean = [i for i, bad in enumerate(cases.POISONED) if not bad]
    alone = run(dict(logits=d['logits'][clean], targets=[t[clean] for t in d['targets']], gout=d['gout'][clean]))
    for name, value in alone.items():
      assert torch.isfinite(value.float()).all(), name
      assert torch.equal(value, got[name][clean]), name


@PATHS
@pytest.mark.parametrize('kind,top', [('f32', 1e4), ('bf16', 1e30)])
def test_extreme_logits(kind, top, fused):
  """f32 logits of 1e4 * N(0,1); bf16 logits of either sign with |x| log-uniform
  up to 1e30.  Every float64 value of these seeds is finite and inside float32's
  range (worst |loss| 1.8e30)."""
  key = ('extreme', kind)
  if key not in _SHAPED:
    rows, n = 8, 63
    rng = np.random.default_rng([rows, n, int(np.log10(top))])
    bins = symexp_twohot_bins(n)
    if kind == 'f32':
      logits = (1e4 * rng.standard_normal((rows, n))).astype(np.float32)
    else:
      logits = cases.bf16_round((rng.choice([-1.0, 1.0], (rows, n)) * 10.0 ** rng.uniform(0, 30, (rows, n))).astype(np.float32))
    targets = [cases.targets_of(rows, bins, rng, special=False) for _ in range(2)]
    gout = rng.standard_normal(rows).astype(np.float32)
    _SHAPED[key] = dict(bins=bins, logits=logits, targets=targets, gout=gout, ref=cases.reference64(logits, bins, targets))
  d = _SHAPED[key]
  ref, coefs = d['ref'], (1.0, 0.7)
  assert np.abs(d['logits']).max() > top / 10
  logits = _tensor(d['logits'], kind).requires_grad_()
  head = TwoHot(logits, d['bins'], fused=fused)
  pred = head.pred()
  loss = head.loss_sum([_cuda(t) for t in d['targets']], coefs)
  loss.backward(_cuda(d['gout']))
  want_loss, want_grad = sum(c * l for c, l in zip(coefs, ref['loss'])), cases.grad64(ref, coefs, d['gout'])
  assert all(np.isfinite(w).all() and np.abs(w).max() < 3e38 for w in (ref['pred'], want_loss, want_grad, ref['lse']))
  ratios = (_pred_ratio(pred.cpu().numpy(), ref), _loss_ratio(loss.detach().cpu().numpy(), want_loss),
            _match(logits.grad.float().cpu().numpy(), want_grad, _grad_bar(want_grad, kind)))
  print(f'|x| to {top:g} {kind} fused={fused}: pred {ratios[0]:.3g}, loss {ratios[1]:.3g}, grad {ratios[2]:.3g} of their bars')
  assert max(ratios) <= 1.0, ratios


def test_two_loss_calls_accumulate_and_broadcast_grad_output():
  d = _shaped(255, 130)
  coefs = (1.0, 0.7)
  targets = [_cuda(t) for t in d['targets']]
  want = cases.grad64(d['ref'], coefs, np.ones(130))
  one = _cuda(d['logits']).requires_grad_()
  TwoHot(one, d['bins'], fused=True).loss_sum(targets, coefs).sum().backward()
  two = _cuda(d['logits']).requires_grad_()
  before = twohot_launches()
  head = TwoHot(two, d['bins'], fused=True)
  (head.loss(targets[0]) + 0.7 * head.loss(targets[1])).sum().backward()
  assert twohot_launches() == before + 5                  # stats, two loss launches, two gradients that autograd adds
  ratios = _loss_ratio(one.grad.cpu().numpy(), want), _loss_ratio(two.grad.cpu().numpy(), want)
  print(f'two calls: loss_sum {ratios[0]:.3g}, loss + 0.7 * loss {ratios[1]:.3g} of the gradient bar')
  assert max(ratios) <= 1.0, ratios
  # .sum() and .mean() hand backward a broadcast scalar: the same bits as the filled-out gout
  for reduce, fill in ((torch.sum, 1.0), (torch.mean, 1.0 / 130)):
    a, b = (_cuda(d['logits']).requires_grad_() for _ in range(2))
    reduce(TwoHot(a, d['bins'], fused=True).loss_sum(targets, coefs)).backward()
    TwoHot(b, d['bins'], fused=True).loss_sum(targets, coefs).backward(torch.full((130,), fill, device='cuda'))
    assert torch.equal(a.grad, b.grad) and a.grad.abs().max() > 0
    assert fill != 1.0 or torch.equal(a.grad, one.grad)


def test_zero_and_infinite_grad_output():
  """gout = 0: every element of the row is a zero, with the sign IEEE gives 0 * x
  (the float64 closed form's and autograd's own), never NaN.  gout = inf: +-inf
  with the sign of the closed form."""
  d = _shaped(63, 37)          # N(0,1), 8 N(0,1), peaked, zero rows; rows 9 and 12 are N(0,1) rows: no probability underflows
  coefs = (1.0, 0.7)
  gout = d['gout'].copy()
  gout[[0, 5, 36]] = 0.0
  gout[[9, 12]] = np.inf, -np.inf
  with np.errstate(invalid='ignore'):
    want = cases.grad64(d['ref'], coefs, gout)
  inner = cases.grad64(d['ref'], coefs, np.ones(37))
  # float32 cannot land on zero or on its other side: nothing of the inf rows underflows, no element cancels
  scale = sum(coefs) * d['ref']['probs'] + sum(c * t for c, t in zip(coefs, d['ref']['twohot']))
  assert np.abs(inner[[9, 12]]).min() > 1e-6 and not np.isnan(want).any()
  assert np.all(np.abs(inner[[0, 5, 9, 12, 36]]) >= 1e-3 * scale[[0, 5, 9, 12, 36]])
  logits = _cuda(d['logits']).requires_grad_()
  TwoHot(logits, d['bins'], fused=True).loss_sum([_cuda(t) for t in d['targets']], coefs).backward(_cuda(gout))
  grad = logits.grad.cpu().numpy()
  assert _match(grad, want, 1e-5 + 1e-5 * np.abs(np.nan_to_num(want, posinf=0, neginf=0))) <= 1.0
  zero = grad[[0, 5, 36]]
  assert not zero.any() and not np.isnan(zero).any()
  assert np.array_equal(np.signbit(zero), np.signbit(want[[0, 5, 36]]))


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
def test_logits_at_an_element_offset(kind):
  """Logits that start one element into an allocation (4-byte aligned float32,
  2-byte aligned bfloat16): the same bits as from a fresh tensor."""
  rows, n = 33, 255
  d = _shaped(n, rows)
  values = _tensor(d['logits'], kind)
  big = torch.zeros(rows * n + 9, device='cuda', dtype=values.dtype)
  big[1:1 + rows * n] = values.reshape(-1)
  results = []
  for source in (values.clone(), big[1:1 + rows * n].view(rows, n)):
    logits = source.detach().requires_grad_()
    head = TwoHot(logits, d['bins'], fused=True)
    assert head._x.data_ptr() == source.data_ptr()                # no copy: the kernels read it where it lies
    pred = head.pred()
    loss = head.loss_sum([_cuda(t) for t in d['targets']], (1.0, 0.7))
    loss.backward(_cuda(d['gout']))
    results.append((source.data_ptr(), pred, loss.detach(), logits.grad))
  (aligned, *first), (offset, *second) = results
  assert aligned % 16 == 0 and offset % 16 == values.element_size()
  for a, b in zip(first, second):
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
