"""The restatements of tests/recon_loss_cases.py, held against what they stand for
-- no GPU: the float64 restatement against the reference's own run
(tests/golden/recon_loss.npz), its autograd against the closed forms and central
differences, the float32 definition against both bars the GPU tests hold the
kernels to, and the new entry points' refusals."""
import ctypes as C
import pathlib

import numpy as np
import pytest

from embodied_amd import _lib
from embodied_amd.outs import MSE, Binary, ImageMSE, recon_loss_launches  # noqa: F401  (every test here fails without the feature)
from tests import recon_loss_cases as cases

GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'recon_loss.npz'


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def test_fixture_digests_match_the_regenerated_inputs(golden):
  for case in range(len(cases.CASES)):
    name = cases.tag(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(cases.inputs(case))), name
  assert GOLDEN.stat().st_size < 900_000


def test_restatement_equals_the_reference_run(golden):
  """rtol 1e-13 on every row and, up to 64 units, every element.  The sigmoid
  rows get one allowance on top: the reference run takes sigmoid(x) - t of a
  sigmoid that float64 has rounded at 2^-53, the restatement does not cancel
  there, so the two may differ by 2 |d| 2^-52 per term d^2."""
  elementwise = 0
  for case, c in enumerate(cases.CASES):
    name = cases.tag(case)
    inp = cases.inputs(case)
    got = cases.restate(c.op, inp['x'], inp['target'])
    slack = 2.0 ** -51 * np.sqrt(got['terms']) if c.op == 'sigmoid' else np.zeros_like(got['terms'])
    want = golden[f'loss_{name}']
    assert (np.abs(got['loss'] - want) <= 1e-13 * np.abs(want) + slack.sum(-1)).all(), name
    if c.units <= cases.ELEMENTWISE_MAX:
      want = golden[f'terms_{name}']
      assert (np.abs(got['terms'] - want) <= 1e-13 * np.abs(want) + slack).all(), name
      elementwise += 1
    else:
      assert f'terms_{name}' not in golden
  assert elementwise >= 40


def test_rounded_restatement_is_the_reference_run_around_its_sigmoid(golden):
  """The composed path's restatement is the reference's own arithmetic with the
  compute dtype's sigmoid in the place of the float64 one: it differs from the
  reference run by no more than that substitution, 2 |y - t| |y - sigmoid64(x)| per
  term, and the float32 sigmoid is within 2^-21 of the float64 one (four ulps: it
  is not a correctly rounded function; bfloat16: its rounding, 2^-8, on top)."""
  for case, c in enumerate(cases.CASES):
    if c.op != 'sigmoid':
      continue
    name = cases.tag(case)
    inp = cases.inputs(case)
    exact = 1 / (1 + np.exp(-inp['x'].astype(np.float64)))
    for kind, near in (('f32', 2.0 ** -21), ('bf16', 2.0 ** -8 + 2.0 ** -21)):
      x = inp['x'] if kind == 'f32' else cases.bf16_round(inp['x'])
      y = cases.sigmoid_of(x, kind).astype(np.float64)
      assert (np.abs(y - 1 / (1 + np.exp(-x.astype(np.float64)))) <= near * y + 2.0 ** -126).all(), (name, kind)   # (below 2^-126 float32 has no 24 bits)
      if kind == 'bf16':
        continue                                                     # (the fixture's run is of the unrounded x)
      got = cases.restate_rounded(c.op, x, inp['target'], kind=kind)
      d = np.abs(y - cases.t32(c.op, inp['target']).astype(np.float64))
      slack = (2 * d * np.abs(y - exact) + np.square(y - exact)).sum(-1)
      want = golden[f'loss_{name}']
      assert (np.abs(got['loss'] - want) <= 1e-13 * np.abs(want) + slack).all(), name


def test_autograd_is_the_closed_form_and_central_differences():
  rng = np.random.default_rng(5)
  for op in cases.OPS:
    for units in (1, 5, 70):
      for scale in cases.SCALES:
        d = cases.data(op, units, 3, scale, salt=11)
        auto = cases.restate(op, d['x'], d['target'], d['gout'])['grad']
        closed = cases.closed_form64(op, d['x'], d['target'], d['gout'])
        s = np.abs(closed).max()
        assert np.abs(auto - closed).max() <= 1e-12 * max(s, 1e-300), (op, units, scale)
        if scale > 5:
          continue                                                   # differences of a saturated sigmoid are all rounding
        x64, h = d['x'].astype(np.float64), 1e-6

        def f(x):
          e = np.exp(-np.abs(x))
          q = e / (1 + e)
          t = cases.t32(op, d['target']).astype(np.float64)
          if op == 'mse':
            terms = (x - t) ** 2
          elif op == 'symlog':
            terms = (x - np.sign(t) * np.log1p(np.abs(t))) ** 2
          elif op == 'sigmoid':
            terms = np.where(x >= 0, (1 - t) - q, q - t) ** 2
          else:
            soft = np.log1p(e)
            terms = -(t * (np.minimum(x, 0) - soft) + (1 - t) * (np.minimum(-x, 0) - soft))
          return (terms.sum(-1) * d['gout']).sum()

        flat = x64.reshape(-1)
        for at in rng.integers(0, flat.size, 6):
          up, down = flat.copy(), flat.copy()
          up[at] += h
          down[at] -= h
          numeric = (f(up.reshape(x64.shape)) - f(down.reshape(x64.shape))) / (2 * h)
          assert abs(numeric - auto.reshape(-1)[at]) <= 1e-6 * max(1.0, np.abs(auto).max()), (op, units, scale, at)


def test_float32_definition_stays_inside_both_bars():
  """Every case the GPU tests use, float32 and bfloat16-rounded x: the float32
  definition alone holds the loss bar and the gradient bar (printed)."""
  worst = {}
  for c in cases.GRID:
    for kind in cases.KINDS:
      d = cases.data(c.op, c.units, c.rows, c.scale, kind)
      want = cases.restate(c.op, d['x'], d['target'], d['gout'])
      got = cases.define32(c.op, d['x'], d['target'], d['gout'])
      loss = cases.loss_ratio(got['loss'], want)
      grad = cases.grad_ratio(got['grad'], want['grad'], cases.row_scale(want['grad']))
      if cases.loss_held(c.op, c.units):
        assert loss <= 1.0, (c, kind, loss)
      if cases.grad_held(c.op, c.units):
        assert grad <= 1.0, (c, kind, grad)
      w = worst.setdefault(c.op, [0.0, 0.0])
      w[0], w[1] = max(w[0], loss), max(w[1], grad)
  for op, (loss, grad) in worst.items():
    print(f'float32 definition, {op}: loss {loss:.3g} of its bar, gradient {grad:.3g} of its bar')
  assert not cases.LOSS_EXEMPT and not cases.GRAD_EXEMPT, 'the float32 definition holds both bars everywhere: none is exempt'


def test_composed_float32_definition_against_its_restatement():
  """The composed path's own float32 definition against the restatement that
  rounds sigmoid(x) and its backward where the reference does: inside both bars at
  every case, no family exempt."""
  worst = {}
  for c in cases.GRID:
    for kind in cases.KINDS:
      d = cases.data(c.op, c.units, c.rows, c.scale, kind)
      want = cases.restate_rounded(c.op, d['x'], d['target'], d['gout'], kind)
      got = cases.define32_composed(c.op, d['x'], d['target'], d['gout'], kind)
      loss = cases.loss_ratio(got['loss'], want)
      grad = cases.grad_ratio(got['grad'], want['grad'], cases.row_scale(want['grad']), kind == 'bf16')
      assert loss <= 1.0 and grad <= 1.0, (c, kind, loss, grad)
      w = worst.setdefault((c.op, kind), [0.0, 0.0])
      w[0], w[1] = max(w[0], loss), max(w[1], grad)
  for (op, kind), (loss, grad) in sorted(worst.items()):
    print(f'composed definition, {op} {kind}: loss {loss:.3g}, gradient {grad:.3g} of the bars')


def test_grid_covers_the_geometry_constants():
  header = (pathlib.Path(__file__).parent.parent / 'embodied_amd' / 'csrc' / 'recon_loss.h').read_text()
  assert f'kReconSegmentMaxUnits = {cases.SEGMENT_MAX};' in header
  assert f'kReconWaveMaxUnits = {cases.WAVE_MAX};' in header
  for bound in (cases.SEGMENT_MAX, cases.WAVE_MAX):
    assert {bound - 1, bound, bound + 1} <= set(cases.WIDTHS)
  for op in cases.OPS:
    for units in cases.WIDTHS:
      assert {c.scale for c in cases.GRID if (c.op, c.units) == (op, units)} == set(cases.SCALES)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
  raw = _lib.lib
  buf = np.zeros(64, np.float32)
  p = C.c_void_p(buf.ctypes.data)
  odd = C.c_void_p(buf.ctypes.data + 1)
  f = C.c_float
  i64 = C.c_int64

  def forward(x=p, xd=_lib.F32, t=p, td=_lib.F32, div=1.0, rows=2, units=3, op=_lib.EMB_RECON_MSE, loss=p):
    return raw.emb_recon_loss(x, xd, t, td, f(div), i64(rows), i64(units), op, loss, None)

  def backward(x=p, xd=_lib.F32, t=p, td=_lib.U8, div=255.0, rows=2, units=3, op=_lib.EMB_RECON_SIGMOID_MSE, gout=p,
               grad=p):
    return raw.emb_recon_loss_grad(x, xd, t, td, f(div), i64(rows), i64(units), op, gout, grad, None)

  def refused(status, word):
    assert status == _lib.ERR_INVALID, status
    assert word in raw.emb_last_error().decode(), raw.emb_last_error()

  for call in (forward, backward):
    who = 'recon_loss_grad' if call is backward else 'recon_loss'
    refused(call(x=None), f'{who}: a pointer is null')
    refused(call(t=None), 'null')
    refused(call(units=0), f'{who}: units must be at least 1')
    refused(call(op=4), 'op must be one of')
    refused(call(op=-1), 'op must be one of')
    refused(call(rows=2 ** 31 - 1, units=2), 'more than 2^31 - 1 elements')
    refused(call(rows=1, units=2 ** 31), 'more than 2^31 - 1 elements')
    refused(call(rows=-1), 'negative rows')
    refused(call(xd=_lib.U8), 'x_dtype')
    refused(call(td=_lib.I32), 'target_dtype')
    refused(call(div=0.0), 'div')
    refused(call(x=odd), 'x is not aligned')
    assert call(x=None, t=None, rows=0) == _lib.OK                   # no rows: nothing to do, nothing launched
  refused(forward(loss=None), 'null')
  refused(backward(gout=None), 'null')
  refused(backward(grad=None), 'null')
  refused(backward(grad=odd), 'grad is not aligned')
  refused(raw.emb_recon_loss_launches(None), 'count is null')
  assert forward(t=odd, td=_lib.U8, rows=0) == _lib.OK
  before = recon_loss_launches()
  assert before >= 0 and recon_loss_launches() == before


def test_python_heads_refuse_what_they_do_not_take():
  import torch
  x = torch.zeros(3, 4)
  for make in (lambda: MSE(x), lambda: ImageMSE(x), lambda: Binary(x)):
    with pytest.raises(RuntimeError, match='no CPU fallback'):
      make()
