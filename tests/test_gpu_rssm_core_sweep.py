"""The paths of the norm + activation and blocked GRU gate kernels
(csrc/norm_act.hip, csrc/gru_gate.hip) that tests/test_gpu_norm_act.py and
tests/test_gpu_gru_gate.py leave untried, at the tables of
tests/rssm_core_sweep_cases.py (tests/test_rssm_core_sweep_host.py shows on the
CPU that they reach the paths they name).  Need a GPU.

  A, B  views that do not start on 16 bytes, at widths that vectorise: the
        element-by-element instantiations at model widths, one pointer moved at
        a time and all together, bit for bit the aligned run
  C     more rows than one pass of the capped grid: tiled rows, every row bit
        for bit the small run's, the column sums against the float64 sums
        weighted by each distinct row's multiplicity
  D     null outputs: each output that is asked for bit for bit the run with all
  E     outputs inside buffers filled with 7: nothing around them is written,
        all of them is, the inputs are left as they were

The entry points are called on device pointers (`_lib.api.emb_norm_act*`,
`_lib.api.emb_gru_gate*`), as tests/test_gpu_recon_loss.py does, and through
`nets.norm_act` / `nets.gru_gate`.  Every aligned run is held to the float64
restatements under the bars of tests/norm_act_cases.py and
tests/gru_gate_cases.py, unchanged; everything else is compared with it bit for
bit (`view(torch.int32)` / `view(torch.int16)`).  Why that holds between the
16-byte and the per-element kernels: `Map::index` and `place` give a thread the
same elements either way, it adds them in the same order, and both files compile
with fp contract(off)."""
import numpy as np
import pytest
import torch

from embodied_amd import _lib, nets
from tests import gru_gate_cases as gates
from tests import norm_act_cases as norms
from tests import rssm_core_sweep_cases as sweep

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize('kind', sweep.KINDS)
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
CODES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}
F32 = torch.float32


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _dev(array, kind='f32'):
  if array is None:
    return None
  t = torch.from_numpy(np.array(array, order='C')).cuda().to(TORCH[kind])       # a copy: the cases' arrays are read-only
  assert t.data_ptr() % 16 == 0                                      # a fresh tensor starts on 16 bytes
  return t


def _host(t):
  return t.detach().float().cpu().numpy()


def _hosts(got):
  return {k: _host(v) for k, v in got.items() if k != 'partials'}


def _bits(t):
  return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _addr(t):
  return None if t is None else t.data_ptr()


def _shifted(t, by=1):
  """The same values in a contiguous view that starts `by` elements into a larger buffer."""
  if t is None or not by:
    return t
  buf = torch.empty(t.numel() + by + 3, dtype=t.dtype, device=t.device)
  assert buf.data_ptr() % 16 == 0
  view = buf[by:by + t.numel()].view(t.shape)
  view.copy_(t)
  assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + by * t.element_size()
  assert view.data_ptr() % 16 != 0
  return view


def _step(dtype, step):
  """Elements of `dtype` to move a pointer by: one element, or 8 bytes (on 8, not on 16)."""
  return 1 if step == 'element' else 8 // torch.empty(0, dtype=dtype).element_size()


def _steps(kind):
  return ('element', 'eight') if kind == 'bf16' else ('element',)


def _unchanged(tensors, kept):
  return all(_same(tensors[k], kept[k]) for k in kept)


def _clones(tensors):
  return {k: v.clone() for k, v in tensors.items() if v is not None}


# --- norm_act on device pointers ----------------------------------------------------------------


def _norm_tensors(inp, kind):
  return {'x': _dev(inp['x'], kind), 'gout': _dev(inp['gout'], kind), 'scale': _dev(inp['scale']), 'shift': _dev(inp['shift'])}


def _norm_raw(t, impl, act, out=None, dx=None, dscale=None, dshift=None, partials=None, floats=None):
  """The forward into `out` if given, then the gradient into what else is given."""
  x = t['x']
  rows, units = x.shape
  head = (x.data_ptr(), _addr(t['scale']), _addr(t['shift']))
  tail = (rows, units, nets.IMPLS[impl], nets.ACTS[act], sweep.EPS)
  stream = _lib.raw_stream(x.device)
  if out is not None:
    _lib.api.emb_norm_act(*head, CODES[x.dtype], *tail, out.data_ptr(), stream)
  if dx is not None or dscale is not None or dshift is not None:
    if floats is None:
      floats = 0 if partials is None else partials.numel()
    _lib.api.emb_norm_act_grad(*head, t['gout'].data_ptr(), CODES[x.dtype], *tail, _addr(dx), _addr(dscale), _addr(dshift),
                               _addr(partials), floats, stream)


def _partial_floats(rows, units):
  return 2 * sweep.partial_rows(rows, units) * units


def _run_norm(t, impl, act, moved=(), step='element', outputs=('out', 'dx', 'dscale', 'dshift')):
  """`outputs` of one forward and one gradient call; the pointers named in `moved`
  (of sweep.NORM_POINTERS) are views off 16 bytes, the others fresh tensors.  With
  dscale or dshift: `partials` of exactly the floats the library asks for, returned too."""
  x = t['x']
  rows, units = x.shape
  by = lambda name, dtype: _step(dtype, step) if name in moved else 0
  call = {k: None if v is None else _shifted(v, by(k, v.dtype)) for k, v in t.items()}
  new = lambda name, shape, dtype: _shifted(torch.zeros(shape, dtype=dtype, device=x.device), by(name, dtype))
  got = {}
  for name in outputs:
    got[name] = new(name, x.shape, x.dtype) if name in ('out', 'dx') else new(name, (units,), F32)
  if 'dscale' in outputs or 'dshift' in outputs:
    got['partials'] = new('partials', (_partial_floats(rows, units),), F32)
  for name, tensor in list(call.items()) + list(got.items()):
    assert tensor is None or (tensor.data_ptr() % 16 != 0) == (name in moved), name
  _norm_raw(call, impl, act, **got)
  return got


def _public_norm(t, impl, act, grads=(True, True, True)):
  """out and the gradients through nets.norm_act, and its (forward, backward) launches."""
  x = t['x'].detach().requires_grad_(grads[0])
  scale = t['scale'].detach().requires_grad_(grads[1])
  shift = None if t['shift'] is None else t['shift'].detach().requires_grad_(grads[2])
  assert x.data_ptr() == t['x'].data_ptr() and scale.data_ptr() == t['scale'].data_ptr()
  before = nets.norm_act_launches()
  out = nets.norm_act(x, scale, shift, impl, act, sweep.EPS, fused=True)
  forward = nets.norm_act_launches() - before
  out.backward(t['gout'])
  backward = nets.norm_act_launches() - before - forward
  got = {'out': out.detach(), 'dx': x.grad, 'dscale': scale.grad, 'dshift': None if shift is None else shift.grad}
  return got, (forward, backward)


# --- A ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('units', sweep.A_UNITS)
@DTYPES
def test_norm_act_views_off_16_bytes_give_the_bits_of_the_aligned_run(units, kind):
  impl, act = sweep.a_case(units, kind)
  inp = sweep.norm_inputs(sweep.A_ROWS, units, impl, kind)
  t = _norm_tensors(inp, kind)
  base = _run_norm(t, impl, act)
  ratios = sweep.norm_ratios(_hosts(base), sweep.norm_reference(inp, impl, act), inp, kind == 'bf16')
  print(f'{sweep.A_ROWS} x {units} {impl} {act} {kind}: aligned', {k: round(v, 4) for k, v in ratios.items()})
  assert max(ratios.values()) <= 1.0, ratios
  pointers = [name for name in sweep.NORM_POINTERS if t.get(name, True) is not None]      # rms has no shift
  runs = 0
  for step in _steps(kind):
    for moved in [(name,) for name in pointers] + [tuple(pointers)]:
      got = _run_norm(t, impl, act, moved, step)
      for key in base:
        assert _same(got[key], base[key]), (units, kind, impl, act, moved, step, key)
      runs += 1
  # nets.norm_act: x one element into its buffer, scale and shift slices at odd offsets of one flat buffer
  flat = torch.zeros(2 * units + 3, device='cuda')
  scale, shift = flat[1:1 + units], flat[units + 3:2 * units + 3]
  scale.copy_(t['scale'])
  if t['shift'] is not None:
    shift.copy_(t['shift'])
  views = dict(t, x=_shifted(t['x']), scale=scale, shift=None if t['shift'] is None else shift)
  assert all(v is None or v.data_ptr() % 16 for k, v in views.items() if k != 'gout')
  want, _ = _public_norm(t, impl, act)
  got, launches = _public_norm(views, impl, act)
  assert launches == (1, 2)
  for key in want:
    assert (want[key] is None and got[key] is None) or _same(got[key], want[key]), (units, kind, key)
    assert want[key] is None or _same(want[key], base[key]), (units, kind, key)
  print(f'{sweep.A_ROWS} x {units} {impl} {act} {kind}: {runs} runs from views off 16 bytes and nets.norm_act on such '
        'views, every output bit for bit the aligned run')


# --- B: gru_gate on device pointers ------------------------------------------------------------


def _gate_tensors(inp, kind):
  return {k: _dev(inp[k], kind) for k in ('x', 'deter', 'gout')}


def _gate_raw(t, blocks, out=None, dx=None, ddeter=None):
  x, d = t['x'], t['deter']
  rows, width = d.shape
  assert x.shape == (rows, 3 * width)
  stream = _lib.raw_stream(x.device)
  if out is not None:
    _lib.api.emb_gru_gate(x.data_ptr(), d.data_ptr(), CODES[x.dtype], rows, width, blocks, out.data_ptr(), stream)
  if dx is not None or ddeter is not None:
    _lib.api.emb_gru_gate_grad(x.data_ptr(), d.data_ptr(), t['gout'].data_ptr(), CODES[x.dtype], rows, width, blocks,
                               _addr(dx), _addr(ddeter), stream)


def _run_gate(t, blocks, moved=(), step='element', outputs=('out', 'dx', 'ddeter')):
  by = lambda name, dtype: _step(dtype, step) if name in moved else 0
  call = {k: _shifted(v, by(k, v.dtype)) for k, v in t.items()}
  got = {}
  for name in outputs:
    like = t['x'] if name == 'dx' else t['deter']
    got[name] = _shifted(torch.zeros_like(like), by(name, like.dtype))
  for name, tensor in list(call.items()) + list(got.items()):
    assert (tensor.data_ptr() % 16 != 0) == (name in moved), name
  _gate_raw(call, blocks, **got)
  return got


def _public_gate(t, blocks, grads=(True, True)):
  x, d = t['x'].detach().requires_grad_(grads[0]), t['deter'].detach().requires_grad_(grads[1])
  before = nets.gru_gate_launches()
  out = nets.gru_gate(x, d, blocks, fused=True)
  out.backward(t['gout'])
  return {'out': out.detach(), 'dx': x.grad, 'ddeter': d.grad}, nets.gru_gate_launches() - before


@pytest.mark.parametrize('deter,blocks', sweep.B_SHAPES)
@DTYPES
def test_gru_gate_views_off_16_bytes_give_the_bits_of_the_aligned_run(deter, blocks, kind):
  worst, runs = {}, 0
  for rows in sweep.B_ROWS:
    inp = sweep.gate_inputs(rows, deter, blocks, kind)
    t = _gate_tensors(inp, kind)
    base = _run_gate(t, blocks)
    want = gates.reference64(inp['x'], inp['deter'], blocks, inp['gout'])
    ratios = sweep.gate_ratios(_hosts(base), want, inp, kind == 'bf16')
    assert max(ratios.values()) <= 1.0, (rows, ratios)
    worst = {k: max(v, worst.get(k, 0.0)) for k, v in ratios.items()}
    for step in _steps(kind):
      for moved in [(name,) for name in sweep.GATE_POINTERS] + [sweep.GATE_POINTERS]:
        got = _run_gate(t, blocks, moved, step)
        for key in base:
          assert _same(got[key], base[key]), (rows, deter, blocks, kind, moved, step, key)
        runs += 1
    public, launches = _public_gate(dict(t, x=_shifted(t['x']), deter=_shifted(t['deter'])), blocks)
    assert launches == 2
    for key in base:
      assert _same(public[key], base[key]), (rows, key)
  print(f'{deter} / {blocks} {kind}: aligned', {k: round(v, 4) for k, v in worst.items()},
        f'and {runs} runs from views off 16 bytes, bit for bit the aligned run')


@DTYPES
def test_gru_gate_element_by_element_past_one_pass_of_the_grid(kind):
  """gates.STRIDED with x one element into its buffer: the per-element kernels over
  2.1 M items, 524 288 a pass.  tests/test_gpu_gru_gate.py holds the aligned run of
  this shape to the float64 restatement; here the bits must be the same."""
  rows, deter, blocks = sweep.B_STRIDED
  inp = gates.inputs_of(rows, deter, 1.0, np.random.default_rng([rows, deter, blocks]))
  t = _gate_tensors(inp, kind)
  base = _run_gate(t, blocks)
  got = _run_gate(t, blocks, ('x',))
  for key in base:
    assert _same(got[key], base[key]), key
  assert bool((base['out'] != 0).any()) and bool((base['dx'] != 0).any())


# --- C ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rows,units', sweep.C_SHAPES)
def test_norm_act_past_one_pass_of_the_grid(rows, units):
  impl, act = sweep.c_case(rows, units)
  for kind in sweep.c_kinds(rows, units):
    inp = sweep.norm_inputs(sweep.DISTINCT, units, impl, kind)
    want = sweep.norm_reference(inp, impl, act)
    t = _norm_tensors(inp, kind)
    small = _run_norm(t, impl, act)
    ratios = sweep.norm_ratios(_hosts(small), want, inp, kind == 'bf16', sums=want)
    assert max(ratios.values()) <= 1.0, (kind, ratios)
    index = torch.arange(rows, device='cuda') % sweep.DISTINCT
    tiled = dict(t, x=t['x'][index], gout=t['gout'][index])
    assert tiled['x'].shape == (rows, units) and tiled['x'].is_contiguous()
    big = _run_norm(tiled, impl, act)
    assert _same(big['out'], small['out'][index]), (kind, 'out')     # a row's out and dx are its own
    assert _same(big['dx'], small['dx'][index]), (kind, 'dx')
    sums = sweep.tiled_sums(inp, impl, act, rows)
    tall = {key: norms.sum_ratio(_host(big[key]), sums[key], sums[key + '_abs']) for key in ('dscale', 'dshift')}
    print(f'{rows} x {units} {impl} {act} {kind}: {sweep.DISTINCT} rows', {k: round(v, 4) for k, v in ratios.items()},
          f'{rows} rows', {k: round(v, 4) for k, v in tall.items()})
    assert max(tall.values()) <= 1.0, (kind, tall)
    again = _run_norm(tiled, impl, act, outputs=('dscale', 'dshift'))
    assert _same(again['dscale'], big['dscale']) and _same(again['dshift'], big['dshift']), kind      # run to run


# --- D ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rows,units', sweep.D_SHAPES)
@pytest.mark.parametrize('impl', norms.IMPLS)
def test_norm_act_null_outputs(rows, units, impl):
  for kind in sweep.KINDS:
    act = sweep.d_case(rows, units, impl, kind)
    inp = sweep.norm_inputs(rows, units, impl, kind)
    want = sweep.norm_reference(inp, impl, act)
    t = _norm_tensors(inp, kind)
    full = _run_norm(t, impl, act)
    ratios = sweep.norm_ratios(_hosts(full), want, inp, kind == 'bf16', sums=want)
    print(f'{rows} x {units} {impl} {act} {kind}: every output', {k: round(v, 4) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (kind, ratios)
    for outputs in (('dx',), ('dscale', 'dshift'), ('dscale',), ('dshift',)):
      got = _run_norm(t, impl, act, outputs=outputs)
      assert ('partials' in got) == (outputs != ('dx',))            # dx alone: partials is null
      for key in outputs:
        assert _same(got[key], full[key]), (kind, outputs, key)
    # nets.norm_act: no gradient for x; then for scale alone
    every, launches = _public_norm(t, impl, act)
    assert launches == (1, 2)
    for grads in ((False, True, True), (False, True, False)):
      got, launches = _public_norm(t, impl, act, grads)
      assert launches == (1, 2), (grads, launches)                   # one forward; the sums and their sum
      assert got['dx'] is None and _same(got['out'], full['out']) and _same(got['dscale'], full['dscale']), grads
      assert _same(got['dscale'], every['dscale'])
      if impl == 'layer' and grads[2]:
        assert _same(got['dshift'], full['dshift']) and _same(got['dshift'], every['dshift'])
      else:
        assert got['dshift'] is None


@pytest.mark.parametrize('deter,blocks', sweep.D_GATE_SHAPES)
@DTYPES
def test_gru_gate_null_outputs(deter, blocks, kind):
  inp = sweep.gate_inputs(sweep.D_GATE_ROWS, deter, blocks, kind)
  t = _gate_tensors(inp, kind)
  full = _run_gate(t, blocks)
  ratios = sweep.gate_ratios(_hosts(full), gates.reference64(inp['x'], inp['deter'], blocks, inp['gout']), inp, kind == 'bf16')
  print(f'{sweep.D_GATE_ROWS} x {deter} / {blocks} {kind}: both gradients', {k: round(v, 4) for k, v in ratios.items()})
  assert max(ratios.values()) <= 1.0, ratios
  for only in ('dx', 'ddeter'):
    got = _run_gate(t, blocks, outputs=(only,))
    assert _same(got[only], full[only]), only
  for grads, only, other in (((True, False), 'dx', 'ddeter'), ((False, True), 'ddeter', 'dx')):
    got, launches = _public_gate(t, blocks, grads)
    assert launches == 2 and got[other] is None
    assert _same(got[only], full[only]) and _same(got['out'], full['out']), grads


# --- E ----------------------------------------------------------------------------------------------


def _banded(shape, dtype, start):
  """A buffer filled with 7 and the view of `shape` that starts `start` elements into it."""
  n = int(np.prod(shape))
  buf = torch.full((start + n + sweep.E_MARGIN + 5,), sweep.FILL, dtype=dtype, device='cuda')
  assert buf.data_ptr() % 16 == 0 and start >= sweep.E_MARGIN
  return buf, buf[start:start + n].view(shape), start, n


def _check_bands(bands, plain, tag):
  for name, (buf, view, start, n) in bands.items():
    assert bool((buf[:start] == sweep.FILL).all()) and bool((buf[start + n:] == sweep.FILL).all()), (tag, name, 'margin')
    assert bool((view != sweep.FILL).all()), (tag, name, 'not all written')
    assert _same(view, plain[name]), (tag, name)


@pytest.mark.parametrize('units', sweep.E_UNITS + sweep.E_UNITS_VEC)
@DTYPES
def test_norm_act_writes_its_outputs_and_nothing_else(units, kind):
  impl, act = sweep.e_case(units)
  rows = sweep.E_ROWS
  inp = sweep.norm_inputs(rows, units, impl, kind)
  t = _norm_tensors(inp, kind)
  kept = _clones(t)
  plain = _run_norm(t, impl, act)
  ratios = sweep.norm_ratios(_hosts(plain), sweep.norm_reference(inp, impl, act), inp, kind == 'bf16')
  assert max(ratios.values()) <= 1.0, ratios
  for name, tensor in plain.items():
    assert bool((tensor != sweep.FILL).all()), name                  # 7 is no value of these outputs
  floats = _partial_floats(rows, units)
  for start in sweep.E_STARTS:
    bands = {'out': _banded((rows, units), TORCH[kind], start), 'dx': _banded((rows, units), TORCH[kind], start),
             'dscale': _banded((units,), F32, start), 'dshift': _banded((units,), F32, start),
             'partials': _banded((floats,), F32, start)}
    on16 = start == sweep.E_STARTS[0]
    assert all((band[1].data_ptr() % 16 == 0) == on16 for band in bands.values())
    _norm_raw(t, impl, act, floats=floats, **{name: band[1] for name, band in bands.items()})
    _check_bands(bands, plain, (units, kind, start))
    assert _unchanged(t, kept), (units, kind, start)
  print(f'{rows} x {units} {impl} {act} {kind}:', {k: round(v, 4) for k, v in ratios.items()},
        'out, dx, dscale, dshift and partials written whole, 16 elements around each and the inputs untouched')


@pytest.mark.parametrize('deter,blocks', sweep.B_SHAPES)
@DTYPES
def test_gru_gate_writes_its_outputs_and_nothing_else(deter, blocks, kind):
  rows = sweep.E_ROWS
  inp = sweep.gate_inputs(rows, deter, blocks, kind)
  t = _gate_tensors(inp, kind)
  kept = _clones(t)
  plain = _run_gate(t, blocks)
  ratios = sweep.gate_ratios(_hosts(plain), gates.reference64(inp['x'], inp['deter'], blocks, inp['gout']), inp, kind == 'bf16')
  assert max(ratios.values()) <= 1.0, ratios
  for name, tensor in plain.items():
    assert bool((tensor != sweep.FILL).all()), name
  for start in sweep.E_STARTS:
    bands = {'out': _banded((rows, deter), TORCH[kind], start), 'dx': _banded((rows, 3 * deter), TORCH[kind], start),
             'ddeter': _banded((rows, deter), TORCH[kind], start)}
    on16 = start == sweep.E_STARTS[0]
    assert all((band[1].data_ptr() % 16 == 0) == on16 for band in bands.values())
    _gate_raw(t, blocks, **{name: band[1] for name, band in bands.items()})
    _check_bands(bands, plain, (deter, blocks, kind, start))
    assert _unchanged(t, kept), (deter, blocks, kind, start)
  print(f'{rows} x {deter} / {blocks} {kind}:', {k: round(v, 4) for k, v in ratios.items()},
        'out, dx and ddeter written whole, 16 elements around each and the inputs untouched')
