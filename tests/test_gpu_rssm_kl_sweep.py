"""Every instantiation of `onehot_kl_kernel<T, W, NPER>` and
`onehot_kl_grad_kernel<T, W, NPER>` (csrc/onehot_kl.hip): the eight rungs of
EMB_ONEHOT_BY_WIDTH, float32 and bfloat16, forward and gradient, at the shapes
tests/rssm_kl_sweep_cases.py derives from the kernels' constants -- per rung its
first and last class count and the boundaries of the NPER slots, stoch 1, kSegs,
kSegs + 1 (a second iteration of the g0 loop with one live segment) and
2 kSegs + 1, rows 1 and 5, and every size the reference ships at stoch 32.

Per rung: (a) parity with `tests.rssm_kl_cases.reference64` at the bars of
tests/test_gpu_rssm_kl.py (forward 1e-5 + 1e-5 |want|; gradient
1e-5 |g| (1 + |want|), bfloat16 plus 2^-8 |want|), the composed path as the
control; (b) a row run alone has the bits it has among its neighbours; (c) the
bfloat16 instantiation has the bits of the float32 one on the same values;
(d) the kl of a distribution with itself is 0 and `OneHot.entropy()` has the
bits of the pair's entropies; (e) through the C ABI, with every output inside a
sentinel-filled allocation at an odd offset, nothing outside the outputs is
written.  tests/test_rssm_kl_sweep_host.py shows without a GPU that the float32
definition sits inside both bars at every input used here and that no row's kl
is within 1e-4 of free_nats.  Need a GPU."""
import numpy as np
import pytest
import torch

from embodied_amd.outs import OneHot, rssm_kl
from embodied_amd import _lib
from tests import rssm_kl_cases as cases
from tests import rssm_kl_sweep_cases as sweep

pytestmark = pytest.mark.gpu
RUNGS = pytest.mark.parametrize('rung', sweep.RUNGS, ids=[f'W{W}x{nper}' for W, nper in sweep.RUNGS])
OUTPUTS = ('dyn', 'rep', 'dyn_ent', 'rep_ent')
GRADS = ('grad_post', 'grad_prior')
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
SENTINEL = -1234.5          # exact in bfloat16
GAP = 321                   # elements of sentinel around a gradient: more than the 256 a wave spans per iteration


@pytest.fixture(scope='module', autouse=True)
def gpu():
  assert torch.cuda.is_available(), 'these tests need the MI355X'
  torch.cuda.set_device(0)


def _host(t):
  return t.detach().float().cpu().numpy()


def _bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_DEVICE = {}


def _device(stoch, classes, rows, scale, kind, held=None):
  """`sweep.data` on the device, uploaded once: post and prior in the dtype of
  `kind` (or `held`: bfloat16-rounded values in float32 tensors), g_dyn and
  g_rep in float32."""
  key = (stoch, classes, rows, scale, kind, held)
  if key not in _DEVICE:
    d = sweep.data(stoch, classes, rows, scale, kind)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}
    for k in ('post', 'prior'):
      t[k] = t[k].to(DTYPES[held or kind])      # exact: the values of kind 'bf16' are bfloat16 numbers
      assert np.array_equal(_host(t[k]), d[k])
    _DEVICE[key] = t
  return _DEVICE[key]


def _run(t, unimix, free, fused, row=None):
  """`rssm_kl` with backward over the device inputs `t` (or over a copy of their
  row `row` alone): the four outputs and both gradients, on the device."""
  pick = (lambda x: x) if row is None else (lambda x: x[row:row + 1].clone())
  post, prior = pick(t['post']).detach().requires_grad_(), pick(t['prior']).detach().requires_grad_()
  out = rssm_kl(post, prior, unimix=unimix, free_nats=free, fused=fused)
  (out['dyn'] * pick(t['g_dyn']) + out['rep'] * pick(t['g_rep'])).sum().backward()
  got = {k: out[k].detach() for k in OUTPUTS}
  assert all(v.dtype == torch.float32 and v.shape == post.shape[:1] for v in got.values())
  assert post.grad.dtype == post.dtype and post.grad.shape == post.shape and prior.grad.shape == prior.shape
  got.update(grad_post=post.grad, grad_prior=prior.grad)
  return got


_FUSED = {}


def _fused(stoch, classes, rows, scale, kind, unimix, free):
  """The kernels' run of one sweep input through the facade, made once: what
  (a) holds against float64 and (b), (c) and (e) compare bits with."""
  key = (stoch, classes, rows, scale, kind, unimix, free)
  if key not in _FUSED:
    _FUSED[key] = _run(_device(stoch, classes, rows, scale, kind), unimix, free, True)
  return _FUSED[key]


def _settings():
  return [(unimix, scale, free) for unimix, scale in sweep.SETTINGS for free in sweep.FREE_NATS]


def _ratios(got, ref, d, kind):
  """(forward, gradient) of a run as shares of their bars."""
  forward = max(cases.forward_ratio(_host(got['dyn']), ref['dyn']), cases.forward_ratio(_host(got['rep']), ref['rep']),
                cases.forward_ratio(_host(got['dyn_ent']), ref['ent_prior']),
                cases.forward_ratio(_host(got['rep_ent']), ref['ent_post']))
  grad = max(cases.grad_ratio(_host(got['grad_post']), ref['grad_post'], d['g_rep'], kind == 'bf16'),
             cases.grad_ratio(_host(got['grad_prior']), ref['grad_prior'], d['g_dyn'], kind == 'bf16'))
  return forward, grad


def _title(rung):
  return f'W = {rung[0]}, NPER = {rung[1]} (kSegs {sweep.segments(rung)})'


@RUNGS
def test_parity_at_every_shape_of_the_rung(rung):
  """(a) Every shape of the rung, rows 1 and 5, both dtypes, unimix 0.01 (scales
  1 and 5) and 0 (scales 0.1 and 1), free_nats 1 and 0: the four outputs and both
  gradients of the kernels against float64; the composed path at stoch kSegs + 1
  of every class count as the control."""
  worst, control, controls = [0.0, 0.0], [0.0, 0.0], []
  for stoch, classes in sweep.shapes(rung):
    assert sweep.width(classes) == rung
    composed = stoch == sweep.control_stoch(classes)
    controls += [f'{stoch}x{classes}'] if composed else []
    for rows in sweep.ROWS:
      for kind in sweep.KINDS:
        for unimix, scale, free in _settings():
          d = sweep.data(stoch, classes, rows, scale, kind)
          ref = cases.reference64(d['post'], d['prior'], unimix, free, d['g_dyn'], d['g_rep'])
          ratios = _ratios(_fused(stoch, classes, rows, scale, kind, unimix, free), ref, d, kind)
          assert max(ratios) <= 1.0, ('fused', stoch, classes, rows, kind, unimix, scale, free, ratios)
          worst = [max(a, b) for a, b in zip(worst, ratios)]
          if composed:
            ratios = _ratios(_run(_device(stoch, classes, rows, scale, kind), unimix, free, False), ref, d, kind)
            assert max(ratios) <= 1.0, ('composed', stoch, classes, rows, kind, unimix, scale, free, ratios)
            control = [max(a, b) for a, b in zip(control, ratios)]
  print(f'{_title(rung)}: ' + ' '.join(f'{s}x{c}' for s, c in sweep.shapes(rung)) + f', rows {sweep.ROWS}: fused forward '
        f'{worst[0]:.3g}, gradient {worst[1]:.3g} of their bars; composed at ' + ' '.join(controls) +
        f': forward {control[0]:.3g}, gradient {control[1]:.3g}')


@RUNGS
def test_a_row_alone_has_the_bits_it_has_among_its_neighbours(rung):
  """(b) Every shape of the rung at rows = 5, every dtype and setting: each row
  run alone (rows = 1, its own allocation) gives the bits of that row in all four
  outputs and both gradients -- what another row or another segment leaked into a
  row would change, inside the tolerance or not."""
  rows = sweep.ROWS[-1]
  for stoch, classes in sweep.shapes(rung):
    for kind in sweep.KINDS:
      for unimix, scale, free in _settings():
        together = _fused(stoch, classes, rows, scale, kind, unimix, free)
        t = _device(stoch, classes, rows, scale, kind)
        alone = [_run(t, unimix, free, True, row) for row in range(rows)]
        for key in OUTPUTS + GRADS:
          assert _same_bits(torch.cat([a[key] for a in alone]), together[key]), (
              key, stoch, classes, kind, unimix, scale, free)


@RUNGS
def test_bfloat16_instantiation_has_the_bits_of_the_float32_one(rung):
  """(c) The two instantiations differ in `load` and `store` alone (the same
  templates, fp contract off, no fast-math flag in the build): the float32
  kernels over the bfloat16 inputs' values held in float32 tensors give the
  forward outputs of the bfloat16 run bit for bit, and gradients whose rounding
  to bfloat16 has the bits of the bfloat16 gradients.  Finite inputs."""
  for stoch, classes in sweep.shapes(rung):
    for rows in sweep.ROWS:
      for unimix, scale, free in _settings():
        narrow = _fused(stoch, classes, rows, scale, 'bf16', unimix, free)
        wide = _run(_device(stoch, classes, rows, scale, 'bf16', held='f32'), unimix, free, True)
        where = (stoch, classes, rows, unimix, scale, free)
        for key in OUTPUTS:
          assert _same_bits(wide[key], narrow[key]), (key, *where)
        for key in GRADS:
          assert wide[key].dtype == torch.float32 and narrow[key].dtype == torch.bfloat16
          assert torch.isfinite(wide[key]).all(), (key, *where)
          assert _same_bits(wide[key].to(torch.bfloat16), narrow[key]), (key, *where)


@RUNGS
def test_self_kl_is_zero_and_entropy_has_the_bits_of_the_pair(rung):
  """(d) At stoch kSegs + 1 of every class count, rows 5, both dtypes:
  `OneHot(x).kl(OneHot(x))` is 0 in every row (both sides run `side()` on the
  same bits), and `OneHot.entropy()` has the bits of rep_ent and dyn_ent of
  `rssm_kl(x, x)` and of the side it is in `rssm_kl(post, prior)`."""
  rows = sweep.ROWS[-1]
  for classes in sweep.CLASSES[rung]:
    stoch = sweep.control_stoch(classes)
    for kind in sweep.KINDS:
      for unimix, scale in sweep.SETTINGS:
        t = _device(stoch, classes, rows, scale, kind)
        where = (stoch, classes, kind, unimix, scale)
        pair = _fused(stoch, classes, rows, scale, kind, unimix, 0.0)
        for x, own in ((t['post'], 'rep_ent'), (t['prior'], 'dyn_ent')):
          dist = OneHot(x, unimix, fused=True)
          assert dist.fused is True
          kl = dist.kl(OneHot(x, unimix, fused=True))
          assert kl.shape == (rows,) and kl.dtype == torch.float32 and (kl == 0).all(), (*where, own, kl)
          entropy = dist.entropy()
          assert torch.isfinite(entropy).all() and (classes == 1 or (entropy > 0).all()), (*where, own, entropy)
          both = rssm_kl(x, x, unimix=unimix, free_nats=0.0, fused=True)
          assert (both['dyn'] == 0).all() and (both['rep'] == 0).all(), (*where, own)
          assert _same_bits(entropy, both['rep_ent']) and _same_bits(entropy, both['dyn_ent']), (*where, own)
          assert _same_bits(entropy, pair[own]), (*where, own)


def _odd(at):
  return at | 1


@RUNGS
def test_nothing_is_written_outside_the_outputs(rung):
  """(e) `emb_onehot_kl` and `emb_onehot_kl_grad` through the C ABI at stoch
  kSegs + 1, rows 5 -- the last row's last iteration has dead segments, and
  padding lanes wherever classes < W NPER -- with each of the five forward
  outputs and both gradients at an odd element offset inside an allocation
  filled with a sentinel: afterwards everything outside the outputs is the
  sentinel, and the outputs have the bits of the facade's run."""
  rows = sweep.ROWS[-1]
  for classes in sweep.CLASSES[rung]:
    stoch = sweep.control_stoch(classes)
    n = rows * stoch * classes
    for kind in sweep.KINDS:
      for unimix, scale, free in _settings():
        t = _device(stoch, classes, rows, scale, kind)
        where = (stoch, classes, kind, unimix, scale, free)
        want = _fused(stoch, classes, rows, scale, kind, unimix, free)
        raw = _fused(stoch, classes, rows, scale, kind, unimix, 0.0)['dyn']      # no maximum: the kl itself
        small = torch.full((5 * (rows + 4) + 3,), SENTINEL, device='cuda')
        starts = [_odd(i * (rows + 4)) for i in range(5)]
        kl, ent_post, ent_prior, dyn, rep = (small[at:at + rows] for at in starts)
        large = torch.full((2 * n + 3 * GAP + 1,), SENTINEL, dtype=DTYPES[kind], device='cuda')
        spots = [_odd(GAP), _odd(GAP + n + GAP)]
        grad_post, grad_prior = (large[at:at + n] for at in spots)
        for view in (kl, ent_post, ent_prior, dyn, rep, grad_post, grad_prior):
          assert (view.data_ptr() // view.element_size()) % 2 == 1 and (view == SENTINEL).all()
        dtype = _lib.F32 if kind == 'f32' else _lib.BF16
        stream = _lib.raw_stream(small.device)
        _lib.api.emb_onehot_kl(t['post'].data_ptr(), t['prior'].data_ptr(), dtype, rows, stoch, classes, unimix, free,
                               kl.data_ptr(), ent_post.data_ptr(), ent_prior.data_ptr(), dyn.data_ptr(), rep.data_ptr(),
                               stream)
        _lib.api.emb_onehot_kl_grad(t['post'].data_ptr(), t['prior'].data_ptr(), dtype, rows, stoch, classes, unimix,
                                    free, kl.data_ptr(), t['g_rep'].data_ptr(), t['g_dyn'].data_ptr(),
                                    grad_post.data_ptr(), grad_prior.data_ptr(), stream)
        inside = torch.zeros_like(small, dtype=torch.bool)
        for at in starts:
          inside[at:at + rows] = True
        assert (small[~inside] == SENTINEL).all() and int((~inside).sum()) == small.numel() - 5 * rows, where
        inside = torch.zeros_like(large, dtype=torch.bool)
        for at in spots:
          inside[at:at + n] = True
        assert (large[~inside] == SENTINEL).all() and int((~inside).sum()) == large.numel() - 2 * n, where
        assert not (small[torch.cat([torch.arange(at, at + rows) for at in starts]).cuda()] == SENTINEL).any(), where
        for got, key in ((kl, None), (dyn, 'dyn'), (rep, 'rep'), (ent_prior, 'dyn_ent'), (ent_post, 'rep_ent'),
                         (grad_post.view(rows, stoch, classes), 'grad_post'),
                         (grad_prior.view(rows, stoch, classes), 'grad_prior')):
          assert _same_bits(got, raw if key is None else want[key]), (key or 'kl', *where)
