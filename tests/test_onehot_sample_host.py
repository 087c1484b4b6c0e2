"""The restatements of tests/onehot_sample_cases.py, held against what they stand
for -- no GPU: the numpy Philox against the Random123 known answers, the float64
restatement against the reference's own run (tests/golden/onehot_sample.npz), its
autograd against the closed form and central differences, the float32 definition
against the acceptance rule and the gradient bar the GPU tests hold the kernels
to, and the statistical test's seeds under the numpy stream."""
import pathlib

import numpy as np
import pytest

from embodied_amd.outs import onehot_sample_launches, philox_uniform  # noqa: F401  (every test here fails without the feature)
from tests import onehot_sample_cases as cases

GOLDEN = pathlib.Path(__file__).parent / 'golden' / 'onehot_sample.npz'


@pytest.fixture(scope='module')
def golden():
  with np.load(GOLDEN) as f:
    return {k: f[k] for k in f.files}


def test_philox_known_answers():
  for counter, key, want in cases.KNOWN_ANSWERS:
    got = cases.philox4x32(counter, key)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
  # vectorised: the same words, element by element
  counters = [np.array([a[0][i] for a in cases.KNOWN_ANSWERS], np.uint32) for i in range(4)]
  keys = [np.array([a[1][i] for a in cases.KNOWN_ANSWERS], np.uint32) for i in range(2)]
  got = cases.philox4x32(counters, keys)
  assert [tuple(int(w[i]) for w in got) for i in range(3)] == [a[2] for a in cases.KNOWN_ANSWERS]


def test_uniforms_are_the_documented_words():
  """u = (word 0 >> 8) * 2^-24 at counter (g, offset) under key seed, 64-bit each."""
  seed, offset, first = 0xa4093822299f31d0, 0x0370734413198a2e, 0x85a308d3243f6a88
  # counter (243f6a88, 85a308d3, 13198a2e, 03707344), key (299f31d0, a4093822): the third known answer's
  # counter with the key halves in the documented order
  word = cases.philox4x32((first & 0xffffffff, first >> 32, offset & 0xffffffff, offset >> 32),
                          (seed & 0xffffffff, seed >> 32))[0]
  u = cases.uniforms(seed, offset, first, 3)
  assert u.dtype == np.float32 and u[0] == np.float32((int(word) >> 8) * 2.0 ** -24)
  assert ((u >= 0) & (u < 1)).all()
  swapped = 0x299f31d0a4093822                                       # key (a4093822, 299f31d0): the known answer itself
  assert cases.uniforms(swapped, offset, first, 1)[0] == np.float32((0xd16cfe09 >> 8) * 2.0 ** -24)
  many = cases.uniforms(5, 0, 2 ** 32 - 2, 4)                        # g crosses 2^32: the high word counts
  assert len(set(many.tolist())) == 4
  assert many[2] == cases.uniforms(5, 0, 2 ** 32, 1)[0] != cases.uniforms(5, 0, 0, 1)[0]


def test_restatement_equals_the_reference_run(golden):
  """probs, argmax (ties first) and the straight-through value of every case."""
  ties = 0
  for case, c in enumerate(cases.CASES):
    name = cases.tag(case)
    inp = cases.inputs(case)
    assert np.array_equal(golden[f'in_{name}'], cases.digest(inp)), name
    got = cases.restate(inp['logits'], c.unimix, inp['index'])
    assert np.allclose(got['probs'], golden[f'probs_{name}'], rtol=1e-13, atol=1e-300), name
    assert np.array_equal(got['argmax'], golden[f'argmax_{name}']), name
    assert np.array_equal(got['value'], golden[f'value_{name}']), name
    assert np.allclose(cases.probs64(inp['logits'], c.unimix), golden[f'probs_{name}'], rtol=1e-12, atol=1e-300), name
    if c.classes >= 3:                                             # the planted tie: the first of the two
      assert golden[f'argmax_{name}'].reshape(-1)[0] == 1, name
      ties += 1
  assert ties > 50


def test_autograd_is_the_closed_form_and_central_differences():
  rng = np.random.default_rng(3)
  for groups, classes in ((3, 5), (0, 64), (3, 96)):
    for unimix in cases.UNIMIX:
      x = cases.logits_of(2, groups, classes, 1.0, rng)
      g = cases.gout_of(x.shape, rng)
      index = rng.integers(0, classes, x.shape[:-1])
      auto = cases.restate(x, unimix, index, g)['grad']
      closed = cases.closed_form64(x, unimix, g)
      assert np.abs(auto - closed).max() <= 1e-13 * np.abs(g).max(), (groups, classes, unimix)
      # central differences of sum(value * g): only probs moves with x
      f = lambda x64: (cases.probs64(x64, unimix) * g).sum()
      x64, h = x.astype(np.float64), 1e-6
      flat = x64.reshape(-1)
      for at in rng.integers(0, flat.size, 12):
        up, down = flat.copy(), flat.copy()
        up[at] += h
        down[at] -= h
        numeric = (f(up.reshape(x.shape)) - f(down.reshape(x.shape))) / (2 * h)
        assert abs(numeric - auto.reshape(-1)[at]) <= 1e-8 * max(1.0, np.abs(g).max()), (groups, classes, unimix, at)


def _draws(rng, count):
  """Uniforms of the stream's grid, with 0 and 1 - 2^-24 among them."""
  u = (rng.integers(0, 2 ** 24, count).astype(np.float64) * 2.0 ** -24).astype(np.float32)
  u.reshape(-1)[:2] = [0.0, 1 - 2.0 ** -24][:u.size]
  return u


def test_float32_definition_stays_inside_the_acceptance_rule():
  """Every shape, row count, scale and unimix, float32 and bfloat16-rounded
  logits: the float32 definition's index is accepted, few draws are near a
  boundary, and its gradient is inside the bar (printed)."""
  worst_cdf, worst_grad, near_count, total = 0.0, 0.0, 0, 0
  for groups, classes in cases.SHAPES:
    tol = cases.tol_of(classes)
    for rows in cases.ROWS:
      for scale in cases.SCALES:
        for unimix in cases.UNIMIX:
          for kind in ('f32', 'bf16'):
            rng = np.random.default_rng([groups, classes, rows, int(scale * 10), int(unimix * 100), kind == 'bf16'])
            x = cases.logits_of(rows, groups, classes, scale, rng)
            if kind == 'bf16':
              x = cases.bf16_round(x)
            u = _draws(rng, x.shape[:-1]).reshape(x.shape[:-1])
            g = cases.gout_of(x.shape, rng)
            got = cases.define32(x, unimix, u, g)
            p64 = cases.probs64(x, unimix)
            ok, near = cases.accepted(p64, u, got['index'], tol)
            assert ok.all(), (groups, classes, rows, scale, unimix, kind)
            assert (np.take_along_axis(got['probs'], got['index'][..., None], -1) > 0).all()
            near_count, total = near_count + int(near.sum()), total + near.size
            cdf32 = got['cdf'] / got['cdf'][..., -1:]
            worst_cdf = max(worst_cdf, float(np.abs(cdf32 - cases.cdf64(p64)).max()) / tol)
            want = cases.restate(x, unimix, got['index'], g)['grad']
            ratio = cases.grad_ratio(got['grad'], want, cases.group_scale(g, unimix))
            if cases.grad_held(unimix, scale):
              assert ratio <= 1.0, (groups, classes, rows, scale, unimix, kind, ratio)
            worst_grad = max(worst_grad, ratio)
  print(f'float32 definition: CDF off by {worst_cdf:.3g} of tol at the worst, {near_count} of {total} draws '
        f'({near_count / total:.2%}) within tol of a boundary, gradient {worst_grad:.3g} of its bar')
  assert worst_cdf <= 1.0 and near_count / total < 0.05
  assert not cases.GRAD_EXEMPT, 'the float32 definition holds the gradient bar everywhere: none is exempt'


def test_exact_boundaries_and_zero_probability_classes():
  """u exactly on a float32 CDF boundary takes the class above it; a class whose
  probability is exactly 0 is never returned, at the ends either."""
  x = np.array([[0.0, -np.inf, 0.0, 0.0, -np.inf]], np.float32)    # p = 1/3, 0, 1/3, 1/3, 0
  d = cases.define32(x, 0.0)
  for u, want in ((0.0, 0), (float(d['cdf'][0, 0] / d['cdf'][0, -1]), 2), (1 - 2.0 ** -24, 3)):
    got = cases.define32(x, 0.0, np.array([u], np.float32))['index'][0]
    assert got == want, (u, got)
    assert cases.select64(cases.probs64(x, 0.0), np.array([u]))[0] in (want, max(want - 2, 0))
  x = np.array([[-np.inf, 2.0, 1.0]], np.float32)
  assert cases.define32(x, 0.0, np.array([0.0], np.float32))['index'][0] == 1
  ok, near = cases.accepted(cases.probs64(x, 0.0), np.array([0.0]), np.array([0]), cases.tol_of(3))
  assert not ok[0]                                                 # a class of probability 0 is refused by the rule


@pytest.mark.parametrize('classes', cases.STAT_CLASSES)
@pytest.mark.parametrize('unimix', cases.UNIMIX)
def test_the_statistical_seeds_pass_under_the_restatement(classes, unimix):
  x = np.broadcast_to(cases.stat_logits(classes), (cases.STAT_GROUPS, classes))
  u = cases.uniforms(cases.STAT_SEEDS[classes], cases.STAT_OFFSET, 0, cases.STAT_GROUPS)
  index = cases.define32(x, unimix, u)['index']
  stat, dof = cases.chi_square(np.bincount(index, minlength=classes), cases.probs64(x[0], unimix))
  bound = cases.chi_square_bound(dof)
  print(f'{classes} classes, unimix {unimix}: chi-square {stat:.1f} on {dof} degrees of freedom, bound {bound:.1f}')
  assert dof >= 3 and stat < bound
  # and a wrong sampler does not: the same draws against the distribution shifted by one class
  wrong, _ = cases.chi_square(np.bincount(index, minlength=classes), np.roll(cases.probs64(x[0], unimix), 1))
  assert wrong > bound
