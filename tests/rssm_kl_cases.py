"""Seeded inputs of the RSSM KL fixture (tests/golden/rssm_kl.npz) and a torch
restatement of `RSSM.loss`'s KL block for the shapes the fixture does not hold.

Shared by `tools/gen_rssm_kl_golden.py` (which feeds the inputs to the
reference's own `RSSM.loss`, `RSSM._dist` and output classes) and by the tests
(which regenerate them and check the digests stored in the fixture).
`reference64` is this project's own torch-CPU code in float64; its autograd is
the gradient oracle.  The host test holds its forward against the fixture's
float64 values on every case, and only then do the GPU tests use it for other
shapes, for bfloat16-rounded inputs and for the gradients.
"""
import collections

import numpy as np
import torch

from tests.scan_cases import digest  # noqa: F401  (same digest as the scan fixtures)
from tests.twohot_cases import bf16_round  # noqa: F401

f32 = np.float32

# (stoch, classes): one group of two, fewer classes than a segment (5, 24), the
# shipped 32 x 32 and 32 x 64, 2 and 4 values per lane (96, 256), and one past
# what the kernels take (257: the composed path only)
SHAPES = ((1, 2), (2, 4), (3, 5), (32, 24), (32, 32), (32, 64), (5, 96), (2, 256), (2, 257))
FUSED_SHAPES = SHAPES[:-1]
SCALES = (0.1, 1.0, 5.0, 30.0, 1e4)
UNIMIX = (0.01, 0.0)
FREE_NATS = (1.0, 0.0)
ROWS = 37
FIELDS = ('kl', 'dyn_f1', 'ent_post', 'ent_prior')     # the rows of a case's array in the fixture
# unimix = 0 multiplies the post gradient by log p - log q of order 1e2 .. 1e5 at
# scales >= 5 and the float32 definition itself misses the gradient bar there:
# gradients of unimix = 0 are held to the bar at these scales only
GRAD_SCALES_NO_UNIMIX = (0.1, 1.0)

Case = collections.namedtuple('Case', 'stoch classes scale unimix')
CASES = tuple(Case(s, c, scale, u) for s, c in SHAPES for scale in SCALES for u in UNIMIX)


def tag(case):
  c = CASES[case]
  return f'c{case}_{c.stoch}x{c.classes}_s{c.scale:g}_u{c.unimix:g}'


def logits_of(rows, stoch, classes, scale, rng):
  """post, prior (rows, stoch, classes) float32: scale * N(0, 1); every fifth row's
  prior is its post plus a twentieth of that noise, a row whose kl is small (below
  free_nats = 1 at every scale but 1e4)."""
  post = (scale * rng.standard_normal((rows, stoch, classes))).astype(f32)
  prior = (scale * rng.standard_normal((rows, stoch, classes))).astype(f32)
  near = np.arange(rows) % 5 == 0
  prior[near] = (post[near] + min(scale, 1.0) * 0.05 * rng.standard_normal((int(near.sum()), stoch, classes))).astype(f32)
  return post, prior


def inputs(case):
  c = CASES[case]
  rng = np.random.default_rng([case, c.stoch, c.classes])
  post, prior = logits_of(ROWS, c.stoch, c.classes, c.scale, rng)
  return {'post': post, 'prior': prior}


def _dist(logits, unimix):
  """outs.py:210-217."""
  if unimix:
    probs = torch.softmax(logits, -1)
    uniform = torch.ones_like(probs) / probs.shape[-1]
    probs = (1 - unimix) * probs + unimix * uniform
    logits = torch.log(probs)
  return logits


def _kl(logits, other):
  """outs.py:236-240, summed over the groups (outs.py:73-76)."""
  logprob = torch.log_softmax(logits, -1)
  logother = torch.log_softmax(other, -1)
  prob = torch.softmax(logits, -1)
  return (prob * (logprob - logother)).sum(-1).sum(-1)


def _entropy(logits):
  """outs.py:230-234, summed over the groups (outs.py:69-71)."""
  logprob = torch.log_softmax(logits, -1)
  prob = torch.softmax(logits, -1)
  return (-(prob * logprob).sum(-1)).sum(-1)


def restate(post, prior, unimix, free_nats, g_dyn=None, g_rep=None, dtype=torch.float64):
  """rssm.py:123-132 on torch CPU in `dtype` over float32 (or bfloat16-rounded)
  values (..., stoch, classes): dict of numpy arrays kl (raw), dyn, rep, ent_post,
  ent_prior and, with upstream gradients g_dyn, g_rep (...), grad_post and
  grad_prior of sum(dyn * g_dyn + rep * g_rep) by autograd."""
  post = torch.from_numpy(np.ascontiguousarray(post)).to(dtype).requires_grad_()
  prior = torch.from_numpy(np.ascontiguousarray(prior)).to(dtype).requires_grad_()
  dyn = _kl(_dist(post.detach(), unimix), _dist(prior, unimix))
  rep = _kl(_dist(post, unimix), _dist(prior.detach(), unimix))
  out = {'kl': dyn.detach().clone()}
  if free_nats:
    floor = torch.tensor(free_nats, dtype=dtype)
    dyn, rep = torch.maximum(dyn, floor), torch.maximum(rep, floor)
  with torch.no_grad():
    out.update(dyn=dyn.detach(), rep=rep.detach(), ent_post=_entropy(_dist(post, unimix)),
               ent_prior=_entropy(_dist(prior, unimix)))
  if g_dyn is not None:
    g_dyn = torch.from_numpy(np.ascontiguousarray(g_dyn)).to(dtype)
    g_rep = torch.from_numpy(np.ascontiguousarray(g_rep)).to(dtype)
    (dyn * g_dyn + rep * g_rep).sum().backward()
    out.update(grad_post=post.grad, grad_prior=prior.grad)
  return {k: v.numpy() for k, v in out.items()}


def reference64(post, prior, unimix, free_nats, g_dyn=None, g_rep=None):
  return restate(post, prior, unimix, free_nats, g_dyn, g_rep, torch.float64)


def forward_ratio(got, want):
  """Worst |got - want| / (1e-5 + 1e-5 |want|); NaN and +-inf where and only where `want` has them."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.array_equal(np.isnan(got), np.isnan(want)), (np.isnan(got).sum(), np.isnan(want).sum())
  ok = np.isfinite(want)
  assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)])
  return float(np.max(np.abs(got - want)[ok] / (1e-5 + 1e-5 * np.abs(want[ok])), initial=0.0))


BF16_GRAD = 2.0 ** -8     # a gradient stored as bfloat16 is rounded once more: half an ulp of 8 significant bits


def grad_ratio(got, want, g, bf16=False):
  """Worst |got - want| / (1e-5 |g| (1 + |want|)) per element, g (...) the row's
  upstream gradient; a bfloat16 result gets BF16_GRAD |want| on top."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  assert np.isfinite(want).all() and np.isfinite(got).all()
  bar = 1e-5 * np.abs(np.asarray(g, np.float64))[..., None, None] * (1 + np.abs(want))
  if bf16:
    bar = bar + BF16_GRAD * np.abs(want)
  err = np.abs(got - want)
  return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)), initial=0.0))
