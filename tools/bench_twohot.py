"""Cost of the symexp_twohot head of one train step: the composed torch ops
against the kernels of csrc/twohot.hip.

    python tools/bench_twohot.py [--calls 1000] [--rounds 5] [--out profiles/twohot_bench.txt]

Per shape and dtype three pieces, each on both paths of `outs.TwoHot`:

  stats     a fresh head's `pred()`: on the kernels that is the one pass that
            also leaves the rows' log-sum-exp.
  loss_sum  `loss_sum((t1, t2), (1.0, 0.7))` of a fresh head, forward only,
            under autograd (the fused figure includes the stats launch, as a
            train step that has not asked for `pred()` pays it).
  backward  `.backward(gout, retain_graph=True)` of one such loss, again and
            again, with a grad_output that differs from row to row (the graph is
            kept so that the backward pass is timed alone; `.grad` is dropped
            between calls, so nothing is accumulated).
and, for the kernels alone, `emb_twohot_stats` and `emb_twohot_grad` called
through the C ABI on buffers made once (`stats kernel`, `grad kernel`): the
façade's pieces above cost the larger of the host's enqueue time and the
device's time, and at these sizes the host's.

  us        time between two device events around `calls` back-to-back calls,
            after a warm-up of the same shape; the paths alternate inside every
            round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own.
  GB/s      for the two kernel rows: the bytes the kernel must move (stats: the
            logits once; grad: the logits once and the gradient once) over the
            median time, beside the copy ceiling that DESIGN.md quotes.

The last lines name the shapes at which the kernels beat the composed path in
every round, and those where they do not: what `outs._path` is set from.
Needs a GPU: there is no CPU fallback and no figure without one.
"""
import argparse
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import pathbench  # noqa: E402
from tools.pathbench import COPY_CEILING_GBS, device_us  # noqa: E402

SHAPES = [(16384, 255, 'f32'), (16384, 255, 'bf16'), (1024, 255, 'f32'), (1008, 255, 'f32'), (16384, 256, 'f32')]
COEFS = (1.0, 0.7)


def backward_call(forward, logits, gout):
  """One forward now; the call repeats its backward pass alone."""
  loss = forward()

  def call():
    logits.grad = None
    loss.backward(gout, retain_graph=True)
  return call


def kernel_calls(outs, logits, bins, targets, gout):
  """`emb_twohot_stats` and `emb_twohot_grad` through the C ABI, buffers made once."""
  import ctypes as C
  from embodied_amd import _lib
  head = outs.TwoHot(logits, bins, fused=True)
  lse, pred = (t.clone() for t in head._stats())
  x, dev_bins, grad = head._x, head._bins, torch.empty_like(head._x)
  rows, n = x.shape
  ptrs = (C.c_void_p * 2)(*[t.data_ptr() for t in targets])
  coefs = (C.c_float * 2)(*COEFS)
  stream = _lib.raw_stream(x.device)
  keep = (head, lse, pred, grad, ptrs, coefs)
  stats = lambda keep=keep: _lib.api.emb_twohot_stats(
      x.data_ptr(), head._dtype, rows, n, dev_bins.data_ptr(), lse.data_ptr(), pred.data_ptr(), stream)
  grads = lambda keep=keep: _lib.api.emb_twohot_grad(
      x.data_ptr(), head._dtype, rows, n, dev_bins.data_ptr(), lse.data_ptr(), ptrs, coefs, 2, gout.data_ptr(),
      grad.data_ptr(), stream)
  return stats, grads


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'twohot_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_twohot needs a GPU'
  from embodied_amd import outs

  device = pathbench.device_line() + f'; outs.TwoHot, two targets, coefs {COEFS}'
  report = pathbench.Report('bench_twohot.py', args, device, [
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window); the kernel rows: the C entry point alone',
      f'# GB/s: bytes the kernel must move / median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<18}{"piece":<10}{"composed us":<34}{"fused us":<34}{"ops composed / fused":<22}fused GB/s',
  ])
  gen = np.random.default_rng(0)
  for rows, n, kind in SHAPES:
    dtype = torch.float32 if kind == 'f32' else torch.bfloat16
    bins = outs.symexp_twohot_bins(n)
    logits = torch.from_numpy(gen.standard_normal((rows, n)).astype(np.float32)).cuda().to(dtype).requires_grad_()
    targets = [torch.from_numpy(np.sign(x) * np.expm1(np.abs(x))).float().cuda()
               for x in gen.uniform(-20, 20, (2, rows))]
    gout = torch.from_numpy(gen.standard_normal(rows).astype(np.float32)).cuda()
    size = logits.element_size() * rows * n
    pieces = {}
    for fused in (False, True):
      head = lambda fused=fused: outs.TwoHot(logits, bins, fused=fused)
      forward = lambda head=head: head().loss_sum(targets, COEFS)
      pieces[fused] = dict(stats=lambda head=head: head().pred(), loss_sum=forward, forward=forward)
    # the same values from both paths before anything is timed
    a, b = (pieces[f]['stats']() for f in (False, True))
    scale = 1 + (torch.softmax(logits.detach().float(), -1) * torch.from_numpy(bins).cuda()).abs().sum(-1)
    assert ((a - b).abs() <= 2e-5 * scale).all(), (rows, n, kind, 'pred')
    grads = []
    for f in (False, True):
      logits.grad = None
      pieces[f]['forward']().backward(gout)
      grads.append(logits.grad.float().clone())
    tol = 1e-5 if kind == 'f32' else 2.0 ** -7
    assert torch.allclose(grads[0], grads[1], rtol=tol, atol=1e-5), (rows, n, kind, 'grad')
    assert torch.allclose(pieces[False]['forward'](), pieces[True]['forward'](), rtol=1e-5, atol=1e-5)
    for f in (False, True):
      pieces[f]['backward'] = backward_call(pieces[f]['forward'], logits, gout)
    for piece in ('stats', 'loss_sum', 'backward'):
      paths = {f: pieces[f][piece] for f in (False, True)}
      got = pathbench.measure(paths, args.calls, args.rounds, budget_us=0.2e6)
      ops = {f: None if args.no_profiler else pathbench.device_ops(paths[f]) for f in paths}
      name = f'{rows}x{n} {kind}'
      report.verdict(f'{name} {piece}', pathbench.every_round_below(got[True], got[False]))
      report.add(f'  {name:<18}{piece:<10}{got[False].cell:<34}{got[True].cell:<34}'
                 f'{pathbench.count(ops[False]) + " / " + pathbench.count(ops[True]):<22}-')
    for piece, call, moved in zip(('stats kernel', 'grad kernel'), kernel_calls(outs, logits, bins, targets, gout),
                                  (size, 2 * size)):
      device_us(call, 50)
      alone = pathbench.run_rounds({piece: call}, args.calls, args.rounds)[piece]
      rate = moved / alone.median / 1e3
      report.add(f'  {f"{rows}x{n} {kind}":<18}{piece:<14}{"":<30}{alone.cell:<34}'
                 f'{"- / 1.0":<22}{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')
  report.closing('fused beats composed, every round of one below every round of the other, at',
                 'fused does not beat composed in every round at', none='no measured shape')
  report.write()


if __name__ == '__main__':
  main()
