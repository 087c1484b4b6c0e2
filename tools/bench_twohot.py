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
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(16384, 255, 'f32'), (16384, 255, 'bf16'), (1024, 255, 'f32'), (1008, 255, 'f32'), (16384, 256, 'f32')]
COEFS = (1.0, 0.7)
COPY_CEILING_GBS = 6290.0       # the copy ceiling of this part, read + write bytes


def device_us(call, calls):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize()
  start.record()
  for _ in range(calls):
    call()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) * 1e3 / calls


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


def device_ops(call, calls=3):
  """Device-side events per call as torch.profiler sees them (None: no profiler)."""
  try:
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      for _ in range(calls):
        call()
      torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return len(events) / calls
  except Exception as e:      # a figure that was not measured is reported as such
    print(f'# torch.profiler window failed: {e!r}', file=sys.stderr)
    return None


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'twohot_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_twohot needs a GPU'
  from embodied_amd import outs

  lines = [
      f'# tools/bench_twohot.py --calls {args.calls} --rounds {args.rounds}',
      f'# {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}), torch {torch.__version__}; outs.TwoHot, two targets, coefs {COEFS}',
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# ops: device operations per call (torch.profiler window); the kernel rows: the C entry point alone',
      f'# GB/s: bytes the kernel must move / median time; copy ceiling {COPY_CEILING_GBS:.0f} GB/s (read + write)',
      f'# {"shape":<18}{"piece":<10}{"composed us":<34}{"fused us":<34}{"ops composed / fused":<22}fused GB/s',
  ]
  print('\n'.join(lines), flush=True)
  gen = np.random.default_rng(0)
  wins, losses = [], []
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
      def timed(fused, calls):
        return device_us(pieces[fused][piece], calls)
      calls, rounds = {}, {False: [], True: []}
      for fused in rounds:                             # warm-up of this shape; sizes the rounds
        timed(fused, 3)
        estimate = timed(fused, 5)
        calls[fused] = int(min(args.calls, max(5, 0.2e6 / estimate)))
      for _ in range(args.rounds):
        for fused in rounds:
          rounds[fused].append(timed(fused, calls[fused]))
      ops = {f: None if args.no_profiler else device_ops(pieces[f][piece]) for f in rounds}
      cell = lambda f: (f'{statistics.median(rounds[f]):9.1f} [{min(rounds[f]):.1f} .. {max(rounds[f]):.1f}] '
                        f'({calls[f]})')
      count = lambda f: 'not measured' if ops[f] is None else f'{ops[f]:.1f}'
      name = f'{rows}x{n} {kind}'
      if max(rounds[True]) < min(rounds[False]):
        wins.append(f'{name} {piece}')
      else:
        losses.append(f'{name} {piece}')
      line = (f'  {name:<18}{piece:<10}{cell(False):<34}{cell(True):<34}'
              f'{count(False) + " / " + count(True):<22}-')
      lines.append(line)
      print(line, flush=True)
    for piece, call, moved in zip(('stats kernel', 'grad kernel'), kernel_calls(outs, logits, bins, targets, gout),
                                  (size, 2 * size)):
      device_us(call, 50)
      values = [device_us(call, args.calls) for _ in range(args.rounds)]
      median = statistics.median(values)
      rate = moved / median / 1e3
      line = (f'  {f"{rows}x{n} {kind}":<18}{piece:<14}{"":<30}'
              f'{f"{median:9.1f} [{min(values):.1f} .. {max(values):.1f}] ({args.calls})":<34}'
              f'{"- / 1.0":<22}{rate:.0f} = {rate / COPY_CEILING_GBS:.2f} of the ceiling')
      lines.append(line)
      print(line, flush=True)
  lines.append('# fused beats composed, every round of one below every round of the other, at: '
               + (', '.join(wins) or 'no measured shape'))
  lines.append('# fused does not beat composed in every round at: ' + (', '.join(losses) or 'no measured shape'))
  print('\n'.join(lines[-2:]), flush=True)
  out = pathlib.Path(args.out)
  out.parent.mkdir(parents=True, exist_ok=True)
  out.write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
