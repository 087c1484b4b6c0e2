"""Cost of `nn.DictConcat` with the masks and the clamp around it
(embodied/jax/nets.py:467-500, dreamerv3/rssm.py:76-79, 137, 216-220): the kernel
of csrc/dict_concat.hip against the composed path of the same module, which is
what a port without this library writes.

    python tools/bench_dict_concat.py [--calls 1000] [--rounds 5] [--out profiles/dict_concat_bench.txt]

The rows:
  the RSSM's action dicts  one discrete key of 18 classes; one float key of 6; two
                           keys of each kind; at 16 and 1024 rows, `reset` and `unit` on
  the Encoder's vectors    8 float keys, 1024 columns in all, `symlog`, at 1024 and
                           65 536 rows
  16 mixed keys            at 1024 rows
each with float32 and bfloat16 out, on two paths:
  composed   `fused=False`: per key a compare, `all`, `where`, the one-hot
             comparison or `symlog`, the cast, `where` and a reshape; then `cat`,
             the reset `where`, `abs`, `maximum`, `div`.
  fused      `fused=True`: one launch.
  entry      `emb_dict_concat` alone through the binding, table and output made
             once: what the fused call costs without the facade's host work.

  us        time between two device events around `calls` back-to-back calls
            ending in a synchronise, after a warm-up of the same shape; the
            paths alternate inside every round; median of the rounds [min .. max].
  ops       device operations (kernels, copies) per call in a torch.profiler
            window of its own, composed / fused.
  ceiling   at the 65 536-row rows: the bytes the call must move (inputs read
            once, the output written once) over the fused median, as a share of
            the copy ceiling of tools/pathbench.py.

The last lines name the rows at which the fused median is below the composed
one, and those where it is not: what `nets._dict_path` is set from.
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


def rows_of():
  """(name, keys as (key, dtype, shape, classes), squish, rows, reset and unit)."""
  disc = [('action', 'int32', (), 18)]
  cont = [('action', 'float32', (6,), None)]
  both = [('a_move', 'int32', (), 18), ('b_arm', 'float32', (6,), None), ('c_tool', 'int32', (), 5), ('d_grip', 'float32', (3,), None)]
  vector = [(f'v{i}', 'float32', (n,), None) for i, n in enumerate((512, 256, 128, 64, 32, 16, 8, 8))]
  kinds = (('float32', (24,), None), ('int32', (), 18), ('int64', (3,), 5), ('uint8', (2,), 4), ('bool', (), 2), ('float32', (2, 3), None))
  mixed = [(f'k{i:02d}', *kinds[i % len(kinds)]) for i in range(16)]
  out = []
  for rows in (16, 1024):
    out += [(f'disc18 {rows}', disc, None, rows, True), (f'float6 {rows}', cont, None, rows, True),
            (f'two of each {rows}', both, None, rows, True)]
  out += [(f'encoder 8 keys x 1024 {rows}', vector, 'symlog', rows, False) for rows in (1024, 65536)]
  out.append(('16 mixed keys 1024', mixed, None, 1024, True))
  return out


def main():
  parser = argparse.ArgumentParser()
  parser.add_argument('--calls', type=int, default=1000)
  parser.add_argument('--rounds', type=int, default=5)
  parser.add_argument('--out', default=str(ROOT / 'profiles' / 'dict_concat_bench.txt'))
  parser.add_argument('--no-profiler', action='store_true')
  args = parser.parse_args()
  assert torch.cuda.is_available(), 'bench_dict_concat needs a GPU'
  from embodied_amd import _lib, nets
  from embodied_amd.space import Space

  device = pathbench.device_line() + '; nets.DictConcat'
  report = pathbench.Report('bench_dict_concat.py', args, device, [
      '# us: time between device events over back-to-back calls, per call: median of rounds [min .. max] (calls per round)',
      '# entry: emb_dict_concat alone through the binding, table and output made once',
      '# ops: device operations per call (torch.profiler window), composed / fused',
      f'# ceiling: share of the copy ceiling ({pathbench.COPY_CEILING_GBS:.0f} GB/s, read + write) the fused median reaches, 65 536-row rows',
      f'# {"row":<34}{"out":<6}{"composed us":<32}{"fused us":<32}{"entry us":<10}{"ops":<16}ceiling',
  ])
  gen = np.random.default_rng(0)
  medians = {}
  for name, keys, squish, rows, masked in rows_of():
    spaces, xs, read = {}, {}, 0
    for key, dtype, shape, classes in keys:
      if classes is None:
        spaces[key] = Space(dtype, shape)
        x = gen.standard_normal((rows, *shape)).astype(dtype)
      elif dtype == 'bool':
        spaces[key] = Space(bool, shape)
        x = gen.integers(0, 2, (rows, *shape)).astype(bool)
      else:
        spaces[key] = Space(dtype, shape, 0, classes)
        x = gen.integers(0, classes, (rows, *shape)).astype(dtype)
      xs[key] = torch.from_numpy(x).cuda()
      read += x.nbytes
    reset = torch.from_numpy(gen.random(rows) < 0.1).cuda() if masked else None
    for kind, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
      concat = nets.DictConcat(spaces, squish=squish, dtype=dtype)
      composed = lambda: concat(xs, reset=reset, unit=masked, fused=False)
      fused = lambda: concat(xs, reset=reset, unit=masked, fused=True)
      a, b = composed().float(), fused().float()
      # the same values from both paths before anything is timed (symlog: within float32 rounding of each other)
      assert torch.allclose(a, b, rtol=1e-6 if squish is None else 2e-2 if kind == 'bf16' else 1e-5, atol=0, equal_nan=True), (name, kind)
      out = torch.empty(rows, concat.width, dtype=dtype, device='cuda')
      table = concat._table(tuple(xs[k].dtype for k in concat.keys))
      for entry_, key in zip(table, concat.keys):
        entry_.x = xs[key].data_ptr()
      stream = _lib.raw_stream(out.device)
      entry = lambda: _lib.fast.emb_dict_concat(table, len(concat.keys), rows, concat.width, out.data_ptr(), concat.width,
                                                nets._DTYPES[dtype], None if reset is None else reset.data_ptr(), int(masked), stream)
      paths = {'composed': composed, 'fused': fused, 'entry': entry}
      got = pathbench.measure(paths, args.calls, args.rounds)
      ops = [None if args.no_profiler else pathbench.device_ops(paths[p]) for p in ('composed', 'fused')]
      medians[name, kind] = {p: got[p].median for p in paths}
      report.verdict(f'{name} {kind}', pathbench.median_below(got['fused'], got['composed']))
      share = '-'
      if rows == 65536:
        moved = read + out.numel() * out.element_size() + (rows if masked else 0)
        share = f'{moved / (got["fused"].median * 1e-6) / 1e9 / pathbench.COPY_CEILING_GBS:.2f}'
      report.add(f'  {name:<34}{kind:<6}{got["composed"].cell:<32}{got["fused"].cell:<32}{got["entry"].median:<10.1f}'
                 f'{" / ".join(pathbench.count(n) for n in ops):<16}{share}')
  report.closing()
  small, large = medians['disc18 16', 'f32'], medians['disc18 1024', 'f32']
  bound = small['fused'] > 2 * small['entry'] and small['fused'] > 0.8 * large['fused']
  report.add(
      f'# 16 rows against 1024, one key of 18 classes, f32: fused {small["fused"]:.1f} / {large["fused"]:.1f} us, the entry '
      f'point alone {small["entry"]:.1f} / {large["entry"]:.1f} us: the fused call at 16 rows is '
      + ('bound by the host\'s enqueue (the facade and the launch), not by the kernel' if bound else
         'not bound by the host\'s enqueue by this measure'))
  report.write()


if __name__ == '__main__':
  main()
