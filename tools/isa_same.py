"""Did a change to csrc/ leave the compiler's device output alone?

    python tools/isa_same.py OLD_TREE NEW_TREE > profiles/NAME.txt

OLD_TREE and NEW_TREE are two checkouts of this repository (for instance
`git archive HEAD | tar -x -C /tmp/old` and the working tree).  Every .hip of
NEW_TREE's build.SOURCES is compiled in both to gfx950 assembly with exactly
build.hip_flags() plus --cuda-device-only -S, from inside its csrc/ so that no
path reaches the output.  One line per file: name, kernels (the output's
.amdhsa_kernel lines, counted and nothing more), SHA-256 of the old and of the
new output, equal yes/no.  Exit status 1 if any file differs.  Needs hipcc, no GPU.
"""
import concurrent.futures
import hashlib
import importlib.util
import pathlib
import subprocess
import sys


def load_build(tree):
  spec = importlib.util.spec_from_file_location('_emb_build', tree / 'embodied_amd' / 'build.py')
  build = importlib.util.module_from_spec(spec)     # not via the package: its __init__ needs the .so
  spec.loader.exec_module(build)
  return build


def assembly(build, tree, name):
  cmd = [build.hipcc(), *build.hip_flags(), '--cuda-device-only', '-S', name, '-o', '-']
  res = subprocess.run(cmd, cwd=tree / 'embodied_amd' / 'csrc', capture_output=True)
  if res.returncode:
    raise RuntimeError(f'{tree}: {" ".join(cmd)}\n{res.stderr.decode()}')
  return res.stdout


def compare(old, new):
  build = load_build(new)
  names = [s for s in build.SOURCES if s.endswith('.hip')]
  with concurrent.futures.ThreadPoolExecutor(8) as pool:
    olds = list(pool.map(lambda n: assembly(build, old, n), names))
    news = list(pool.map(lambda n: assembly(build, new, n), names))
  rows = []
  for name, a, b in zip(names, olds, news):
    kernels = sum(line.startswith(b'\t.amdhsa_kernel ') for line in b.splitlines())
    rows.append((name, kernels, hashlib.sha256(a).hexdigest(), hashlib.sha256(b).hexdigest(), a == b))
  return rows


if __name__ == '__main__':
  if len(sys.argv) != 3:
    sys.exit(__doc__)
  rows = compare(*(pathlib.Path(p).resolve() for p in sys.argv[1:]))
  print('# file  kernels  sha256(old)  sha256(new)  equal')
  for name, kernels, a, b, same in rows:
    print(f'{name}  {kernels}  {a}  {b}  {"yes" if same else "NO"}')
  sys.exit(0 if all(r[4] for r in rows) else 1)
