"""One line per gfx950 kernel of the given .hip files: what the compiler made of it.

    python tools/kernel_table.py embodied_amd/csrc/movers.hip ... > profiles/kernel_table.txt

Each file is compiled for the device only with build.py's flags and
-Rpass-analysis=kernel-resource-usage; a line holds the demangled kernel name,
its SGPRs, VGPRs, AGPRs, scratch bytes per lane, LDS bytes per workgroup,
occupancy (waves per SIMD) and the size of its symbol in the device object
(llvm-readelf -s).  The lines are sorted by name and carry no file name: two
arrangements of the same kernels over translation units give the same table
exactly when every kernel came out the same.  Needs hipcc, no GPU.
"""
import importlib.util
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location('_emb_build', ROOT / 'embodied_amd' / 'build.py')
build = importlib.util.module_from_spec(_spec)    # not via the package: its __init__ needs the .so
_spec.loader.exec_module(build)

FIELDS = [('sgpr', r'TotalSGPRs: (\d+)'), ('vgpr', r' VGPRs: (\d+)'), ('agpr', r'AGPRs: (\d+)'),
          ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('lds', r'LDS Size \[bytes/block\]: (\d+)'),
          ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)')]


def resource_remarks(text):
  """{mangled kernel name: {field: value}} from the compiler's remarks."""
  kernels, cur = {}, None
  for line in text.splitlines():
    m = re.search(r'Function Name: (\S+)', line)
    if m:
      cur = kernels.setdefault(m.group(1), {})
      continue
    for field, pattern in FIELDS:
      m = re.search(pattern, line)
      if m and cur is not None:
        cur[field] = int(m.group(1))
  return kernels


def symbol_sizes(obj, readelf):
  """{symbol: bytes} of the FUNC symbols of a device object."""
  out = subprocess.run([readelf, '-s', '-W', str(obj)], capture_output=True, text=True, check=True).stdout
  sizes = {}
  for line in out.splitlines():
    parts = line.split()
    if len(parts) == 8 and parts[3] == 'FUNC':
      sizes[parts[7]] = int(parts[2])
  return sizes


def demangle(names):
  tool = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
  if not tool or not names:
    return dict(zip(names, names))
  out = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True, check=True).stdout
  return dict(zip(names, out.splitlines()))


def table(sources):
  cc = pathlib.Path(build.hipcc())
  readelf = shutil.which('llvm-readelf') or str(cc.resolve().parent.parent / 'llvm' / 'bin' / 'llvm-readelf')
  rows = {}
  with tempfile.TemporaryDirectory() as tmp:
    for source in map(pathlib.Path, sources):
      obj = pathlib.Path(tmp) / (source.name + '.device.o')
      cmd = [str(cc), *build.hip_flags(), '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only',
             '--no-gpu-bundle-output', '-c', str(source), '-o', str(obj)]
      res = subprocess.run(cmd, capture_output=True, text=True)
      if res.returncode:
        raise RuntimeError(f'{" ".join(cmd)}\n{res.stderr}')
      sizes = symbol_sizes(obj, readelf)
      for name, fields in resource_remarks(res.stderr).items():
        if name in rows:
          raise RuntimeError(f'{name} is defined by more than one file')
        rows[name] = dict(fields, size=sizes[name])
  pretty = demangle(sorted(rows))
  return sorted(
      f'{pretty[name]}  sgpr={r["sgpr"]} vgpr={r["vgpr"]} agpr={r["agpr"]} scratch={r["scratch"]} '
      f'lds={r["lds"]} occupancy={r["occupancy"]} size={r["size"]}' for name, r in rows.items())


if __name__ == '__main__':
  if len(sys.argv) < 2:
    sys.exit(__doc__)
  print('\n'.join(table(sys.argv[1:])))
