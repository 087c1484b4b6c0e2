"""build.SOURCES names exactly the translation units under csrc/ (no GPU).  A
shared library links without complaint when a unit is missing: its launchers
are undefined symbols that fail only when the library is loaded."""
import importlib.util
import pathlib

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_sources_list_every_translation_unit():
  spec = importlib.util.spec_from_file_location('_emb_build', ROOT / 'embodied_amd' / 'build.py')
  build = importlib.util.module_from_spec(spec)     # not via the package: its __init__ needs the .so
  spec.loader.exec_module(build)
  on_disk = {str(p.relative_to(build.CSRC)) for p in build.CSRC.rglob('*') if p.suffix in ('.hip', '.cpp')}
  assert len(build.SOURCES) == len(set(build.SOURCES)), build.SOURCES
  assert set(build.SOURCES) - on_disk == set(), 'listed in SOURCES, not in csrc/'
  assert on_disk - set(build.SOURCES) == set(), 'in csrc/, not listed in SOURCES'
