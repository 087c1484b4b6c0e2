"""TEST INFRASTRUCTURE, build container only (needs the reference tree).  Usage:

    python -m oracle.gen_reference_runs

Runs every function the suite registers with `tests.reference_record.recorded`
(the reference's own code on the suite's inputs) and writes what they return to
tests/golden/reference_runs.json: the record the suite compares against on
machines where the reference tree is not readable."""
import importlib
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

MODULES = ['tests.test_oracle_golden', 'tests.test_wrappers_host', 'tests.test_scan_golden',
           'tests.test_normalize_golden', 'tests.test_limiters_streams_host', 'tests.test_run_loops_host',
           'tests.test_product_chunks_host', 'tests.test_param_counts_host']


def main():
  from oracle import refload
  if not refload.available():
    raise SystemExit(f'reference tree not readable at {refload.REFERENCE}')
  from tests import reference_record
  for name in MODULES:
    importlib.import_module(name)
  out = {name: reference_record.plain(reference_record.RUNS[name]()) for name in sorted(reference_record.RUNS)}
  with open(reference_record.PATH, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
  print(f'{len(out)} records -> {reference_record.PATH.relative_to(ROOT)}')


if __name__ == '__main__':
  main()
