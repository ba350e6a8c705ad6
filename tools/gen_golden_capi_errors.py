"""Record tests/golden/capi_errors.json: the return code and lddl_last_error()
text of every refusal in tests/capi_error_cases.py, from the library of the
commit that a change to the C API's host side is compared against.

  tools/ab_head.sh <parent rev> head
  LDDL_LIB=ab/lib_head.so python tools/gen_golden_capi_errors.py

Needs a GPU.  Every case must be refused (rc < 0): one that the library
accepts is a mistake in the table.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import capi_error_cases  # noqa: E402


def main():
  recs = [dict(call=c, case=k, rc=rc, message=m) for c, k, rc, m in capi_error_cases.run_all()]
  accepted = [(r['call'], r['case'], r['rc']) for r in recs if r['rc'] >= 0]
  assert not accepted, accepted
  keys = [(r['call'], r['case']) for r in recs]
  assert len(set(keys)) == len(keys), [k for k in keys if keys.count(k) > 1]
  out = os.path.join(ROOT, 'tests', 'golden', 'capi_errors.json')
  with open(out, 'w') as f:
    json.dump(recs, f, indent=0, sort_keys=True)
    f.write('\n')
  print('%d refusals of %d calls -> %s (library: %s)' % (
      len(recs), len({r['call'] for r in recs}), out, os.environ.get('LDDL_LIB', 'the working tree')))


if __name__ == '__main__':
  main()
