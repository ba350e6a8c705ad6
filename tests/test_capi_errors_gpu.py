"""The refusals of the C API are those of tests/golden/capi_errors.json: the
return code and the lddl_last_error() text of every case in
tests/capi_error_cases.py, recorded from the parent commit's library by
tools/gen_golden_capi_errors.py when the host side (lddl_amd/csrc/capi*.hip)
was split by subsystem.  Compared exactly, in the table's order.
"""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'capi_errors.json')


def test_refusals_are_unchanged(gpu):
  import capi_error_cases
  with open(GOLDEN) as f:
    exp = json.load(f)
  got = [dict(call=c, case=k, rc=rc, message=m) for c, k, rc, m in capi_error_cases.run_all()]
  assert [(r['call'], r['case']) for r in got] == [(r['call'], r['case']) for r in exp]  # the table the fixture was made from
  assert exp and all(r['rc'] < 0 for r in exp)
  bad = [(g, e) for g, e in zip(got, exp) if g != e]
  assert not bad, 'differs from the recorded refusal (got, expected): %r' % (bad[:5],)
