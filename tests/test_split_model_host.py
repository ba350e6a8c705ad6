"""The byte-level model of the GPU sentence split (tests/split_model.py) held
to the host path it restates, preprocess.split_records with the rule-based
splitter, in both modes (id + body, whole line): identical sentence bytes,
offsets, document offsets and ids on adversarial, random-code-point, edge and
synthetic Wikipedia records, on structures shifted through every 64-byte step
and a piece boundary, and on degenerate records; and every kind of invalid
UTF-8 is invalid in the model and raises in the Python path."""
import numpy as np
import pytest

import split_model as M

MODES = [pytest.param(False, id='id_body'), pytest.param(True, id='whole_line')]


def _check(records, whole_line):
  raws = [r.encode('utf-8') for r in records]
  buf, rec_off = M.join(raws)
  data, so, dso, id_end = M.split_model(buf, rec_off, 1 if whole_line else 0)
  edata, eso, edso, eids = M.reference(records, whole_line)
  assert np.array_equal(dso, edso)
  assert np.array_equal(so, eso)
  assert data == edata
  assert M.model_ids(raws, id_end, rec_off) == eids


@pytest.mark.parametrize('whole_line', MODES)
@pytest.mark.parametrize('seed', range(4))
def test_adversarial(seed, whole_line):
  _check(M.adversarial(seed, 3000), whole_line)


@pytest.mark.parametrize('whole_line', MODES)
def test_random_code_points(whole_line):
  _check(M.random_code_points(11, 2000), whole_line)


@pytest.mark.parametrize('whole_line', MODES)
def test_edge_and_wiki(whole_line):
  _check(M.EDGE, whole_line)
  _check(M.wiki(300_000), whole_line)


@pytest.mark.parametrize('whole_line', MODES)
def test_shift_sweep(whole_line):
  recs = M.shift_sweep()
  # every case starts on a piece boundary, so shift k puts its structure k + 4 bytes behind one
  buf, rec_off = M.join([r.encode('utf-8') for r in recs])
  assert sum(1 for r in range(len(recs)) if not recs[r].startswith('p') and rec_off[r] % M.PIECE == 0) == \
      len(M.STRUCTURES) * len(M.SHIFTS)
  _check(recs, whole_line)


def test_shift_sweep_structures_decide_as_meant():
  """the hand-made structures break (or not) where they were built to"""
  def n(body):
    return len(M.reference(['id ' + body], False)[1]) - 1
  assert n('He met Mr. Smith today. Then left') == 2 and n('In the U.S. Army now. Yes') == 2
  assert n('See e.g. Figure two. Done') == 2 and n('It is approx. Five of them') == 1
  assert n('Temp K. Next one') == 1 and n('Name É. Next') == 1 and n('Name Σ. Next') == 1
  assert n('Name İ. Next') == 2  # (its lower() is two characters)
  assert n('What?!")] 　Next one') == 2 and n('End.\u0085Next.\u0085\u0085Again') == 3
  assert n('Wow' + '!' * 70 + ' Next') == 2 and n('End.' + ')' * 70 + ' Next') == 2
  assert n('End.' + ' ' * 70 + 'Next') == 2 and n('(' * 70 + 'mr. Smith') == 1 and n('(["' * 67 + 'cat. Next') == 2
  assert n('. Next one') == 2 and n('The end.   ') == 1


@pytest.mark.parametrize('whole_line', MODES)
def test_degenerate(whole_line):
  for recs in M.degenerate(300_000):
    _check(recs, whole_line)


@pytest.mark.parametrize('raw', M.INVALID)
def test_invalid_utf8(raw):
  with pytest.raises(UnicodeDecodeError):
    raw.decode('utf-8')
  for raws, bad in (([raw], [0]), ([b'ok A. B.', raw, b'fine. C'], [1]), ([raw, b'', raw], [0, 2])):
    buf, rec_off = M.join(raws)
    assert M.invalid_records(buf, rec_off) == bad
    for mode in (0, 1):
      with pytest.raises(M.InvalidUtf8) as e:
        M.split_model(buf, rec_off, mode)
      assert e.value.bad == bad


def test_truncated_then_continuation():
  """a record ending inside a sequence and the next one starting with its continuation bytes: the buffer as a
  whole decodes, both records are invalid, the first is the lowest"""
  raws = [b'ok. Fine', b'id trunc \xe2\x82', b'', b'\xac rest. A', b'id good']
  buf, rec_off = M.join(raws)
  buf.decode('utf-8')
  for r in (1, 3):
    with pytest.raises(UnicodeDecodeError):
      raws[r].decode('utf-8')
  assert M.invalid_records(buf, rec_off) == [1, 3]


def test_valid_records_are_valid():
  recs = M.adversarial(5, 300) + M.random_code_points(6, 300)
  buf, rec_off = M.join([r.encode('utf-8') for r in recs])
  assert M.invalid_records(buf, rec_off) == []
