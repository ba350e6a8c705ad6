"""tests/mask_regimes.py on the host: for every configuration the GPU tests
run, the oracle's rows alone reach every regime of the masked packer that the
configuration is there for (conditions on the corpus, not measurements: a
corpus seed that misses one fails here), and the instantiation is the one the
launch would pick."""
import pytest

import mask_regimes as mr


@pytest.mark.parametrize('seq,ratio', mr.CONFIGS)
def test_oracle_rows_reach_required_regimes(seq, ratio):
  _, _, rows = mr.oracle_rows(seq, ratio)
  inst, req = mr.required(seq, ratio)
  assert mr.instantiation(seq, ratio) == inst
  got = mr.classify(rows, seq, ratio)
  assert not req - got, sorted(req - got, key=str)


def test_instantiation_thresholds():
  """MASK = 1 up to MLM_PICKS_1 picks at the longest row of seq <= 512"""
  assert mr.instantiation(512, 0.5) == 1 and mr.instantiation(512, 0.502) == 2  # rint(257.02) = 257
  assert mr.instantiation(512, 513 / 1024) == 1  # rint(256.5) = 256, half to even
  assert mr.instantiation(128, 1.0) == 1 and mr.instantiation(128, 0.0) == 1
  assert mr.instantiation(1024, 0.0) == 2 and mr.instantiation(513, 0.15) == 2


def test_pair_regime_by_hand():
  """rows written out by hand against the kernel's formulas"""
  ids = list(range(1000, 2000))
  row = lambda a, b, pos, expl=False: (a, b, False, len(a) + len(b) + 3, pos, [0] * len(pos), expl)  # noqa: E731
  # seq 1024, ratio 0.6: n = 854 -> 512 picks, 512 + 512 <= 1024 splits; n = 855 -> 513 picks, unsplit
  r = mr.pair_regime(row(ids[:400], ids[:451], list(range(1, 401)) + list(range(402, 514))), 1024, 0.6)
  assert (r['nm'], r['split'], r['tr8'], r['chunks']) == (512, True, 512, 6)
  r = mr.pair_regime(row(ids[:400], ids[:452], list(range(1, 401)) + list(range(402, 515))), 1024, 0.6)
  assert (r['nm'], r['split'], r['tr8'], r['chunks']) == (513, False, 856, 0)
  # no candidates at all; one candidate
  r = mr.pair_regime(row([mr.SEP], [mr.CLS, mr.CLS], [], True), 128, 0.15)
  assert (r['m'], r['nm'], r['split'], r['tr8']) == (0, 0, False, 0)
  r = mr.pair_regime((([mr.MASK_ID], [mr.CLS], False, 5, [1], [1500], True)), 128, 0.15)
  assert (r['m'], r['nm'], r['split'], r['tr8']) == (1, 1, False, 8)
  assert mr.classify([[row([mr.SEP], [mr.CLS], [], True)]], 128, 1.0) == {('zero',), ('nm', 0), ('tr8', 0), ('passes', 0)}
