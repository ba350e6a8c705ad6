"""tests/span_model.py and lddl_span_params pinned on the host: the solver
against the closed forms of include/lddl_amd.h, the model with max_span 1
against tests/wwm_model.py, the statistics the definition promises, and
hand-made rows.  No GPU: lddl_span_params needs no ctx."""
import ctypes
import fractions

import numpy as np
import pytest

import mask_model as mm
import span_model as sm
import wwm_model as wm

# a vocabulary of 40 entries: 0 [PAD], 1 [CLS], 2 [SEP], 3 [MASK], 4..21 words, 22..39 '##' pieces
V, CLS, SEP, MASK, IGNORE = 40, 1, 2, 3, -1
TABLE = np.arange(V) >= 22
LAWS = [(10, 0.2), (3, 0.5), (16, 0.05)]
EINVAL = -1


def raw_params(L, g, p, q=True, cdf=True):
  from lddl_amd import _lib
  qv, cv = ctypes.c_double(-1.0), (ctypes.c_double * 16)(*([-1.0] * 16))
  rc = _lib.lib().lddl_span_params(L, g, p, ctypes.byref(qv) if q else None, cv if cdf else None)
  return rc, qv.value, list(cv)


def exact_cdf(L, g):
  """cdf[1 .. L] of the law, the closed form in exact rational arithmetic over the double g, rounded once"""
  g = fractions.Fraction(g)
  return np.asarray([float((1 - (1 - g) ** t) / (1 - (1 - g) ** L)) for t in range(1, L + 1)])


@pytest.mark.parametrize('L,g', LAWS + [(1, 0.3), (16, 1.0), (2, 1e-9), (16, 1e-3)])
def test_cdf_is_the_closed_form(L, g):
  for p in (0.0, 0.15, 1.0):
    q, cdf = sm.params(L, g, p)
    assert np.abs(cdf[:L] - exact_cdf(L, g)).max() <= 1e-15
    assert cdf[L - 1] == 1.0 and (cdf[L:] == 1.0).all() and (np.diff(cdf) >= 0).all()
    assert L == 1 or cdf[L - 2] < 1.0 or g == 1.0
  if g > 0.01:  # (the double form of the law cancels for a small g)
    assert np.abs(np.cumsum(sm.law(L, g)) - exact_cdf(L, g)).max() <= 1e-14


@pytest.mark.parametrize('p', [0.15, 0.3, 0.5])
@pytest.mark.parametrize('L,g', LAWS)
def test_q_covers_an_interior_word_with_probability_p(L, g, p):
  q, cdf = sm.params(L, g, p)
  S = np.concatenate([[1.0], 1.0 - cdf[:L - 1]])  # S_0 .. S_{L-1}
  assert abs(1.0 - np.prod(1.0 - q * S) - p) <= 1e-12
  assert 0.0 < q < p


def test_q_at_the_ends_and_for_single_words():
  for p in (0.0, 0.15, 0.3, 1.0 / 3, 1.0):
    for g in (0.2, 1.0):
      assert sm.params(1, g, p)[0] == p  # exactly
  for L, g in LAWS:
    assert sm.params(L, g, 0.0)[0] == 0.0 and sm.params(L, g, 1.0)[0] == 1.0
  # g = 1: every span has one word, whatever L
  assert abs(sm.params(7, 1.0, 0.25)[0] - 0.25) <= 1e-15


@pytest.mark.parametrize('L,g,p', [(0, 0.2, 0.15), (17, 0.2, 0.15), (-1, 0.2, 0.15), (10, 0.0, 0.15), (10, -0.1, 0.15),
                                   (10, 1.0001, 0.15), (10, float('nan'), 0.15), (10, 0.2, -0.01), (10, 0.2, 1.01),
                                   (10, 0.2, float('nan')), (10, float('inf'), 0.15)])
def test_refused_parameters(L, g, p):
  from lddl_amd import _lib
  rc, q, cdf = raw_params(L, g, p)
  assert rc == EINVAL and _lib.lib().lddl_last_error()
  assert q == -1.0 and cdf == [-1.0] * 16  # nothing written


def test_null_outputs_are_refused():
  assert raw_params(10, 0.2, 0.15, q=False)[0] == EINVAL
  assert raw_params(10, 0.2, 0.15, cdf=False)[0] == EINVAL
  assert raw_params(10, 0.2, 0.15)[0] == 0


def random_rows(n, S, seed, p_cont=0.45, p_special=0.04):
  """[CLS] first, specials sprinkled in mid-row, a padded tail of random length; ids in and around the vocabulary"""
  rng = np.random.default_rng(seed)
  ids = np.where(rng.random((n, S)) < p_cont, rng.integers(22, V, (n, S)), rng.integers(4, 22, (n, S))).astype(np.int64)
  sp = (rng.random((n, S)) < p_special).astype(np.int64)
  sp[:, 0] = 1
  for r in range(n):
    sp[r, S - int(rng.integers(0, S // 4)):] = 1
  ids[sp != 0] = SEP
  return ids, sp


@pytest.mark.parametrize('g', [0.2, 1.0])
@pytest.mark.parametrize('p', [0.15, 0.5])
def test_max_span_1_is_whole_word_masking(p, g):
  ids, sp = random_rows(40, 150, 3)
  ids[5, 7], ids[6, 9] = V + 3, -2  # ids outside the vocabulary are no continuations
  rows = np.arange(40) + (1 << 30)
  for seed, counter in ((31, 9), ((1 << 63) + 12345, 1 << 40)):
    a = sm.mask(ids, sp, TABLE, seed, counter, p, 1, g, MASK, V, IGNORE, rows=rows)
    b = wm.mask(ids, sp, TABLE, seed, counter, p, MASK, V, IGNORE, rows=rows)
    for k in ('input_ids', 'labels', 'select', 'masked', 'random'):
      assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.select.any() and (a.length[a.open] == 1).all()


def test_no_continuations_and_max_span_1_is_token_masking():
  ids, sp = random_rows(20, 90, 4, p_cont=0.0)
  a = sm.mask(ids, sp, None, 7, 2, 0.3, 1, 0.2, MASK, V, IGNORE)
  b = mm.mask(ids, sp, 7, 2, 0.3, MASK, V, IGNORE)
  assert np.array_equal(a.input_ids, b.input_ids) and np.array_equal(a.labels, b.labels)


@pytest.mark.parametrize('L,g,p', [(10, 0.2, 0.15), (3, 0.5, 0.5), (16, 0.05, 0.3)])
def test_statistics(L, g, p):
  """Over N >= 200 000 interior words (word index >= L within the segment) the selected fraction is p to within
  5 sigma, sigma^2 = (2L - 1) p (1 - p) / N: the coverage of words fewer than L apart is correlated (they share
  heads), so a word's indicator has at most 2L - 1 correlated neighbours, itself included.  The mean drawn length of
  the open heads is the law's mean to within 5 standard errors."""
  n, S = 800, 512
  ids, sp = random_rows(n, S, 11, p_cont=0.2, p_special=0.004)
  m = sm.mask(ids, sp, TABLE, 12345, 6, p, L, g, MASK, V, IGNORE)
  first = wm.starts(ids, sp, TABLE)  # one count per word: at its first column
  interior = first & (m.word >= L)
  N = int(interior.sum())
  assert N >= 200_000
  assert abs(m.select[interior].mean() - p) <= 5.0 * np.sqrt((2 * L - 1) * p * (1 - p) / N)
  # the first words of a segment see fewer heads in front of them: covered less often, the very first with q
  q, _ = sm.params(L, g, p)
  edge = first & (m.word == 1)
  ne = int(edge.sum())
  assert abs(m.select[edge].mean() - q) <= 5.0 * np.sqrt(q * (1 - q) / ne) and q < p
  # a word is selected whole
  head = wm.heads(ids, sp, TABLE)
  assert np.array_equal(m.select, np.take_along_axis(m.select, head, axis=1) & (sp == 0))
  # lengths
  pl, l = sm.law(L, g), np.arange(1, L + 1)
  mean, var = (l * pl).sum(), (l * l * pl).sum() - (l * pl).sum() ** 2
  drawn = m.length[m.open]
  assert drawn.min() >= 1 and drawn.max() <= L and len(drawn) > 1000
  assert abs(drawn.mean() - mean) <= 5.0 * np.sqrt(var / len(drawn))
  assert abs(m.open[first].mean() - q) <= 5.0 * np.sqrt(q * (1 - q) / int(first.sum()))
  # 80 / 10 / 10 of the selected tokens, per token
  k = int(m.select.sum())
  assert abs(m.masked.sum() / k - 0.8) <= 5.0 * np.sqrt(0.16 / k)
  assert abs(m.random.sum() / k - 0.1) <= 5.0 * np.sqrt(0.09 / k)


def find(rows_of, want, L, g, p, tries=400):
  """the first counter at which the model's planes of the row satisfy want"""
  ids, sp = rows_of
  for counter in range(tries):
    m = sm.mask(ids, sp, TABLE, 5, counter, p, L, g, MASK, V, IGNORE)
    if want(m):
      return m
  raise AssertionError('no such draw in %d counters' % tries)


def W(i):
  return 4 + i % 18


def C(i):
  return 22 + i % 18


def test_a_span_is_clipped_at_sep():
  # [CLS] w w w w [SEP] w w w w [SEP] pad pad: columns 1..4 and 6..9
  ids = np.asarray([[CLS, W(0), W(1), W(2), W(3), SEP, W(4), W(5), W(6), W(7), SEP, 0, 0]], np.int64)
  sp = np.asarray([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1]], np.int64)
  # the only open head is the last word of A, with a span of three words or more
  m = find((ids, sp), lambda m: np.flatnonzero(m.open[0]).tolist() == [4] and m.length[0, 4] >= 3, 10, 0.2, 0.5)
  assert np.flatnonzero(m.select[0]).tolist() == [4]
  assert (m.labels[0, 5:] == IGNORE).all() and np.array_equal(m.input_ids[0, 5:], ids[0, 5:])
  # and of B, past the final [SEP] and the padding
  m = find((ids, sp), lambda m: np.flatnonzero(m.open[0]).tolist() == [8] and m.length[0, 8] >= 4, 10, 0.2, 0.5)
  assert np.flatnonzero(m.select[0]).tolist() == [8, 9]
  # inside a segment the same length runs its course
  m = find((ids, sp), lambda m: np.flatnonzero(m.open[0]).tolist() == [6] and m.length[0, 6] == 3, 10, 0.2, 0.5)
  assert np.flatnonzero(m.select[0]).tolist() == [6, 7, 8]


def test_a_segment_that_begins_with_a_piece_starts_a_word():
  # [CLS] w ##c [SEP] ##c ##c w ##c w [SEP]: B's words are columns 4..5, 6..7 and 8
  ids = np.asarray([[CLS, W(0), C(0), SEP, C(1), C(2), W(1), C(3), W(2), SEP]], np.int64)
  sp = np.asarray([[1, 0, 0, 1, 0, 0, 0, 0, 0, 1]], np.int64)
  assert np.flatnonzero(wm.starts(ids, sp, TABLE)[0]).tolist() == [1, 4, 6, 8]
  m = find((ids, sp), lambda m: np.flatnonzero(m.open[0]).tolist() == [4] and m.length[0, 4] == 2, 3, 0.5, 0.5)
  assert m.word[0].tolist() == [0, 1, 1, 0, 1, 1, 2, 2, 3, 0]
  assert np.flatnonzero(m.select[0]).tolist() == [4, 5, 6, 7]
  # A's word before the [SEP] does not reach the pieces behind it
  m = find((ids, sp), lambda m: np.flatnonzero(m.open[0]).tolist() == [1] and m.length[0, 1] >= 2, 3, 0.5, 0.5)
  assert np.flatnonzero(m.select[0]).tolist() == [1, 2]


def test_overlapping_spans_union():
  ids = np.asarray([[CLS] + [W(i) for i in range(10)] + [SEP]], np.int64)
  sp = np.asarray([[1] + [0] * 10 + [1]], np.int64)

  def want(m):
    h = np.flatnonzero(m.open[0]).tolist()
    return len(h) == 2 and h[1] - h[0] < m.length[0, h[0]] and h[1] + m.length[0, h[1]] > h[0] + m.length[0, h[0]]
  m = find((ids, sp), want, 10, 0.2, 0.3)
  h0, h1 = np.flatnonzero(m.open[0]).tolist()
  end = min(h1 + int(m.length[0, h1]), 11)
  assert np.flatnonzero(m.select[0]).tolist() == list(range(h0, end))
