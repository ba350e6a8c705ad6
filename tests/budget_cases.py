"""The inputs of the exact-count masking tests (lddl_set_mask_budget) that can
be made without a GPU: the hand-made rows of tests/test_mask_budget_gpu.py, and
the committed cases that drive the radix select of mask_budget.hip to a chosen
level and exit.  Plain helper module: no tests, no fixtures.

  ROWS, segments(), cont()   the row table's rows over 'tiny64' (tests/synth_vocab.py)
  Case, CASES                the committed cases
  planes(case)               (ids, special) [row + 1, S] as the front end sees the batch
  units(case)                (keys, weights, budget) of the case's row
  trace(case)                budget_model.radix_steps of it

A case is `(front, seed, counter, row, n, word, P, p, src)`: the front end
('mask_tokens': lddl_mask_tokens over planes; 'rows': a row-table collate,
mask_budget_kernel), the collate's base seed and batch counter, the batch row
and its number of columns, whole-word mode, max_predictions and
mlm_probability, and where the row comes from: for 'mask_tokens' the
(generator seed, density of special columns) of token_plane, for 'rows' the
index into ROWS.  The rows in front of the case's row are ROWS[0].

How the deep cases were found (once, on the host; only the constants are
kept).  The key of column h is (sm(k + 3 ((row << 20) | h)) & ~0xFFFFF) | h.
Two units whose keys share 8 L bits or more stay in one bin down to level L,
so the search has to go on to level L when it looks for the second of them:
for a candidate seed all keys of the row are sorted, an adjacent pair with a
long common prefix is taken, p is 1.0 and P the weight in front of the pair's
second key (were it the first, the search would end at a shallow level, the
bin holding nothing in front of it).  In whole-word mode P plus all but one of
that word's tokens gives the exit where a word fits in part.  A third key
right behind the pair and as close gives a bin of several heads at the exit.
tests/test_budget_model_host.py derives each case's exit again and holds the
table to what the suite claims to cover.
"""
import collections
import functools

import numpy as np

import budget_model as bm
import mask_model as mm
import synth_vocab as sv
import wwm_model as wm

V, PAD, CLS, SEP, MASK, IGNORE = 64, 0, 2, 3, 4, -1
# (tokens, s, '##' density; 'word': segment 0 is one word)
ROWS = [(5, 1, 0), (9, 1, .3), (64, 1, .3), (65, 1, 'word'), (128, 1, 0), (129, 1, .3), (512, 1, 'word'), (2048, 1, .3),
        (7, 1, .3), (131, 0, .3), (130, 1, .3)]

Case = collections.namedtuple('Case', 'front seed counter row n word P p src')


@functools.lru_cache(maxsize=None)
def segments():
  """per row of ROWS its two segments' ids (letters 5..30, their '##' forms 31..56); s = 0: segment 0 is empty"""
  rng = np.random.default_rng(5)
  segs = []
  for n, s, dens in ROWS:
    a = (n - 3) // 2 if s else 0
    seg = []
    for k, m in enumerate((a, n - 2 - s - a)):
      d = 1.0 if dens == 'word' and k == 0 else 0.3 if dens else 0.0
      seg.append(np.where(rng.random(m) < d, rng.integers(31, 57, m), rng.integers(5, 31, m)).tolist())
    segs.append(seg)
  return segs


@functools.lru_cache(maxsize=None)
def cont():
  """the '##' table of 'tiny64'"""
  return wm.cont_table(sv.vocab_bytes('tiny64').decode().split('\n')[:V])


def table_row(g):
  """row g of ROWS as a collate shows it: (ids, special), [n] each"""
  a, b = segments()[g]
  ids = [CLS] + a + ([SEP] if ROWS[g][1] else []) + b + [SEP]
  sp = np.isin(ids, (CLS, SEP))
  assert len(ids) == ROWS[g][0] and sp.sum() == 2 + ROWS[g][1]
  return np.asarray(ids, np.int64), sp.astype(np.int64)


def token_plane(n, gen, special):
  """(ids, special) [1, n] for lddl_mask_tokens: a '##' form at three columns in ten, special columns at the given
  density (0: none)"""
  rng = np.random.default_rng(gen)
  ids = np.where(rng.random((1, n)) < 0.3, rng.integers(31, 57, (1, n)), rng.integers(5, 31, (1, n)))
  sp = (rng.random((1, n)) < special).astype(np.int64) if special else np.zeros((1, n), np.int64)
  return ids, sp


def planes(case):
  """the unmasked batch of the case, padded to its row: rows 0 .. row - 1 are ROWS[0]"""
  if case.front == 'mask_tokens':
    assert case.row == 0
    ids, sp = token_plane(case.n, *case.src)
  else:
    assert ROWS[case.src][0] == case.n >= ROWS[0][0]
    ids, sp = np.full((case.row + 1, case.n), PAD, np.int64), np.ones((case.row + 1, case.n), np.int64)
    for r in range(case.row + 1):
      i, s = table_row(case.src if r == case.row else 0)
      ids[r, :len(i)], sp[r, :len(i)] = i, s
  assert ids.shape == sp.shape == (case.row + 1, case.n)
  return ids, sp


def units(case, ids=None, sp=None):
  """(keys ascending, weights, budget) of the case's row"""
  if ids is None:
    ids, sp = planes(case)
  sp = np.asarray(sp) != 0
  r = case.row
  head = wm.heads(ids, sp, cont())[r] if case.word else np.arange(case.n, dtype=np.int64)
  h0 = mm.draws(case.seed, case.counter, r, np.arange(case.n))[0]
  _, keys, w = bm.row_units(head, sp[r], h0)
  return keys, w, bm.budget(int((~sp[r]).sum()), case.p, case.P)


def trace(case):
  return bm.radix_steps(*units(case))


S63 = (1 << 63) + 12345  # the seed and counter of tests/test_mask_budget_gpu.py
C40 = 1 << 40
BIG = (1 << 20) - 1  # the longest row lddl_mask_tokens takes
# case -> the (exit level index, reason) it was committed for; `several`: the exit bin holds more than one head
CASES = [
    # lddl_mask_tokens, tokens
    (Case('mask_tokens', 11, 9, 0, 9, False, 20, 1.0, (3, 0.05)), 0, 'take_all'),
    (Case('mask_tokens', 11, 9, 0, 9, False, 1, 0.15, (3, 0.05)), 0, 'spent'),
    (Case('mask_tokens', 11, 9, 0, 2047, False, 80, 0.15, (3, 0.05)), 1, 'spent'),
    (Case('mask_tokens', S63, C40, 0, 65536, False, 4096, 0.15, (4, 0.05)), 2, 'spent'),  # test_one_row_of_65536_columns
    (Case('mask_tokens', 0, 9, 0, 8191, False, 464, 1.0, (0, 0)), 3, 'spent'),            # a pair sharing 27 bits
    (Case('mask_tokens', 59, 9, 0, 131071, False, 107779, 1.0, (3, 0)), 3, 'spent'),      # 29 bits, a third key in the bin
    (Case('mask_tokens', 0, 9, 0, 131071, False, 14776, 1.0, (0, 0)), 4, 'spent'),        # 33 bits
    (Case('mask_tokens', 2, 9, 0, BIG, False, 735786, 1.0, (2, 0)), 5, 'spent'),          # 44 bits
    (Case('mask_tokens', 773, 9, 0, BIG, False, 605961, 1.0, (3, 0)), 6, 'spent'),        # 48 bits
    # lddl_mask_tokens, whole words
    (Case('mask_tokens', 11, 9, 0, 9, True, 20, 1.0, (3, 0.05)), 0, 'take_all'),
    (Case('mask_tokens', 11, 9, 0, 9, True, 1, 0.15, (3, 0.05)), 0, 'one_head'),
    (Case('mask_tokens', 11, 9, 0, 2047, True, 300, 0.15, (3, 0.05)), 1, 'spent'),
    (Case('mask_tokens', S63, C40, 0, 65536, True, 4096, 0.15, (4, 0.05)), 2, 'spent'),   # test_one_row_of_65536_columns
    (Case('mask_tokens', 773, 9, 0, BIG, True, 605598, 1.0, (5, 0)), 6, 'one_head'),      # one of the word's two tokens fits
    (Case('mask_tokens', 773, 9, 0, BIG, True, 605597, 1.0, (5, 0)), 6, 'spent'),
    # a row table (mask_budget_kernel): ROWS[7], the longest row a collate takes, as batch row 1; a pair sharing 32 bits
    (Case('rows', 9502, 9, 1, 2048, False, 552, 1.0, 7), 4, 'spent'),
    (Case('rows', 9502, 9, 1, 2048, True, 559, 1.0, 7), 4, 'spent'),
]
SEVERAL = Case('mask_tokens', 59, 9, 0, 131071, False, 107779, 1.0, (3, 0))


def case_id(entry):
  c, level, reason = entry
  return '%s-%s-%d-L%d-%s' % (c.front, 'words' if c.word else 'tokens', c.n, level, reason) + ('-several' if c == SEVERAL else '')
