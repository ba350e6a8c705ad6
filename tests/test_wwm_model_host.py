"""tests/wwm_model.py, the numpy model of whole-word dynamic masking that the
GPU tests (test_wwm_gpu.py) compare bit for bit against: the word structure
on hand-written rows, its reduction to mask_model.mask when no token is a
continuation, one select per word, and the marginal selection rate."""
import numpy as np

import mask_model as mm
import wwm_model as wm

# ids: 0 [PAD] 1 [CLS] 2 [SEP] 3 [MASK]; 10..19 whole words; 20..29 '##' pieces
TOKENS = ['[PAD]', '[CLS]', '[SEP]', '[MASK]'] + ['x'] * 6 + ['w%d' % i for i in range(10)] + ['##p%d' % i for i in range(10)]
TABLE = wm.cont_table(TOKENS)
CLS, SEP, PAD = 1, 2, 0
DRAW = dict(seed=12345, counter=3, mask_id=3, n_random=len(TOKENS), ignore=-1)


def plane(rows):
  """lists of ids -> (ids, special) padded with [PAD]; [CLS], [SEP] and the padding are special"""
  S = max(len(r) for r in rows)
  ids = np.asarray([r + [PAD] * (S - len(r)) for r in rows], np.int64)
  return ids, np.isin(ids, (CLS, SEP, PAD)).astype(np.int64)


def test_cont_table_and_out_of_range_ids():
  assert TABLE.sum() == 10 and TABLE[20:].all() and not TABLE[:20].any()
  assert wm.cont([20, 19, -1, 30, 1 << 40, -(1 << 40)], TABLE).tolist() == [True, False, False, False, False, False]
  assert wm.cont_table([b'##a', b'#a', b'a##', b'##', b'#']).tolist() == [True, False, False, True, False]


def test_heads_on_hand_written_rows():
  rows = [
      [CLS, 10, 20, 21, 11, SEP, 12, 22, SEP],   # un ##a ##b w | w ##c
      [CLS, 20, 21, 10, SEP, 22, 23, 11, SEP],   # a leading '##' in A, a '##' right after [SEP]
      [CLS, 10, 20, 21, 22, 23, 24, 25, SEP],    # one word (single segment)
      [CLS, SEP, 20, SEP],                       # empty A, B of one '##' piece
      [CLS, 10, 20, SEP, 21, SEP],               # A's last word ends at [SEP]; B is one piece
  ]
  ids, sp = plane(rows)
  h = wm.heads(ids, sp, TABLE)
  st = wm.starts(ids, sp, TABLE)
  assert h[0].tolist() == [0, 1, 1, 1, 4, 5, 6, 6, 8]
  assert h[1].tolist() == [0, 1, 1, 3, 4, 5, 5, 7, 8]
  assert h[2].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 8]
  assert h[3].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8]  # specials and padding head themselves
  assert h[4].tolist() == [0, 1, 1, 3, 4, 5, 6, 7, 8]
  assert st[1].tolist() == [False, True, False, True, False, True, False, True, False]
  assert not st[sp != 0].any()
  # without any special column, column 0 starts a word whatever it holds
  ids1 = np.asarray([[20, 21, 10, 22]], np.int64)
  assert wm.heads(ids1, np.zeros_like(ids1), TABLE).tolist() == [[0, 0, 2, 2]]
  # the caller's special mask inside a word cuts it
  assert wm.heads(ids1, np.asarray([[0, 1, 0, 0]]), TABLE).tolist() == [[0, 1, 2, 2]]


def test_row_without_continuations_is_mask_model():
  rng = np.random.default_rng(5)
  ids = rng.integers(10, 20, size=(7, 130))
  ids[:, 0] = CLS
  ids[:, 60] = SEP
  ids[:, 129] = SEP
  sp = np.isin(ids, (CLS, SEP)).astype(np.int64)
  for p in (0.0, 0.15, 1.0):
    a = wm.mask(ids, sp, TABLE, p=p, **DRAW)
    b = mm.mask(ids, sp, p=p, **DRAW)
    for x, y in zip(a, b):
      assert np.array_equal(x, y)
  # and so is any row under a table without '##' entries
  ids2 = rng.integers(4, 30, size=(3, 70))
  a = wm.mask(ids2, np.zeros_like(ids2), np.zeros(30, bool), p=0.15, **DRAW)
  b = mm.mask(ids2, np.zeros_like(ids2), p=0.15, **DRAW)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_columns_of_a_word_share_select_and_keep_their_own_replacement_draws():
  rng = np.random.default_rng(9)
  n, S = 64, 96
  ids = np.where(rng.random((n, S)) < 0.6, rng.integers(20, 30, (n, S)), rng.integers(10, 20, (n, S)))
  ids[:, 0], ids[:, 40], ids[:, S - 1] = CLS, SEP, SEP
  sp = np.isin(ids, (CLS, SEP)).astype(np.int64)
  m = wm.mask(ids, sp, TABLE, p=0.3, **DRAW)
  h = wm.heads(ids, sp, TABLE)
  r = np.arange(n)[:, None]
  assert np.array_equal(m.select[sp == 0], m.select[r, h][sp == 0])
  assert not m.select[sp != 0].any()
  # the select draw of a head is the per-token one; the 80/10/10 planes of selected columns are the per-token draws
  t = mm.mask(ids, np.zeros_like(sp), p=1.0, **DRAW)
  heads_only = (h == np.arange(S)[None, :]) & (sp == 0)
  assert np.array_equal(m.select[heads_only], mm.mask(ids, sp, p=0.3, **DRAW).select[heads_only])
  assert np.array_equal(m.masked, m.select & t.masked) and np.array_equal(m.random, m.select & t.random)
  assert np.array_equal(m.labels, np.where(m.select, ids, -1))
  assert np.array_equal(m.input_ids[~m.select], ids[~m.select])
  assert m.select.any() and (m.select & (h != np.arange(S)[None, :])).any()


def test_marginal_selection_rate_is_p():
  """>= 10^5 single-piece and >= 10^5 three-piece words at p = 0.15: the
  selected share of tokens is within 4 standard deviations of p.  Tokens of a
  word are selected together, so the deviation is that of the words: with W1
  single-piece and W3 three-piece words, var(selected tokens) = p (1 - p) (W1
  + 9 W3)."""
  p, n, S = 0.15, 1024, 1 + 4 * 110
  row = [CLS] + [10, 11, 21, 22] * 110  # w | w ##p ##p, 110 times: 110 words of each kind per row
  ids = np.tile(np.asarray(row, np.int64), (n, 1))
  sp = (ids == CLS).astype(np.int64)
  m = wm.mask(ids, sp, TABLE, p=p, **DRAW)
  w1 = w3 = n * 110
  assert w1 >= 10 ** 5
  tokens = w1 + 3 * w3
  sd = np.sqrt(p * (1 - p) * (w1 + 9 * w3)) / tokens
  share = m.select.sum() / tokens
  assert abs(share - p) < 4 * sd, (share, sd)
  # each kind on its own, too
  one = m.select[:, 1::4]
  three = m.select[:, 2::4]
  assert abs(one.mean() - p) < 4 * np.sqrt(p * (1 - p) / w1)
  assert abs(three.mean() - p) < 4 * np.sqrt(p * (1 - p) / w3)
  assert np.array_equal(three, m.select[:, 3::4]) and np.array_equal(three, m.select[:, 4::4])
