"""tests/mask_model.py is right, and the draw it models is sound: no GPU.

The GPU tests (tests/test_mask_draws_gpu.py) hold every dynamic-masking route
to the model bit for bit, so what is asked of the draw itself -- rates,
independence across columns, rows and batches, the range of the random words
-- is asked here of the model, where it runs on every checkout.

1. The model against things that are not the model: splitmix64's published
   vector, and a second implementation in Python ints masked to 64 bits,
   element by element on the edges of every input: seeds and counters with
   bit 63 and bit 32 set (a half lost on the way in), rows at 4095 / 4096
   (row << 20 passes 2^32), 2^31 and 2^43 (row << 20 reaches bit 63), columns
   at both ends of the 20 bits the index gives them.
2. The distribution.  The runs are deterministic: the bounds are conditions,
   the values in the docstrings are what this model gives.
"""
import functools

import numpy as np

import mask_model as mm

M64 = (1 << 64) - 1
SEEDS = [0, 1, 12345, 1 << 63, M64]
COUNTERS = [0, 1, 1 << 32, M64]
ROWS = [0, 1, 4095, 4096, 1 << 31, 1 << 43]
COLS = [0, 1, 63, 64, 2047, (1 << 20) - 1]


# ---- 1. the model against things that are not the model --------------------------
def sm_int(x):
  x = (x + 0x9E3779B97F4A7C15) & M64
  x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
  x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
  return x ^ (x >> 31)


def int_below(x, p):
  """unit(h) < p for x = h >> 11, without a double: x / 2^53 against p's own integer ratio"""
  num, den = float(p).as_integer_ratio()
  return x * den < num * (1 << 53)


def twin(tok, special, row, col, seed, counter, p, mask_id, n_random, ignore):
  """(input id, label, the three hashes) of one column, in Python ints"""
  k = sm_int(seed ^ sm_int(counter))
  i = ((((row << 20) & M64) | col) * 3) & M64
  h = [sm_int((k + i + j) & M64) for j in range(3)]
  if special or not int_below(h[0] >> 11, p):
    return tok, ignore, h
  if int_below(h[1] >> 11, 0.8):
    return mask_id, tok, h
  if int_below(h[2] >> 11, 0.5):
    return ((h[2] & 0xFFFFFFFF) * n_random) >> 32, tok, h
  return tok, tok, h


def test_splitmix64_published_vector():
  """Vigna's splitmix64.c seeded with 1234567: the state advances by the golden
  gamma per call, so the n-th output is sm(seed + (n - 1) * gamma)"""
  assert int(mm.sm(1234567)[0]) == 6457827717110365317
  assert int(mm.sm(1234567 + 0x9E3779B97F4A7C15)[0]) == 3203168211198807973
  assert int(mm.sm(0)[0]) == 16294208416658607535
  assert sm_int(1234567) == 6457827717110365317 and sm_int(0) == 16294208416658607535
  # wraps: the largest input, as an array and as a Python int
  assert int(mm.sm(M64)[0]) == sm_int(M64) == int(mm.sm(np.asarray([M64], np.uint64))[0])


def test_unit_is_exact():
  h = np.asarray([0, 2047, 2048, 1 << 63, M64 - 2047, M64], np.uint64)
  assert mm.unit(h).tolist() == [0.0, 0.0, 2.0 ** -53, 0.5, 1 - 2.0 ** -53, 1 - 2.0 ** -53]
  assert mm.unit(M64)[0] < 1.0


def test_threshold_08_as_integers():
  """the pure-int twin compares h >> 11 with 0.8 as a double: the double 0.8
  is 3602879701896397 / 2^52, just above 4/5"""
  num, den = (0.8).as_integer_ratio()
  assert den == 1 << 52 and num == 3602879701896397 and num * 5 > 4 * den
  t = 2 * num  # unit(h) < 0.8  <=>  h >> 11 < 0.8 * 2^53 = 2 * num
  for x in (t - 1, t, t + 1):
    assert (x * 2.0 ** -53 < 0.8) == (x < t)


def test_numpy_model_equals_pure_int_twin():
  """every seed x counter x row x col of the edge sets, element by element:
  the hashes, and the outcome at p = 0.5 (so that all four outcomes occur)
  and at the vocabulary sizes 30522, 5 and 2^31 - 1"""
  rows, cols = np.asarray(ROWS, np.uint64), np.asarray(COLS, np.uint64)
  shape = (len(ROWS), len(COLS))
  ids = (np.arange(len(ROWS) * len(COLS), dtype=np.int64).reshape(shape) * 977 + (1 << 40))
  special = np.zeros(shape, np.int64)
  special[0, 0] = special[2, 3] = 1
  seen = set()
  for seed in SEEDS:
    for counter in COUNTERS:
      h = mm.draws(seed, counter, rows[:, None], cols[None, :])
      assert h.shape == (3,) + shape and h.dtype == np.uint64
      for n_random in (30522, 5, (1 << 31) - 1):
        m = mm.mask(ids, special, seed, counter, 0.5, 103, n_random, -100, rows=rows[:, None], cols=cols[None, :])
        for a, row in enumerate(ROWS):
          for b, col in enumerate(COLS):
            tok, lab, hh = twin(int(ids[a, b]), bool(special[a, b]), row, col, seed, counter, 0.5, 103, n_random, -100)
            assert [int(x) for x in h[:, a, b]] == hh, (seed, counter, row, col)
            assert (int(m.input_ids[a, b]), int(m.labels[a, b])) == (tok, lab), (seed, counter, row, col, n_random)
            seen.add('keep' if lab == -100 else 'mask' if tok == 103 else 'same' if tok == lab else 'word')
  assert seen == {'keep', 'mask', 'same', 'word'}


def test_every_input_reaches_the_hash():
  """what the pooled rates cannot see: the hashes of the edge sets are all
  different, so no seed half, counter, row bit or column is dropped, and the
  three draws of a column are not the next column's"""
  rows, cols = np.asarray(ROWS, np.uint64), np.asarray(COLS, np.uint64)
  allh = [mm.draws(s, c, rows[:, None], cols[None, :]).reshape(-1) for s in SEEDS for c in COUNTERS]
  allh = np.concatenate(allh)
  assert len(np.unique(allh)) == allh.size == 3 * len(SEEDS) * len(COUNTERS) * len(ROWS) * len(COLS)
  # a column's hashes are those of index 3 * col .. 3 * col + 2 on one key: consecutive columns chain, never overlap
  h = mm.draws(12345, 7, np.zeros(1, np.uint64), np.arange(4, dtype=np.uint64))
  k = mm.sm(mm.u64(12345) ^ mm.sm(7))
  assert np.array_equal(h.T.reshape(-1), mm.sm(k + np.arange(12, dtype=np.uint64)))


# ---- 2. the distribution ---------------------------------------------------------
P, R, C, NC, V = 0.15, 256, 512, 64, 30522


def z(k, n, q):
  return (k - n * q) / np.sqrt(n * q * (1 - q))


@functools.lru_cache(maxsize=None)
def planes():
  """seed 12345, counters 0 .. 63, 256 x 512 columns, none special: the select
  planes [64, 256, 512], the counts of [MASK] and random-word columns, the random words"""
  ids, sp = np.full((R, C), 7, np.int64), np.zeros((R, C), np.int64)
  sel = np.zeros((NC, R, C), bool)
  n_mask = n_word = 0
  words = []
  for c in range(NC):
    m = mm.mask(ids, sp, 12345, c, P, 103, V, -1)
    sel[c] = m.select
    assert not (m.masked & m.random).any() and not ((m.masked | m.random) & ~m.select).any()
    n_mask += int(m.masked.sum())
    n_word += int(m.random.sum())
    words.append(m.input_ids[m.random])
  return sel, n_mask, n_word, np.concatenate(words)


def test_rates():
  """overall select rate: |z| <= 5 (measured 2.52: 1 260 902 of 8 388 608).
  [MASK] and random-word shares of the selected columns within 5 sigma of 0.8
  and 0.1 (0.79964 and 0.10015; sigma 0.00036 and 0.00027)"""
  sel, n_mask, n_word, _ = planes()
  ns = int(sel.sum())
  assert abs(z(ns, sel.size, P)) <= 5
  assert abs(n_mask / ns - 0.8) <= 5 * np.sqrt(0.8 * 0.2 / ns)
  assert abs(n_word / ns - 0.1) <= 5 * np.sqrt(0.1 * 0.9 / ns)


def test_rate_per_column_and_per_row():
  """select rate of each column over rows x counters and of each row over
  columns x counters: max |z| <= 5 each (3.31, 3.32).  A column or a row that
  did not reach the index would make whole lines of the plane all or nothing"""
  sel = planes()[0]
  assert np.abs(z(sel.sum((0, 1)), NC * R, P)).max() <= 5
  assert np.abs(z(sel.sum((0, 2)), NC * C, P)).max() <= 5


def test_consecutive_counters_and_adjacent_columns_are_independent():
  """both selected at one (row, col) in consecutive counters, and in adjacent
  columns of one row: |z| <= 5 around p^2 (1.35, 2.49).  A counter that did
  not reach the key gives z in the thousands; hashes shared between
  neighbouring columns correlate the second"""
  sel = planes()[0]
  both = sel[1:] & sel[:-1]
  assert abs(z(int(both.sum()), both.size, P * P)) <= 5
  adj = sel[:, :, 1:] & sel[:, :, :-1]
  assert abs(z(int(adj.sum()), adj.size, P * P)) <= 5


def test_random_words_are_uniform_and_reach_both_ends():
  """the 126 281 random words in 64 equal buckets of [0, 30522): chi^2 over 63
  degrees of freedom <= 120 (57.4); minimum 0 and maximum 30521, both reached"""
  words = planes()[3]
  expect = np.bincount(np.arange(V) * 64 // V, minlength=64) * (len(words) / V)
  got = np.bincount(words * 64 // V, minlength=64)
  assert ((got - expect) ** 2 / expect).sum() <= 120
  assert words.min() == 0 and words.max() == V - 1


def test_five_random_words():
  """n_random = 5 at p = 1 on one 256 x 512 plane (counter 0): every word in
  [0, 5), each value between 2 400 and 2 800 times (2 565 .. 2 689)"""
  m = mm.mask(np.full((R, C), 7, np.int64), np.zeros((R, C), np.int64), 12345, 0, 1.0, 103, 5, -1)
  words = m.input_ids[m.random]
  assert words.min() >= 0 and words.max() < 5
  count = np.bincount(words, minlength=5)
  assert count.min() >= 2400 and count.max() <= 2800, count


def test_top_word_is_reachable_at_every_size():
  """the largest low word gives n_random - 1 and never n_random, at the sizes
  the GPU tests use and at int32's end"""
  for n in (5, 6, 64, 65, 30522, 52000, 65536, (1 << 31) - 1):
    assert (0xFFFFFFFF * n) >> 32 == n - 1
    assert (((1 << 32) - (1 << 32) // n) * n) >> 32 == n - 1  # a whole band of low words, not one value


def test_probability_edges():
  """p = 0 selects nothing, p = 1 every non-special column, and p = 2^-53
  exactly the columns whose first hash is below 2^11 (unit() = 0)"""
  ids = np.arange(R * C, dtype=np.int64).reshape(R, C)
  sp = (np.arange(R * C).reshape(R, C) % 7 == 0).astype(np.int64) * np.asarray([1, 2, -1, 1 << 32])[np.arange(C) % 4]
  for counter in (0, 5):
    none = mm.mask(ids, sp, 12345, counter, 0.0, 103, V, -1)
    assert not none.select.any() and np.array_equal(none.input_ids, ids) and (none.labels == -1).all()
    full = mm.mask(ids, sp, 12345, counter, 1.0, 103, V, -1)
    assert np.array_equal(full.select, sp == 0) and np.array_equal(full.labels[sp != 0], np.full((sp != 0).sum(), -1))
    assert np.array_equal(full.labels[sp == 0], ids[sp == 0])
    tiny = mm.mask(ids, sp, 12345, counter, 2.0 ** -53, 103, V, -1)
    h0 = mm.draws(12345, counter, np.arange(R)[:, None], np.arange(C)[None, :])[0]
    assert np.array_equal(tiny.select, (sp == 0) & (h0 < np.uint64(1 << 11)))
  # on hashes made by hand, since no plane this small holds one below 2^11
  h = np.asarray([0, 1, 2047, 2048, 4095, 4096, 1 << 63, M64], np.uint64)
  assert np.array_equal(mm.unit(h) < 2.0 ** -53, h < np.uint64(1 << 11))
  assert (mm.unit(h) < 1.0).all() and not (mm.unit(h) < 0.0).any()
  assert np.array_equal(mm.unit(h) < 1 - 2.0 ** -53, (h >> np.uint64(11)) < np.uint64((1 << 53) - 1))
