"""The dynamic 80/10/10 masking of lddl_mask_tokens and of every mode-2
collate, in numpy: `_mask_tokens` (lddl/torch/bert.py:156-196) with the
counter-based draw that include/lddl_amd.h documents in place of torch's
generator.  Plain helper module: no tests, no fixtures.

Everything is uint64 arithmetic that wraps, and doubles that are exact
((h >> 11) * 2^-53 has 53 significant bits), so the GPU has to give these
values bit for bit; tests/test_mask_model_host.py pins the model itself
(published splitmix64 vector, a pure-int twin, the distribution).

  sm(x)                              splitmix64's output function
  unit(h)                            (h >> 11) * 2^-53, in [0, 1)
  draws(seed, counter, rows, cols)   the three hashes of every (row, col)
  mask(ids, special, seed, ...)      (input_ids, labels, select, masked, random)

rows is the row of the batch, whatever table row it shows, and cols the
column of the padded row (the position within its row of a token of the
padding-free stream): what all four kernels pass.
"""
import collections

import numpy as np

_GOLDEN, _MUL1, _MUL2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)

Masked = collections.namedtuple('Masked', 'input_ids labels select masked random')


def u64(x):
  """ints (Python ints up to 2^64 - 1 included) or an integer array -> a uint64 array of at least one dimension"""
  if isinstance(x, (int, np.integer)):
    return np.atleast_1d(np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF))
  x = np.asarray(x)
  if x.dtype == object:
    return np.asarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in x.reshape(-1)], np.uint64).reshape(x.shape)
  return np.atleast_1d(x.astype(np.uint64))


def sm(x):
  x = u64(x)
  with np.errstate(over='ignore'):
    x = x + _GOLDEN
    x = (x ^ (x >> np.uint64(30))) * _MUL1
    x = (x ^ (x >> np.uint64(27))) * _MUL2
  return x ^ (x >> np.uint64(31))


def unit(h):
  return (u64(h) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draws(seed, counter, rows, cols):
  """[3, ...] uint64: the select, [MASK] and random-word hashes of every
  (row, col); rows and cols broadcast against each other (a plane is
  rows[:, None], cols[None, :])"""
  k = sm(u64(seed) ^ sm(counter))
  with np.errstate(over='ignore'):
    i = ((u64(rows) << np.uint64(20)) | u64(cols)) * np.uint64(3)
    return np.stack([sm(k + i + np.uint64(j)) for j in range(3)])


def mask(ids, special, seed, counter, p, mask_id, n_random, ignore, rows=None, cols=None):
  """ids, special: int64 arrays of one shape, [n, S] unless rows / cols say
  otherwise (default: the plane's own row and column numbers; they broadcast
  to ids' shape).  special != 0 is never selected.  Returns int64 input_ids
  and labels, and the boolean select / [MASK] / random-word planes."""
  ids = np.asarray(ids, np.int64)
  if rows is None:
    assert ids.ndim == 2 and cols is None
    rows, cols = np.arange(ids.shape[0])[:, None], np.arange(ids.shape[1])[None, :]
  h = np.broadcast_to(draws(seed, counter, rows, cols), (3,) + ids.shape)
  select = (np.asarray(special) == 0) & (unit(h[0]) < p)
  masked = select & (unit(h[1]) < 0.8)
  random = select & ~masked & (unit(h[2]) < 0.5)
  word = (((h[2] & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)
  out = np.where(masked, np.int64(mask_id), np.where(random, word, ids))
  return Masked(out, np.where(select, ids, np.int64(ignore)), select, masked, random)
