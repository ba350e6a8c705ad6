"""Whole-word dynamic masking (lddl_set_whole_word_mask, defined in
include/lddl_amd.h) in numpy, over tests/mask_model.py: the word structure of
a row from its unmasked ids, and mask_model's draws with the select draw taken
at the head column of each token's word.  Plain helper module: no tests, no
fixtures.

  cont_table(tokens)              bool [V]: entry id begins with '##'
  cont(ids, table)                table[id] for 0 <= id < V, False elsewhere
  starts(ids, special, table)     bool plane: a word starts at the column
  heads(ids, special, table)      int64 plane: the head column of every column
                                  (a special column: itself)
  mask(ids, special, table, ...)  mask_model.Masked, as mask_model.mask

ids and special are [n, S] planes, the padding of a padded batch being special
columns; a token of the padding-free stream is its row's column of that plane.
"""
import numpy as np

import mask_model as mm


def cont_table(tokens):
  return np.asarray([(t.encode() if isinstance(t, str) else bytes(t))[:2] == b'##' for t in tokens], bool)


def cont(ids, table):
  ids = np.asarray(ids, np.int64)
  inside = (ids >= 0) & (ids < len(table))
  return inside & np.asarray(table, bool)[np.where(inside, ids, 0)]


def starts(ids, special, table):
  ids = np.asarray(ids, np.int64)
  sp = np.asarray(special) != 0
  assert ids.ndim == 2 and sp.shape == ids.shape
  first = np.ones_like(sp)  # j == 0, or the column to the left is special
  first[:, 1:] = sp[:, :-1]
  return ~sp & (first | ~cont(ids, table))


def heads(ids, special, table):
  st = starts(ids, special, table)
  col = np.broadcast_to(np.arange(st.shape[1], dtype=np.int64)[None, :], st.shape)
  h = np.maximum.accumulate(np.where(st, col, -1), axis=1)
  sp = np.asarray(special) != 0
  assert (h[~sp] >= 0).all()  # every non-special column has a head
  return np.where(sp, col, h)


def mask(ids, special, table, seed, counter, p, mask_id, n_random, ignore, rows=None):
  """mask_model.mask with whole words selected: rows default to the plane's
  own row numbers, the columns are the plane's"""
  ids = np.asarray(ids, np.int64)
  n, S = ids.shape
  rows = (np.arange(n) if rows is None else np.asarray(rows))[:, None]
  cols = np.arange(S)[None, :]
  h = np.broadcast_to(mm.draws(seed, counter, rows, cols), (3, n, S))
  h0 = mm.draws(seed, counter, rows, heads(ids, special, table))[0]
  select = (np.asarray(special) == 0) & (mm.unit(h0) < p)
  masked = select & (mm.unit(h[1]) < 0.8)
  random = select & ~masked & (mm.unit(h[2]) < 0.5)
  word = (((h[2] & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)
  out = np.where(masked, np.int64(mask_id), np.where(random, word, ids))
  return mm.Masked(out, np.where(select, ids, np.int64(ignore)), select, masked, random)
