"""Exact-count dynamic masking (lddl_set_mask_budget, include/lddl_amd.h) in
numpy and Python ints, over tests/mask_model.py and tests/wwm_model.py: per
row, the units in ascending rank key, taken while their weights fit the
budget.  Plain helper module.  ids and special are [n, S] planes, as in
wwm_model; mask returns mask_model.Masked; table None: tokens, not words.
"""
import numpy as np

import mask_model as mm
import wwm_model as wm


def budget(c, p, max_predictions):
  return min(max_predictions, c, max(1, round(c * p))) if c else 0  # (round: half to even, on the double product)


def mask(ids, special, table, seed, counter, p, max_predictions, mask_id, n_random, ignore, rows=None):
  ids = np.asarray(ids, np.int64)
  sp = np.asarray(special) != 0
  n, S = ids.shape
  rows = np.arange(n) if rows is None else np.asarray(rows)
  cols = np.arange(S, dtype=np.int64)
  head = np.broadcast_to(cols, (n, S)) if table is None else wm.heads(ids, sp, table)
  h = mm.draws(seed, counter, rows[:, None], cols[None, :])
  select = np.zeros((n, S), bool)
  for r in range(n):
    left = budget(int((~sp[r]).sum()), p, max_predictions)
    units = {}  # head column -> weight
    for j in np.flatnonzero(~sp[r]):
      units[int(head[r, j])] = units.get(int(head[r, j]), 0) + 1
    key = {u: (int(h[0, r, u]) & ~0xFFFFF) | u for u in units}
    taken = []
    for u in sorted(units, key=key.get):
      if units[u] > left:
        break
      left -= units[u]
      taken.append(u)
    select[r] = ~sp[r] & np.isin(head[r], taken)
  masked = select & (mm.unit(h[1]) < 0.8)
  random = select & ~masked & (mm.unit(h[2]) < 0.5)
  word = (((h[2] & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)
  out = np.where(masked, np.int64(mask_id), np.where(random, word, ids))
  return mm.Masked(out, np.where(select, ids, np.int64(ignore)), select, masked, random)
