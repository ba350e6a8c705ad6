"""Exact-count dynamic masking (lddl_set_mask_budget, include/lddl_amd.h) in
numpy and Python ints, over tests/mask_model.py and tests/wwm_model.py: per
row, the units in ascending rank key, taken while their weights fit the
budget.  Plain helper module.  ids and special are [n, S] planes, as in
wwm_model; mask returns mask_model.Masked; table None: tokens, not words.

  select_loop     the plain definition: a dict of units per row, sorted, taken one by one
  select_sorted   the same by argsort and cumsum (a row of 2^20 - 1 columns in well under a second)
  mask            the model every GPU result is judged against (select_sorted; loop=True: select_loop)
  radix_steps / radix_trace   a replay of mask_budget.hip's radix select, only to classify cases
"""
import numpy as np

import mask_model as mm
import wwm_model as wm


def budget(c, p, max_predictions):
  return min(max_predictions, c, max(1, round(c * p))) if c else 0  # (round: half to even, on the double product)


def select_loop(head, sp, h0, p, max_predictions):
  """the plain definition: per row a dict of units, sorted by key, taken while they fit"""
  select = np.zeros(sp.shape, bool)
  for r in range(sp.shape[0]):
    left = budget(int((~sp[r]).sum()), p, max_predictions)
    units = {}  # head column -> weight
    for j in np.flatnonzero(~sp[r]):
      units[int(head[r, j])] = units.get(int(head[r, j]), 0) + 1
    key = {u: (int(h0[r, u]) & ~0xFFFFF) | u for u in units}
    taken = []
    for u in sorted(units, key=key.get):
      if units[u] > left:
        break
      left -= units[u]
      taken.append(u)
    select[r] = ~sp[r] & np.isin(head[r], taken)
  return select


def row_units(head_r, sp_r, h0_r):
  """one row's units in ascending key: (head columns, keys, weights)"""
  u, w = np.unique(head_r[~sp_r], return_counts=True)
  key = (h0_r[u] & ~np.uint64(0xFFFFF)) | u.astype(np.uint64)
  order = np.argsort(key, kind='stable')
  return u[order], key[order], w[order].astype(np.int64)


def select_sorted(head, sp, h0, p, max_predictions):
  """select_loop in numpy: per row an argsort of the unit keys and a cumsum of the weights; the units in front of
  the first one that does not fit are those whose cumulative weight is within the budget (weights are >= 1)"""
  select = np.zeros(sp.shape, bool)
  for r in range(sp.shape[0]):
    u, _, w = row_units(head[r], sp[r], h0[r])
    taken = np.zeros(sp.shape[1], bool)
    taken[u[np.cumsum(w) <= budget(int((~sp[r]).sum()), p, max_predictions)]] = True
    select[r] = ~sp[r] & taken[head[r]]
  return select


def mask(ids, special, table, seed, counter, p, max_predictions, mask_id, n_random, ignore, rows=None, loop=False):
  """loop: select_loop in place of select_sorted (tests/test_budget_model_host.py holds the two equal)"""
  ids = np.asarray(ids, np.int64)
  sp = np.asarray(special) != 0
  n, S = ids.shape
  rows = np.arange(n) if rows is None else np.asarray(rows)
  cols = np.arange(S, dtype=np.int64)
  head = np.broadcast_to(cols, (n, S)) if table is None else wm.heads(ids, sp, table)
  h = mm.draws(seed, counter, rows[:, None], cols[None, :])
  select = (select_loop if loop else select_sorted)(head, sp, h[0], p, max_predictions)
  masked = select & (mm.unit(h[1]) < 0.8)
  random = select & ~masked & (mm.unit(h[2]) < 0.5)
  word = (((h[2] & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)
  out = np.where(masked, np.int64(mask_id), np.where(random, word, ids))
  return mm.Masked(out, np.where(select, ids, np.int64(ignore)), select, masked, random)


# ---- the radix select of mask_budget.hip, replayed --------------------------------
# Only to say which levels and exits of budget_threshold a case reaches
# (tests/budget_cases.py, tests/test_budget_model_host.py); no GPU result is
# judged against it.
TAKE_ALL = (1 << 64) - 1


def radix_steps(keys, weights, budget):
  """budget_threshold level by level over one row's units (keys: unique uint64, weights >= 1, in any order; budget:
  the row's, budget(c, p, P)): a list of dicts (level, bin, before, left, heads, weight), the last one with thr and
  reason.  256 bins per level over the keys that carry the prefix found so far; the first bin whose running weight
  passes `left`.  reason: 'take_all' (no such bin), 'spent' (before == left: nothing is left for the bin, whatever
  it holds), 'one_head' (the bin holds one unit and before < left: a word of which only a part would fit)."""
  keys = np.asarray(keys, np.uint64)
  weights = np.asarray(weights, np.int64)
  assert keys.shape == weights.shape and keys.ndim == 1 and len(np.unique(keys)) == len(keys)
  prefix, left, steps = 0, int(budget), []
  for level in range(8):
    shift = 56 - 8 * level
    under = np.ones(len(keys), bool) if level == 0 else (keys >> np.uint64(shift + 8)) == np.uint64(prefix)
    digit = ((keys[under] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
    wt = np.bincount(digit, weights[under], 256).astype(np.int64)
    hd = np.bincount(digit, minlength=256)
    run = np.cumsum(wt)
    step = dict(level=level, left=left)
    steps.append(step)
    if not (run > left).any():
      assert level == 0  # below it the bin's weight is known to pass
      step.update(thr=TAKE_ALL, reason='take_all')
      return steps
    b = int(np.argmax(run > left))
    before = int(run[b] - wt[b])
    prefix = prefix << 8 | b
    step.update(bin=b, before=before, heads=int(hd[b]), weight=int(wt[b]))
    if hd[b] == 1 or before == left:
      step.update(thr=prefix << shift, reason='spent' if before == left else 'one_head')
      return steps
    left -= before
  raise AssertionError('unique keys: a bin of the last level holds one head')


def radix_trace(keys, weights, budget):
  """-> (thr, exit_level, reason) of radix_steps"""
  last = radix_steps(keys, weights, budget)[-1]
  return last['thr'], last['level'], last['reason']
