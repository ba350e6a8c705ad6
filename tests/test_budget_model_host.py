"""The host side of the exact-count masking tests, without a GPU: the
vectorised model of tests/budget_model.py against its plain loop, the replica
of mask_budget.hip's radix select against the sort model, and the committed
cases of tests/budget_cases.py against what they were committed for, with the
coverage the GPU suite claims (lists it).

Exit level index 7 (two keys of one row sharing 56 bits: about 2^-17 per seed
at 2^20 - 1 columns) is not reached by any case and is not required here."""
import numpy as np
import pytest

import budget_cases as bc
import budget_model as bm
import mask_model as mm
import wwm_model as wm


def batch(gs):
  """rows gs of bc.ROWS as one padded batch: (ids, special)"""
  rows = [bc.table_row(g) for g in gs]
  S = max(len(i) for i, _ in rows)
  ids, sp = np.zeros((len(gs), S), np.int64), np.ones((len(gs), S), np.int64)
  for r, (i, s) in enumerate(rows):
    ids[r, :len(i)], sp[r, :len(i)] = i, s
  return ids, sp


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
def test_vectorised_model_is_the_loop(wwm):
  ids, sp = batch(range(len(bc.ROWS)))
  table = bc.cont() if wwm else None
  for p in (0.0, 0.15, 0.5, 1.0):
    for P in (1, 20, 80, 4096):
      a = bm.mask(ids, sp, table, bc.S63, bc.C40, p, P, bc.MASK, bc.V, bc.IGNORE)
      b = bm.mask(ids, sp, table, bc.S63, bc.C40, p, P, bc.MASK, bc.V, bc.IGNORE, loop=True)
      assert all(np.array_equal(x, y) for x, y in zip(a, b)), (p, P)
      count, cand = a.select.sum(1), (sp == 0).sum(1)
      want = [bm.budget(int(c), p, P) for c in cand]
      assert (count <= want).all() and (wwm or count.tolist() == want)
  assert a.select.any() and not a.select.all()


def test_vectorised_model_other_rows_and_an_empty_row():
  """batch rows that are not the plane's own numbers, and a row without candidates"""
  ids, sp = batch([1, 3, 9])
  sp[1] = 1
  for table in (None, bc.cont()):
    a = bm.mask(ids, sp, table, 7, 3, 0.5, 20, bc.MASK, bc.V, bc.IGNORE, rows=[5, 0, 1 << 30])
    b = bm.mask(ids, sp, table, 7, 3, 0.5, 20, bc.MASK, bc.V, bc.IGNORE, rows=[5, 0, 1 << 30], loop=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not a.select[1].any() and a.select[0].any()


def sort_prefix(keys, weights, budget):
  """the sort model over bare units: how many of them, in ascending key, are taken"""
  order = np.argsort(keys)
  return order, int((np.cumsum(weights[order]) <= budget).sum())


@pytest.mark.parametrize('spread', [64, 44, 20, 9, 3], ids=lambda s: '%d-bit' % s)
def test_replica_selects_the_models_prefix(spread):
  """random rows; the 44 hash bits of the keys drawn from 2^spread values (64: the whole word), so that the
  search has to go deep; unique by their low 20 bits, as the kernel's are"""
  rng = np.random.default_rng(spread)
  levels, reasons = set(), set()
  for trial in range(120):
    n = int(rng.integers(1, 400))
    if spread == 64:
      hi = (rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1)) & ~np.uint64(0xFFFFF)
    else:
      hi = rng.integers(0, 1 << spread, n, dtype=np.uint64) << np.uint64(20)
    keys = hi | rng.permutation(1 << 12)[:n].astype(np.uint64)
    weights = rng.integers(1, 5, n) if trial % 2 else np.ones(n, np.int64)
    total = int(weights.sum())
    for budget in {0, 1, int(rng.integers(0, total + 1)), total - 1, total}:
      thr, level, reason = bm.radix_trace(keys, weights, budget)
      order, taken = sort_prefix(keys, weights, budget)
      assert np.array_equal(keys < np.uint64(thr), np.isin(np.arange(n), order[:taken])), (trial, budget)
      assert (reason == 'take_all') == (taken == n) == (thr == bm.TAKE_ALL)
      if taken < n:
        spent = int(weights[order[:taken]].sum())
        assert (reason == 'spent') == (spent == budget) and (thr >> (56 - 8 * level)) == (int(keys[order[taken]]) >> (56 - 8 * level))
      levels.add(level)
      reasons.add(reason)
  assert reasons == {'take_all', 'one_head', 'spent'}
  assert max(levels) >= {64: 0, 44: 0, 20: 3, 9: 6, 3: 7}[spread]  # (few values: equal high digits, a deep search)


def test_replica_keys_of_a_real_row():
  """the kernel's own keys: ROWS[7] in both modes at every budget from 0 to all"""
  ids, sp = batch([7])
  h0 = mm.draws(3, 4, 0, np.arange(ids.shape[1]))[0]
  for table in (None, bc.cont()):
    head = np.arange(ids.shape[1]) if table is None else wm.heads(ids, sp != 0, table)[0]
    _, keys, w = bm.row_units(head, sp[0] != 0, h0)
    for budget in range(0, int(w.sum()) + 1, 97):
      thr, _, _ = bm.radix_trace(keys, w, budget)
      assert int((keys < np.uint64(thr)).sum()) == int((np.cumsum(w) <= budget).sum())


TRACES = {}


def steps_of(case):
  if case not in TRACES:
    TRACES[case] = bm.radix_steps(*bc.units(case))
  return TRACES[case]


@pytest.mark.parametrize('entry', bc.CASES, ids=bc.case_id)
def test_case_exits_where_it_was_committed_for(entry):
  case, level, reason = entry
  last = steps_of(case)[-1]
  assert (last['level'], last['reason']) == (level, reason)
  keys, w, budget = bc.units(case)
  assert int((keys < np.uint64(last['thr'])).sum()) == int((np.cumsum(w) <= budget).sum())  # the replica, on this row
  if case == bc.SEVERAL:
    assert last['heads'] > 1
  if reason == 'one_head':
    assert last['heads'] == 1 and last['before'] < last['left'] < last['before'] + last['weight']


def test_cases_cover_what_the_suite_claims():
  ids = [bc.case_id(e) for e in bc.CASES]
  assert len(set(ids)) == len(ids)
  hit = {}
  for case, level, reason in bc.CASES:
    last = steps_of(case)[-1]
    hit.setdefault((case.front, case.word), []).append((last['level'], last['reason'], last.get('heads', 0)))
  tok, word = hit['mask_tokens', False], hit['mask_tokens', True]
  assert {l for l, _, _ in tok} >= set(range(7))
  deepest = max(l for l, _, _ in word)
  assert deepest >= 3 and {l for l, _, _ in word} >= {0, 1, 2, deepest}
  assert {r for _, r, _ in tok + word} == {'take_all', 'one_head', 'spent'}
  assert any(r == 'one_head' and l >= 3 for l, r, _ in tok + word)  # (one_head is before < left: radix_steps)
  assert any(r == 'spent' and l >= 3 and h > 1 for l, r, h in tok + word)
  for word_mode in (False, True):
    assert max(l for l, _, _ in hit['rows', word_mode]) >= 4
  assert max(l for v in hit.values() for l, _, _ in v) == 6  # index 7 is not reached: see the module's docstring
