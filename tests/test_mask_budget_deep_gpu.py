"""Exact-count dynamic masking (lddl_set_mask_budget) where
tests/test_mask_budget_gpu.py does not reach: the lower levels of
mask_budget.hip's radix select, a wave's second row, the life of the
thresholds' workspace slot on one ctx, and the routes that were never run with
the switch on (MlmCollate, the RowBatches iterators).  Everything is compared
bit for bit with the sort model of tests/budget_model.py.

The deep cases are the constants of tests/budget_cases.py;
tests/test_budget_model_host.py derives, without a GPU, which level and exit of
budget_threshold each of them reaches.  Exit level index 7 (two keys of one row
sharing 56 bits, about 2^-17 per seed at 2^20 - 1 columns) is reached by none
and is not required.
"""
import functools

import numpy as np
import pytest
import torch

import budget_cases as bc
import budget_model as bm
from test_mask_budget_gpu import COUNTER, IGNORE, MASK, ROWS, V, check_route, collate, host, model, table, tokenizer, world

pytestmark = pytest.mark.gpu

SHORT = [g for g, r in enumerate(ROWS) if r[0] <= 131]  # the rows of 5 .. 131 tokens
P_MANY, p_MANY = 20, 0.5  # the cap binds on the rows of 64 tokens and more, the ratio on the shorter ones


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the committed cases -------------------------------------------------------------
@pytest.mark.parametrize('entry', bc.CASES, ids=bc.case_id)
def test_committed_case(gpu, entry):
  case = entry[0]
  ids, sp = bc.planes(case)
  m = bm.mask(ids, sp, bc.cont() if case.word else None, case.seed, case.counter, case.p, case.P, MASK, V, IGNORE)
  col = collate(False, case.word, case.P, case.p, seed=case.seed, counter=case.counter)
  if case.front == 'mask_tokens':
    x, lab = col.mask_tokens(dev(ids), dev(sp), counter=case.counter)
  else:
    res, idx = world()[1], [0] * case.row + [case.src]
    enc = col.collate_rows(res, idx, mode=0)  # the batch the case was derived from
    assert np.array_equal(host(enc['input_ids']), ids) and np.array_equal(host(enc['special_tokens_mask']), sp)
    out = col.collate_rows(res, idx)
    x, lab = out['input_ids'], out['labels']
  assert np.array_equal(host(lab), m.labels) and np.array_equal(host(x), m.input_ids)
  r = case.row
  count, want = int(m.select[r].sum()), bm.budget(int((sp[r] == 0).sum()), case.p, case.P)
  assert count <= want and (case.word or count == want)  # (a word that fits in part leaves the rest of the budget)


# ---- 2. more rows than one pass of the grid ------------------------------------------------
def n_many():
  return torch.cuda.get_device_properties(0).multi_processor_count * 32 + 5  # grid_rows: 8 blocks of 4 rows per CU


@functools.lru_cache(maxsize=None)
def many(code, wwm):
  """the short rows cycled over more rows than one pass of the grid: the row indices, the unmasked padded batch,
  its attention mask and the model over it"""
  cycle = [g for g in SHORT[::-1] if code or ROWS[g][1]]  # (a BERT collate takes the rows that have the first [SEP])
  idx = [cycle[i % len(cycle)] for i in range(n_many())]
  enc = collate(code, wwm, P_MANY, p_MANY).collate_rows(world()[1], idx, mode=0)
  m = model(host(enc['input_ids']), host(enc['special_tokens_mask']), wwm, P_MANY, p_MANY)
  return idx, enc, host(enc['attention_mask']) != 0, m


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
@pytest.mark.parametrize('route', ['mask_tokens', 'rows', 'unpadded', 'fixed', 'code_rows'])
def test_more_rows_than_one_pass(gpu, route, wwm):
  code = route == 'code_rows'
  idx, enc, keep, m = many(code, wwm)
  n, width = len(idx), 131 if code else 136
  fixed = dict(max_tokens=int(keep.sum()) + 7, max_seqs=n + 3, max_seqlen=width)
  check_route(collate(code, wwm, P_MANY, p_MANY, compact_mlm=True), 'rows' if code else route, world()[1], idx, enc, keep, m,
              fixed, width, (route, wwm))
  # teeth: a later-pass row shows the table row of a first-pass row and is masked differently
  first, later = n - 5, 0
  for r in range(first, n):
    r0 = next(q for q in range(first) if idx[q] == idx[r])
    assert np.array_equal(host(enc['input_ids'][r]), host(enc['input_ids'][r0]))
    if ROWS[idx[r]][0] >= 64:
      later += 1
      assert not np.array_equal(m.labels[r], m.labels[r0])
  assert later >= 2
  if not wwm:
    cand = (host(enc['special_tokens_mask']) == 0).sum(1)
    assert m.select.sum(1).tolist() == [bm.budget(int(c), p_MANY, P_MANY) for c in cand]  # (and the GPU equals m)


def test_word_planes_without_special_columns(gpu):
  """lddl_mask_tokens over more rows than one pass, 64 columns and no special one, a '##' id in column 0: what is
  in front of column 0 is nothing, at every level of every row, not the last column of the level or row before
  (about one row in six goes on to the second level: some 45 words over 256 bins)"""
  n = n_many()
  rng = np.random.default_rng(64)
  ids = np.where(rng.random((n, 64)) < 0.4, rng.integers(31, 57, (n, 64)), rng.integers(5, 31, (n, 64)))
  ids[:, 0] = rng.integers(31, 57, n)
  sp = np.zeros((n, 64), np.int64)
  m = model(ids, sp, True, P_MANY, p_MANY)
  x, lab = collate(False, True, P_MANY, p_MANY).mask_tokens(dev(ids), dev(sp), counter=COUNTER)
  assert np.array_equal(host(lab), m.labels) and np.array_equal(host(x), m.input_ids)
  assert m.select[:, 0].any() and not m.select[:, 0].all()


# ---- 3. the thresholds' slot on one ctx --------------------------------------------------
@pytest.mark.parametrize('side', [False, True], ids=['default-stream', 'side-stream'])
def test_slot_life_cycle_on_one_ctx(gpu, side):
  """3 rows, more rows than one pass (the slot grows), 3 rows again; another max_predictions on the same ctx; then
  off, which is the ctx that never had it on"""
  from lddl_amd.tokenizer import Tokenizer
  import synth_vocab as sv
  res, tok, never = world()[1], Tokenizer(sv.vocab_path('tiny64'), 0), Tokenizer(sv.vocab_path('tiny64'), 0)
  small, (big, _, _, m_big) = [5, 3, 10], many(False, True)
  enc = collate(False, True, 0, p_MANY).collate_rows(res, small, mode=0)
  ids, sp = host(enc['input_ids']), host(enc['special_tokens_mask'])
  stream = torch.cuda.Stream() if side else torch.cuda.current_stream()

  def run(P, idx, t=tok, rows=True):
    with torch.cuda.stream(stream):
      col = collate(False, True, P, p_MANY, tok=t)  # (sets the switch on t's ctx)
      if rows:
        out = col.collate_rows(res, idx)
        got = out['input_ids'], out['labels']
      else:
        got = col.mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], counter=COUNTER)
    stream.synchronize()
    return host(got[0]), host(got[1])

  def same(got, m):
    return np.array_equal(got[1], m.labels) and np.array_equal(got[0], m.input_ids)
  m20, m7 = model(ids, sp, True, P_MANY, p_MANY), model(ids, sp, True, 7, p_MANY)
  assert not np.array_equal(m20.labels, m7.labels)
  assert same(run(P_MANY, small), m20)
  assert same(run(P_MANY, big), m_big)
  assert same(run(P_MANY, small), m20)
  assert same(run(P_MANY, small, rows=False), m20)  # lddl_mask_tokens shares the slot
  assert same(run(7, small), m7)
  assert same(run(7, small, rows=False), m7)
  off, plain = run(0, small), run(0, small, t=never)
  assert np.array_equal(off[0], plain[0]) and np.array_equal(off[1], plain[1])
  assert not np.array_equal(off[1], m7.labels) and (off[1] != IGNORE).any()
  assert same(run(P_MANY, small), m20)  # and on again


# ---- 4. routes never run with the switch on ------------------------------------------------
@functools.lru_cache(maxsize=None)
def mlm_world():
  """the rows of ROWS as single-segment rows ([CLS] A B [SEP], no NSP): an MLM-only table"""
  segs = [[[], a + b] for a, b in bc.segments()]
  return table(tokenizer(), segs, [0] * len(segs), kind='mlm')


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
@pytest.mark.parametrize('route', ['rows', 'unpadded', 'fixed'])
def test_mlm_collate(gpu, route, wwm):
  from lddl_amd.loader import MlmCollate
  res, idx = mlm_world(), [7, 3, 0, 5, 1, 9, 2, 8, 4, 6, 10]
  for P, p in ((20, 0.15), (80, 0.5), (1, 1.0)):
    enc = collate(True, wwm, P, p, cls=MlmCollate).collate_rows(res, idx, mode=0)
    assert 'next_sentence_labels' not in enc and not enc['token_type_ids'].any()
    keep = host(enc['attention_mask']) != 0
    assert keep.sum(1).tolist() == [ROWS[g][0] - ROWS[g][1] for g in idx]
    m = model(host(enc['input_ids']), host(enc['special_tokens_mask']), wwm, P, p)
    fixed = dict(max_tokens=int(keep.sum()) + 9, max_seqs=len(idx) + 2, max_seqlen=2047)
    check_route(collate(True, wwm, P, p, cls=MlmCollate, compact_mlm=True), route, res, idx, enc, keep, m, fixed, 2047,
                (route, wwm, P, p))


def epoch_equals_model(col_of, res, batches, route, wwm, P, p, seed):
  """every batch of an epoch against the model at that batch's counter -> the number of batches"""
  col, ref = col_of(compact_mlm=True), col_of()
  col.counter = ref.counter = 0
  steps = 0
  for step, idx in enumerate(batches):
    enc = ref.collate_rows(res, idx, mode=0)  # (mode 0 leaves the counter)
    assert col.counter == step
    keep = host(enc['attention_mask']) != 0
    m = model(host(enc['input_ids']), host(enc['special_tokens_mask']), wwm, P, p, seed=seed, counter=step)
    lab = check_route(col, route, res, idx, enc, keep, m, None, enc['input_ids'].shape[1], (route, wwm, step))
    assert m.select.sum(1).max() <= P and (lab != IGNORE).sum() == m.select.sum()  # no row has more than P labels
    steps += 1
  assert col.counter == steps
  return steps


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
def test_row_batches(gpu, wwm):
  from lddl_amd.loader import CodeCollate, RowBatches
  res, P, p = world()[1], 20, 0.5
  make = lambda **kw: collate(True, wwm, P, p, seed=77, cls=CodeCollate, **kw)  # noqa: E731 (rows with and without [SEP])
  assert epoch_equals_model(make, res, RowBatches(res, 4, seed=3), 'rows', wwm, P, p, 77) == 3
  assert epoch_equals_model(make, res, RowBatches(res, max_tokens=2200, max_rows=5, seed=3), 'unpadded', wwm, P, p, 77) >= 3


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
def test_row_batches_data_parallel_pair(gpu, wwm):
  """two ranks in one process: the even and the odd rows of ROWS as the ranks' tables, counts / steps given"""
  from lddl_amd.loader import CodeCollate, RowBatches, rank_seed
  P, p, segs, tok = 20, 0.5, bc.segments(), tokenizer()
  mine = [list(range(r, len(ROWS), 2)) for r in (0, 1)]
  tables = [table(tok, [segs[g] for g in gs], [ROWS[g][1] for g in gs]) for gs in mine]
  counts = [[len(gs)] for gs in mine]
  steps = []
  for r, t in enumerate(tables):
    seed = rank_seed(77, r)
    make = lambda **kw: collate(True, wwm, P, p, seed=seed, cls=CodeCollate, **kw)  # noqa: E731
    binned = RowBatches(t, 2, seed=3, rank=r, world_size=2, counts=counts)
    steps.append(epoch_equals_model(make, t, binned, 'rows', wwm, P, p, seed))
    tokens = RowBatches(t, max_tokens=2200, max_rows=3, seed=3, rank=r, world_size=2, steps=2)
    assert epoch_equals_model(make, t, tokens, 'unpadded', wwm, P, p, seed) == 2
  assert steps[0] == steps[1] == 3  # the fewest rows of a rank: 5, in batches of 2
