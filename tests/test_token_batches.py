"""plan_token_batches: the token-budget batches of the padding-free collate
(loader.RowBatches(res, max_tokens=...)), against a restatement of its rule:
permute all rows, walk the permutation and close the batch when the next row
would break the token or the row limit.  No GPU."""
import types

import numpy as np
import pytest

from lddl_amd.loader import RowBatches, plan_row_batches, plan_token_batches


def restated(lengths, max_tokens, max_rows, seed, epoch):
  rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, epoch])))
  out, cur, tokens = [], [], 0
  for g in rng.permutation(len(lengths)):
    if cur and (tokens + lengths[g] > max_tokens or (max_rows is not None and len(cur) + 1 > max_rows)):
      out.append(cur)
      cur, tokens = [], 0
    cur.append(int(g))
    tokens += int(lengths[g])
  if cur:
    out.append(cur)
  return out


LENGTHS = np.random.default_rng(11).integers(5, 513, 3001)


@pytest.mark.parametrize('max_tokens', [512, 513, 4096])
@pytest.mark.parametrize('max_rows', [1, 7, None])
def test_plan_token_batches(max_tokens, max_rows):
  plan = plan_token_batches(LENGTHS, max_tokens, max_rows, seed=5, epoch=2)
  assert all(b.dtype == np.int64 and b.ndim == 1 and len(b) > 0 for b in plan)
  assert sorted(np.concatenate(plan).tolist()) == list(range(len(LENGTHS)))  # every row once
  for k, b in enumerate(plan):
    tokens = int(LENGTHS[b].sum())
    assert tokens <= max_tokens and (max_rows is None or len(b) <= max_rows)
    if k + 1 < len(plan):  # the batch was closed because the next row did not fit
      nxt = int(LENGTHS[plan[k + 1][0]])
      assert tokens + nxt > max_tokens or (max_rows is not None and len(b) + 1 > max_rows)
  assert [b.tolist() for b in plan] == restated(LENGTHS, max_tokens, max_rows, 5, 2)
  if max_rows == 1:
    assert len(plan) == len(LENGTHS)


def test_seed_and_epoch():
  a = plan_token_batches(LENGTHS, 2048, seed=9, epoch=0)
  b = plan_token_batches(LENGTHS, 2048, seed=9, epoch=0)
  assert [x.tolist() for x in a] == [x.tolist() for x in b]
  c = plan_token_batches(LENGTHS, 2048, seed=9, epoch=1)
  assert [x.tolist() for x in a] != [x.tolist() for x in c]
  d = plan_token_batches(LENGTHS, 2048, seed=10, epoch=0)
  assert [x.tolist() for x in a] != [x.tolist() for x in d]
  # the permutation is drawn as plan_row_batches draws one bin's
  one = plan_row_batches(None, len(LENGTHS), seed=9, epoch=0, n_rows=len(LENGTHS))
  assert np.concatenate(a).tolist() == one[0].tolist()


def test_refusals_and_empty():
  with pytest.raises(ValueError):
    plan_token_batches([5, 513, 7], 512)
  assert [b.tolist() for b in plan_token_batches([512], 512)] == [[0]]
  for bad in (0, -3):
    with pytest.raises(ValueError):
      plan_token_batches([5, 6], bad)
  with pytest.raises(ValueError):
    plan_token_batches([5, 6], 64, max_rows=0)
  assert plan_token_batches([], 512) == []
  assert plan_token_batches(np.zeros(0, np.int64), 512, max_rows=3) == []


def test_row_batches_takes_one_of_the_two():
  res = types.SimpleNamespace()  # refused before the result is looked at
  with pytest.raises(ValueError):
    RowBatches(res)
  with pytest.raises(ValueError):
    RowBatches(res, 64, max_tokens=2048)
  with pytest.raises(ValueError):
    RowBatches(res, batch_size=64, max_tokens=2048)
