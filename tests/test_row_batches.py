"""lddl_amd.loader.plan_row_batches: the batch plan RowBatches iterates, over
hand-made bin arrays on the host (no GPU)."""
import numpy as np
import pytest

from lddl_amd.loader import plan_row_batches

BINS = np.array([2, 0, 0, 3, 2, 2, 0, 3, 2, 2, 0, 0, 2, 5, 2, 0, 2], dtype=np.uint8)  # bins 1 and 4 are empty


def _flat(plan):
  return np.concatenate(plan) if plan else np.zeros(0, np.int64)


@pytest.mark.parametrize('batch_size', [1, 2, 3, 4, 100])
def test_every_row_once_and_no_batch_mixes_bins(batch_size):
  plan = plan_row_batches(BINS, batch_size, seed=7, epoch=0)
  assert all(b.dtype == np.int64 and 1 <= len(b) <= batch_size for b in plan)
  assert sorted(_flat(plan).tolist()) == list(range(len(BINS)))
  for b in plan:
    assert len(set(BINS[b].tolist())) == 1
  # per bin: full batches and at most one short one
  for k in np.unique(BINS):
    sizes = sorted(len(b) for b in plan if BINS[b[0]] == k)
    c = int((BINS == k).sum())
    assert sizes == sorted([batch_size] * (c // batch_size) + ([c % batch_size] if c % batch_size else []))


def test_deterministic_per_seed_and_epoch():
  a = plan_row_batches(BINS, 3, seed=7, epoch=2)
  b = plan_row_batches(BINS, 3, seed=7, epoch=2)
  assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_order_differs_between_epochs_and_seeds():
  bins = np.repeat(np.arange(4), 50)
  plans = [_flat(plan_row_batches(bins, 8, seed=s, epoch=e)).tolist() for s, e in ((7, 0), (7, 1), (8, 0), (8, 1))]
  assert all(sorted(p) == list(range(200)) for p in plans)
  assert len({tuple(p) for p in plans}) == 4
  # rows inside a bin and the batch list are both permuted
  p = plan_row_batches(bins, 8, seed=7, epoch=0)
  assert [int(bins[b[0]]) for b in p] != sorted(int(bins[b[0]]) for b in p)
  assert any(b.tolist() != sorted(b.tolist()) for b in p)


def test_drop_last_drops_only_the_short_batches():
  keep = plan_row_batches(BINS, 3, seed=1, epoch=0, drop_last=False)
  drop = plan_row_batches(BINS, 3, seed=1, epoch=0, drop_last=True)
  assert all(len(b) == 3 for b in drop)
  # bins of 6, 8, 2 and 1 rows: 2 + 2 full batches, and one short batch from each of the last three
  assert len(drop) == 4 and len(keep) == 7
  assert sorted(len(b) for b in keep) == [1, 2, 2, 3, 3, 3, 3]
  full = {tuple(b.tolist()) for b in keep if len(b) == 3}
  assert {tuple(b.tolist()) for b in drop} == full  # the same draws: only the short ones are gone


def test_unbinned_is_one_bin():
  plan = plan_row_batches(None, 4, seed=3, epoch=0, n_rows=10)
  assert sorted(len(b) for b in plan) == [2, 4, 4]
  assert sorted(_flat(plan).tolist()) == list(range(10))
  same = plan_row_batches(np.zeros(10, np.uint8), 4, seed=3, epoch=0)
  assert all(np.array_equal(x, y) for x, y in zip(plan, same))


def test_empty_bins_and_empty_input():
  plan = plan_row_batches(np.array([4, 4, 4, 9], np.uint8), 2, seed=0, epoch=0)  # bins 0-3 and 5-8 empty
  assert sorted(len(b) for b in plan) == [1, 1, 2]
  assert plan_row_batches(np.zeros(0, np.uint8), 4) == []
  assert plan_row_batches(None, 4, n_rows=0) == []


def test_batch_size_larger_than_a_bin():
  plan = plan_row_batches(BINS, 1000, seed=5, epoch=0)
  assert sorted(len(b) for b in plan) == [1, 2, 6, 8]
  assert plan_row_batches(BINS, 1000, seed=5, epoch=0, drop_last=True) == []
  with pytest.raises(ValueError):
    plan_row_batches(BINS, 0)
