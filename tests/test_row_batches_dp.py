"""The data-parallel half of lddl_amd.loader on the host (no GPU): the deal of
shard files to ranks (rank_shard_files), the two planners every rank runs
(plan_row_batches_dp, plan_token_batches_dp), mid-epoch resume (start_step),
the per-rank mask seed (rank_seed), and RowBatches agreeing on counts and on
steps over gloo with 2 and 3 processes."""
import os
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from lddl_amd.loader import (RowBatches, plan_row_batches_dp, plan_token_batches, plan_token_batches_dp, rank_seed,
                             rank_shard_files, shard_files)

COUNTS = np.array([[7, 0, 5, 3], [9, 1, 5, 2], [7, 2, 6, 3]], dtype=np.int64)  # bin 1: empty on rank 0, 1 < a batch
BATCH = 3


# ---- rank_shard_files ---------------------------------------------------------------
def _names(stem='shard-%d'):
  return ['d/' + (stem % p) + '.parquet_%d' % b for p in (7, 0, 21, 3, 10, 4) for b in (2, 0, 1)]


@pytest.mark.parametrize('stem', ['shard-%d', 'part.%d'])
@pytest.mark.parametrize('world', [1, 2, 3, 6])
def test_rank_files_partition_the_list_and_keep_partitions_whole(world, stem):
  files = shard_files(_names(stem))
  assert len(files) == 18
  parts = sorted({f[1] for f in files})
  assert parts == [0, 3, 4, 7, 10, 21]
  per_rank = [rank_shard_files(files, r, world) for r in range(world)]
  assert sorted(f for fs in per_rank for f in fs) == sorted(files) and sum(len(fs) for fs in per_rank) == 18
  for r, fs in enumerate(per_rank):
    assert fs == [f for f in files if f in fs]  # (partition, bin) order kept
    assert sorted({f[1] for f in fs}) == parts[r::world]  # round-robin over the sorted distinct partitions
    for p in {f[1] for f in fs}:
      assert [f[2] for f in fs if f[1] == p] == [0, 1, 2]  # a shard and its bins never split


def test_rank_files_unbinned():
  files = shard_files(['shard-%d.parquet' % k for k in range(4)])
  assert rank_shard_files(files, 1, 2) == [('shard-1.parquet', 1, None), ('shard-3.parquet', 3, None)]


def test_rank_files_refusals():
  files = shard_files(_names())
  with pytest.raises(ValueError, match=r'6 partitions.*world_size 4'):
    rank_shard_files(files, 0, 4)
  for rank, world in ((2, 2), (-1, 2), (0, 0)):
    with pytest.raises(ValueError):
      rank_shard_files(files, rank, world)


# ---- plan_row_batches_dp ------------------------------------------------------------
def _rank_bins(counts, rank):
  """the rows of a rank in an order that is not sorted by bin"""
  bins = np.repeat(np.arange(counts.shape[1]), counts[rank])
  return bins[np.random.default_rng(100 + rank).permutation(bins.size)].astype(np.uint8)


def _plans(world, drop_last, seed=7, epoch=0):
  counts = COUNTS[:world]
  bins = [_rank_bins(counts, r) for r in range(world)]
  return counts, bins, [plan_row_batches_dp(bins[r], counts, r, BATCH, seed, epoch, drop_last) for r in range(world)]


@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('world', [1, 2, 3])
def test_row_plans_agree_across_ranks(world, drop_last):
  counts, bins, plans = _plans(world, drop_last)
  used = counts.min(axis=0)
  steps = [int(n) // BATCH if drop_last else -(-int(n) // BATCH) for n in used]
  assert all(len(p) == sum(steps) for p in plans)  # the same number of steps
  step_bins = [int(bins[0][b[0]]) for b in plans[0]]
  assert [step_bins.count(b) for b in range(4)] == steps
  for r, plan in enumerate(plans):
    assert all(b.dtype == np.int64 and 1 <= len(b) <= BATCH for b in plan)
    assert [len(b) for b in plan] == [len(b) for b in plans[0]]  # the same batch length at every step
    for b, k in zip(plan, step_bins):
      assert (bins[r][b] == k).all()  # every row in the bin its step names, the same bin on every rank
    flat = np.concatenate(plan)
    assert len(set(flat.tolist())) == flat.size  # no row used twice
    per_bin = np.bincount(bins[r][flat], minlength=4)
    want = [(n // BATCH) * BATCH for n in used] if drop_last else used
    assert per_bin.tolist() == [int(n) for n in want]  # exactly min_w rows per bin (less the short batch dropped)
  if world == 3 and not drop_last:
    assert used.tolist() == [7, 0, 5, 2] and steps == [3, 0, 2, 1]
    assert sorted(len(b) for b in plans[0]) == [1, 2, 2, 3, 3, 3]


def test_row_plans_differ_between_ranks_and_epochs_and_repeat():
  counts = np.full((2, 3), 40, dtype=np.int64)
  bins = np.repeat(np.arange(3), 40).astype(np.uint8)  # both ranks hold the same layout: only the seed tells them apart
  plan = lambda r, e, s=7: plan_row_batches_dp(bins, counts, r, 8, s, e)  # noqa: E731
  flat = lambda p: np.concatenate(p).tolist()  # noqa: E731
  a, b = plan(0, 0), plan(1, 0)
  assert [int(bins[x[0]]) for x in a] == [int(bins[x[0]]) for x in b]
  assert flat(a) != flat(b)  # ranks' row orders differ
  assert flat(a) != flat(plan(0, 1)) and flat(a) != flat(plan(0, 0, 8))  # epochs and seeds differ
  assert [int(bins[x[0]]) for x in a] != [int(bins[x[0]]) for x in plan(0, 1)]  # and so does the step order
  assert [int(bins[x[0]]) for x in a] != sorted(int(bins[x[0]]) for x in a)  # the steps are permuted
  again = plan(0, 0)
  assert len(a) == len(again) and all(np.array_equal(x, y) for x, y in zip(a, again))


def test_row_plan_surplus_rows_rotate_between_epochs():
  """a rank with more than min_w rows leaves some out each epoch, and not always the same ones"""
  counts = np.array([[10], [4]], dtype=np.int64)
  left_out = set()
  for epoch in range(6):
    flat = np.concatenate(plan_row_batches_dp(None, counts, 0, 2, 7, epoch, n_rows=10))
    assert flat.size == 4 and len(set(flat.tolist())) == 4
    left_out.add(tuple(sorted(set(range(10)) - set(flat.tolist()))))
  assert len(left_out) > 1


def test_row_plan_refusals():
  bins = _rank_bins(COUNTS, 1)
  with pytest.raises(ValueError, match='batch_size'):
    plan_row_batches_dp(bins, COUNTS, 1, 0)
  with pytest.raises(ValueError, match='counts'):
    plan_row_batches_dp(bins, COUNTS, 0, 3)  # another rank's rows
  with pytest.raises(ValueError):
    plan_row_batches_dp(bins, COUNTS, 3, 3)
  with pytest.raises(ValueError):
    plan_row_batches_dp(bins, COUNTS[1], 0, 3)


# ---- plan_token_batches_dp ----------------------------------------------------------
LENGTHS = np.random.default_rng(3).integers(5, 65, 150)


@pytest.mark.parametrize('rank', [0, 1, 2])
def test_token_plan_keeps_both_caps_and_every_row_once(rank):
  plan = plan_token_batches_dp(LENGTHS, rank, 128, 4, seed=7, epoch=0)
  assert all(b.dtype == np.int64 and 1 <= len(b) <= 4 and int(LENGTHS[b].sum()) <= 128 for b in plan)
  assert sorted(np.concatenate(plan).tolist()) == list(range(150))
  assert any(len(b) == 4 for b in plan) and any(int(LENGTHS[b].sum()) + int(LENGTHS.min()) > 128 for b in plan)
  again = plan_token_batches_dp(LENGTHS, rank, 128, 4, seed=7, epoch=0)
  assert len(plan) == len(again) and all(np.array_equal(x, y) for x, y in zip(plan, again))


def test_token_plan_steps_truncate_and_oversize_raises():
  whole = plan_token_batches_dp(LENGTHS, 1, 128, 4, seed=7, epoch=2)
  n = len(whole)
  for steps in (0, 1, n - 1, n):
    cut = plan_token_batches_dp(LENGTHS, 1, 128, 4, seed=7, epoch=2, steps=steps)
    assert len(cut) == steps and all(np.array_equal(x, y) for x, y in zip(cut, whole))
    flat = np.concatenate(cut) if cut else np.zeros(0, np.int64)
    assert len(set(flat.tolist())) == flat.size  # no row appears twice
  with pytest.raises(ValueError, match='steps %d' % (n + 1)):
    plan_token_batches_dp(LENGTHS, 1, 128, 4, seed=7, epoch=2, steps=n + 1)
  with pytest.raises(ValueError, match='max_tokens'):
    plan_token_batches_dp(LENGTHS, 1, int(LENGTHS.max()) - 1, 4)  # a row longer than a batch may be


def test_token_plans_differ_between_ranks_and_epochs():
  flat = lambda r, e: np.concatenate(plan_token_batches_dp(LENGTHS, r, 128, 4, seed=7, epoch=e)).tolist()  # noqa: E731
  assert flat(0, 0) != flat(1, 0) and flat(0, 0) != flat(0, 1)
  assert flat(0, 0) != np.concatenate(plan_token_batches(LENGTHS, 128, 4, seed=7, epoch=0)).tolist()


# ---- RowBatches on a stand-in result -------------------------------------------------
def _result(bins, lengths=None, nbins=4):
  """what RowBatches reads of a PackResult, on the CPU: len0 / len1 / flags / bins / n_pairs / nbins"""
  n = len(bins)
  lengths = np.full(n, 10) if lengths is None else np.asarray(lengths)
  l0 = (lengths - 3) // 2
  return types.SimpleNamespace(len0=torch.from_numpy(l0.astype(np.int16)),
                               len1=torch.from_numpy((lengths - 3 - l0).astype(np.int16)),
                               flags=torch.full((n,), 2, dtype=torch.uint8),
                               bins=torch.from_numpy(np.asarray(bins, np.uint8)), n_pairs=n, nbins=nbins)


def _lists(it):
  return [b.tolist() for b in it]


@pytest.mark.parametrize('dp', [False, True])
@pytest.mark.parametrize('tokens', [False, True])
def test_start_step_iterates_the_tail_of_the_plan(dp, tokens):
  res = _result(_rank_bins(COUNTS, 1), np.random.default_rng(4).integers(5, 65, int(COUNTS[1].sum())))
  kw = dict(max_tokens=128, max_rows=4) if tokens else dict(batch_size=BATCH)
  if dp:
    kw.update(rank=1, world_size=3, **(dict(steps=5) if tokens else dict(counts=COUNTS)))
  full = _lists(RowBatches(res, seed=7, epoch=3, **kw))
  n = len(full)
  assert n == (5 if dp and tokens else len(RowBatches(res, seed=7, epoch=3, **kw))) and n >= 5
  for k in (0, 1, n - 1, n, n + 2):
    rb = RowBatches(res, seed=7, epoch=3, start_step=k, **kw)
    assert len(rb) == n  # the whole epoch
    assert _lists(rb) == full[k:]
  rb = RowBatches(res, seed=7, **kw)
  rb.set_epoch(3, start_step=2)
  assert _lists(rb) == full[2:] and len(rb) == n
  rb.set_epoch(3)  # the next epoch starts at its first batch again
  assert _lists(rb) == full
  with pytest.raises(ValueError, match='start_step'):
    RowBatches(res, seed=7, start_step=-1, **kw)


def test_row_batches_uses_the_dp_planners():
  bins = [_rank_bins(COUNTS, r) for r in range(3)]
  for r in range(3):
    rb = RowBatches(_result(bins[r]), BATCH, seed=9, epoch=2, rank=r, world_size=3, counts=COUNTS)
    want = plan_row_batches_dp(bins[r], COUNTS, r, BATCH, 9, 2)
    assert _lists(rb) == [b.tolist() for b in want] and len(rb) == len(want) == 6
  lengths = np.random.default_rng(4).integers(5, 65, 40)
  rb = RowBatches(_result(np.zeros(40, np.uint8), lengths, nbins=1), max_tokens=128, max_rows=4, seed=9, rank=2,
                  world_size=3, steps=7)
  assert _lists(rb) == [b.tolist() for b in plan_token_batches_dp(lengths, 2, 128, 4, 9, 0, steps=7)]
  # an unbinned table is one bin; a world of one needs no counts and no group
  rb = RowBatches(_result(np.zeros(10, np.uint8), nbins=1), 4, rank=0, world_size=1)
  assert sorted(len(b) for b in rb) == [2, 4, 4]
  assert len(RowBatches(_result(np.zeros(10, np.uint8), nbins=1), max_tokens=30, rank=0, world_size=1)) == 4


def test_row_batches_refusals():
  res = _result(_rank_bins(COUNTS, 0))
  for kw in (dict(batch_size=3, rank=0, world_size=3),             # no process group and no counts
             dict(max_tokens=128, rank=0, world_size=3),           # ... and no steps
             dict(batch_size=3, world_size=3),                     # a world without a rank
             dict(batch_size=3, counts=COUNTS),
             dict(batch_size=3, rank=0),                           # no group to take the world from
             dict(batch_size=3, rank=3, world_size=3, counts=COUNTS),
             dict(batch_size=3, rank=1, world_size=3, counts=COUNTS),   # another rank's counts
             dict(batch_size=3, rank=0, world_size=2, counts=COUNTS),   # three rows of counts for two ranks
             dict(batch_size=3, rank=0, world_size=3, steps=4),
             dict(max_tokens=128, rank=0, world_size=3, counts=COUNTS)):
    with pytest.raises(ValueError):
      RowBatches(res, **kw)
  with pytest.raises(ValueError, match='steps'):
    RowBatches(res, max_tokens=128, rank=0, world_size=3, steps=1000).plan()


def test_without_a_rank_the_plans_are_the_old_ones():
  from lddl_amd.loader import plan_row_batches
  bins = _rank_bins(COUNTS, 2)
  res = _result(bins)
  want = plan_row_batches(bins, BATCH, 5, 1)
  assert _lists(RowBatches(res, BATCH, seed=5, epoch=1)) == [b.tolist() for b in want]
  lengths = np.full(len(bins), 10)
  want = plan_token_batches(lengths, 35, None, 5, 1)
  assert _lists(RowBatches(res, max_tokens=35, seed=5, epoch=1)) == [b.tolist() for b in want]


# ---- rank_seed ----------------------------------------------------------------------
def test_rank_seed_is_distinct_and_stable():
  seeds = [rank_seed(1234, r) for r in range(8)]
  assert len(set(seeds)) == 8 and all(0 <= s < 1 << 64 for s in seeds)
  assert 1234 not in seeds and len({rank_seed(s, 0) for s in (1234, 1235, 12345)}) == 3
  # splitmix64's output function over base + (rank + 1) * 0x9E3779B97F4A7C15, written out here
  m = (1 << 64) - 1
  for r, s in enumerate(seeds):
    z = (1234 + (r + 1) * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    assert s == z ^ (z >> 31)
  assert seeds[:2] == PINNED[:2] and rank_seed(0, 0) == PINNED[2] and rank_seed((1 << 64) - 1, 7) == PINNED[3]


# rank_seed(0, 0) is the first output of splitmix64 seeded with 0, 0xE220A8397B1DCDAF
PINNED = [13478418381427711195, 10936887474700444964, 0xE220A8397B1DCDAF, 4638043754431676516]


# ---- gloo ---------------------------------------------------------------------------
def _gloo_rank(rank, world, port, q):
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  counts = COUNTS[:world]
  bins = _rank_bins(counts, rank)
  lengths = np.random.default_rng(50 + rank).integers(5, 65, bins.size)
  res = _result(bins, lengths)
  out = {}
  rb = RowBatches(res, BATCH, seed=11, rank=rank)  # the world from the group, the counts gathered
  out['counts'] = rb.counts.tolist()
  for epoch in (0, 1):
    rb.set_epoch(epoch)
    out['rows', epoch] = (len(rb), _lists(rb))
  tb = RowBatches(res, max_tokens=128, max_rows=4, seed=11, rank=rank, world_size=world)
  for epoch in (0, 1):
    tb.set_epoch(epoch)
    out['tokens', epoch] = (len(tb), _lists(tb))
  q.put((rank, bins.tolist(), lengths.tolist(), out))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_agree_over_gloo(world):
  """no explicit counts or steps: every rank reports the step count and the bin sequence of the pure planner over
  the gathered counts, and the token plans stop at the shortest rank's"""
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = 29500 + (os.getpid() + 7 * world) % 1000
  procs = [ctx.Process(target=_gloo_rank, args=(r, world, port, q)) for r in range(world)]
  for p in procs:
    p.start()
  got = sorted(q.get(timeout=120) for _ in range(world))
  for p in procs:
    p.join(60)
    assert p.exitcode == 0
  counts = COUNTS[:world]
  for epoch in (0, 1):
    seqs, local = [], []
    for rank, bins, lengths, out in got:
      bins, lengths = np.asarray(bins, np.uint8), np.asarray(lengths)
      assert out['counts'] == counts.tolist()
      want = plan_row_batches_dp(bins, counts, rank, BATCH, 11, epoch)
      n, plan = out['rows', epoch]
      assert n == len(plan) == len(want) and plan == [b.tolist() for b in want]
      seqs.append([(int(bins[b[0]]), len(b)) for b in plan])
      local.append(len(plan_token_batches_dp(lengths, rank, 128, 4, 11, epoch)))
    assert all(s == seqs[0] for s in seqs) and len(seqs[0]) > 0
    for rank, bins, lengths, out in got:
      n, plan = out['tokens', epoch]
      want = plan_token_batches_dp(np.asarray(lengths), rank, 128, 4, 11, epoch, steps=min(local))
      assert n == len(plan) == min(local) and plan == [b.tolist() for b in want]
  assert len(set(local)) > 1 or world == 1  # the ranks' own plans differ in length: the minimum cut something
