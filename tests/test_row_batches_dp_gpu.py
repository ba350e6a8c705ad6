"""Data-parallel batches on the GPU, one process and one device standing in for
every rank: ``load_shards(..., rank=, world_size=)`` over a balanced shard
directory, and ``RowBatches(rank table, ..., rank=, world_size=, counts= /
steps=)`` through every collate route, against the single-process loader.  A
rank's batch must be, bit for bit, the collate of the same rows taken from the
table of the whole directory; a row is found there through (partition,
position within the partition).

The shards are written by hand with pyarrow in the load balancer's layout
(``shard-<k>.parquet_<b>``, the rows of a bin spread so that shards differ by
one row at most): 6 shards x 4 bins at sequence length 64 (bins of 16 tokens),
250 rows of words from the vocabulary, plain and with static masks.  The
CodeBERT and MLM-only directories are 4 shards x 2 bins at length 32."""
import io
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from lddl_amd import _lib

pytestmark = pytest.mark.gpu

BIN = 16
BASE, EXTRA = [9, 14, 11, 6], [2, 0, 5, 3]  # rows of bin b in shard k: BASE[b] + (k < EXTRA[b])
N_ROWS = 6 * sum(BASE) + sum(EXTRA)
SHARD_IDS = [0, 1, 2, 3, 4, 5]


def words_of(vocab_file, n=300):
  with open(vocab_file, 'rb') as f:
    toks = [l.rstrip() for l in f.read().decode('utf-8').split('\n')]
  pick = [t for t in toks[2000:] if t.isascii() and t.isalpha() and t.islower()][:n]
  assert len(pick) == n
  return pick


def npy(positions):
  f = io.BytesIO()
  np.save(f, np.asarray(positions, np.uint16))
  return f.getvalue()


def bert_rows(rng, words, b, n, static):
  """n rows of bin b: num_tokens = len(A) + len(B) + 3 in (16 b, 16 b + 16]"""
  cols = {k: [] for k in ('A', 'B', 'is_random_next', 'num_tokens', 'masked_lm_positions', 'masked_lm_labels')}
  for _ in range(n):
    total = int(rng.integers(max(BIN * b + 1, 6), BIN * b + BIN + 1))
    la = int(rng.integers(1, total - 3))
    lb = total - 3 - la
    a, bb = [words[j] for j in rng.integers(0, len(words), la)], [words[j] for j in rng.integers(0, len(words), lb)]
    if static:  # the shard shows the masked tokens; the labels hold the original ones
      shown = [None] + a + [None] + bb + [None]
      cand = [p for p, t in enumerate(shown) if t is not None]
      pos = sorted(rng.permutation(cand)[:max(1, int(0.15 * total))].tolist())
      cols['masked_lm_positions'].append(npy(pos))
      cols['masked_lm_labels'].append(' '.join(shown[p] for p in pos))
      for p in pos:
        draw = rng.random()
        shown[p] = '[MASK]' if draw < 0.8 else words[int(rng.integers(0, len(words)))] if draw < 0.9 else shown[p]
      a, bb = shown[1:1 + la], shown[2 + la:2 + la + lb]
    cols['A'].append(' '.join(a))
    cols['B'].append(' '.join(bb))
    cols['is_random_next'].append(bool(rng.integers(0, 2)))
    cols['num_tokens'].append(total)
  t = {'A': pa.array(cols['A'], pa.string()), 'B': pa.array(cols['B'], pa.string()),
       'is_random_next': pa.array(cols['is_random_next'], pa.bool_()),
       'num_tokens': pa.array(cols['num_tokens'], pa.uint16())}
  if static:
    t['masked_lm_positions'] = pa.array(cols['masked_lm_positions'], pa.binary())
    t['masked_lm_labels'] = pa.array(cols['masked_lm_labels'], pa.string())
  return pa.table(t)


def single_rows(rng, words, b, n, code):
  """n rows of bin b at length 32: MLM-only (A, num_tokens = len(A) + 2), or CodeBERT (doc / code / num_tokens,
  every third row without a docstring: code + 2)"""
  docs, codes, nts = [], [], []
  for i in range(n):
    total = int(rng.integers(max(BIN * b + 1, 6), BIN * b + BIN + 1))
    if code and i % 3:
      ld = int(rng.integers(1, total - 3))
      docs.append(' '.join(words[j] for j in rng.integers(0, len(words), ld)))
      codes.append(' '.join(words[j] for j in rng.integers(0, len(words), total - 3 - ld)))
    else:
      docs.append('')
      codes.append(' '.join(words[j] for j in rng.integers(0, len(words), total - 2)))
    nts.append(total)
  nt = pa.array(nts, pa.uint16())
  if code:
    return pa.table({'id': pa.array(['d%d' % i for i in range(n)]), 'doc': pa.array(docs), 'code': pa.array(codes),
                     'num_tokens': nt})
  return pa.table({'A': pa.array(codes), 'num_tokens': nt})


@pytest.fixture(scope='module')
def tok(gpu):
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(_lib.VOCAB_BERT, 0)


@pytest.fixture(scope='module')
def dirs(tmp_path_factory):
  """{'plain' / 'static' / 'mlm' / 'code': a balanced directory}"""
  out = {}
  bert, codebert = words_of(_lib.VOCAB_BERT), words_of(_lib.VOCAB_CODEBERT)
  for kind in ('plain', 'static'):
    d = out[kind] = str(tmp_path_factory.mktemp(kind))
    rng = np.random.default_rng(17)
    for k in SHARD_IDS:
      for b in range(4):
        pq.write_table(bert_rows(rng, bert, b, BASE[b] + (k < EXTRA[b]), kind == 'static'),
                       os.path.join(d, 'shard-%d.parquet_%d' % (k, b)))
  for kind in ('mlm', 'code'):
    d = out[kind] = str(tmp_path_factory.mktemp(kind))
    rng = np.random.default_rng(23)
    for k in range(4):
      for b in range(2):
        pq.write_table(single_rows(rng, codebert if kind == 'code' else bert, b, 11 + 3 * b + (k < 1 + b),
                                   kind == 'code'), os.path.join(d, 'shard-%d.parquet_%d' % (k, b)))
  return out


def bert_collate(tok, **kw):
  """alignment = the bin size, so that a bin is a padded length"""
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=tok, sequence_length_alignment=BIN, **kw)


class World:
  """the whole table of a directory, every rank's table, where each of its rows lies in the whole, and the counts"""

  def __init__(self, collate, path, world):
    from lddl_amd.loader import load_shards
    self.world = world
    self.whole = load_shards(collate, path)
    self.tables = [load_shards(collate, path, rank=r, world_size=world) for r in range(world)]
    wpart = self.whole.part[:self.whole.n_pairs].cpu().numpy()
    self.to_whole, counts = [], []
    for t in self.tables:
      part = t.part[:t.n_pairs].cpu().numpy()
      m = np.empty(t.n_pairs, np.int64)
      for p in np.unique(part):
        m[part == p] = np.flatnonzero(wpart == p)  # position within the partition: both are in (bin, file) order
      self.to_whole.append(torch.from_numpy(m).to(t.part.device))
      counts.append(np.bincount(t.bins[:t.n_pairs].cpu().numpy(), minlength=t.nbins))
    self.counts = np.stack(counts).astype(np.int64)


_WORLDS = {}


def world_of(tok, dirs, kind, world):
  if (kind, world) not in _WORLDS:
    _WORLDS[kind, world] = World(bert_collate(tok), dirs[kind], world)
  return _WORLDS[kind, world]


def assert_same(a, b, what):
  assert set(a) == set(b), what
  for k in a:
    if torch.is_tensor(a[k]):
      assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (what, k)
    else:
      assert a[k] == b[k], (what, k)


# ---- per-rank tables -------------------------------------------------------------------
@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('kind', ['plain', 'static'])
def test_rank_tables_split_the_whole(tok, dirs, kind, world):
  w = world_of(tok, dirs, kind, world)
  whole = w.whole
  assert whole.n_pairs == N_ROWS and whole.nbins == 4
  assert sum(t.n_pairs for t in w.tables) == N_ROWS
  assert sum(t.n_tokens for t in w.tables) == whole.n_tokens
  seen = []
  for r, t in enumerate(w.tables):
    n = t.n_pairs
    assert t.spans and t.nbins == 4 and t.kind == 'bert' and (t.mlm_token is not None) == (kind == 'static')
    assert sorted(set(t.part[:n].tolist())) == SHARD_IDS[r::world]  # the assigned partitions, by their own numbers
    m = w.to_whole[r]
    for name in ('part', 'bins', 'len0', 'len1', 'flags'):
      assert torch.equal(getattr(t, name)[:n], getattr(whole, name)[m]), name
    assert w.counts[r].tolist() == [sum(BASE[b] + (k < EXTRA[b]) for k in SHARD_IDS[r::world]) for b in range(4)]
    seen.append(m.cpu().numpy())
  assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N_ROWS))
  assert len({tuple(c) for c in w.counts.tolist()}) > 1  # the ranks do not hold the same counts: min_w matters


def test_partitions_must_divide(tok, dirs):
  from lddl_amd.loader import load_shards
  with pytest.raises(ValueError, match=r'6 partitions.*world_size 4'):
    load_shards(bert_collate(tok), dirs['plain'], rank=0, world_size=4)
  with pytest.raises(ValueError, match='together'):
    load_shards(bert_collate(tok), dirs['plain'], rank=0)


# ---- bitwise identity with the single-process loader -----------------------------------
def identity(w, make, batches_kw, route, route_kw=None, modes=(0,), seed=31):
  """every batch of every rank against the same rows of the whole table -> per rank, the batches of the first mode"""
  from lddl_amd.loader import RowBatches
  out = []
  for r, t in enumerate(w.tables):
    kw = dict(batches_kw(r))
    plan = list(RowBatches(t, seed=seed, epoch=1, rank=r, world_size=w.world, **kw))
    assert len(plan) == len(RowBatches(t, seed=seed, epoch=1, rank=r, world_size=w.world, **kw)) > 0
    kept = []
    for mode in modes:
      mine, ref = make(), make()  # the same seed and counter on both sides
      for step, idx in enumerate(plan):
        got = getattr(mine, route)(t, idx, mode=mode, **(route_kw or {}))
        want = getattr(ref, route)(w.whole, w.to_whole[r][idx], mode=mode, **(route_kw or {}))
        assert_same(got, want, (r, mode, step))
        if mode == modes[0]:
          kept.append(got)
    out.append(kept)
  return out


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('kind,modes', [('plain', (0, 2)), ('static', (1,))])
def test_rank_batches_are_the_single_process_loaders(tok, dirs, kind, modes, world):
  w = world_of(tok, dirs, kind, world)
  per_rank = identity(w, lambda: bert_collate(tok, base_seed=5), lambda r: dict(batch_size=8, counts=w.counts),
                      'collate_rows', modes=modes)
  used = w.counts.min(axis=0)
  assert all(len(b) == sum(-(-int(n) // 8) for n in used) for b in per_rank)  # the same steps on every rank
  for step in range(len(per_rank[0])):
    shapes = {tuple(b[step]['input_ids'].shape) for b in per_rank}
    assert len(shapes) == 1, (step, shapes)  # the same rows and the same padded length on every rank
  assert len({b['input_ids'].shape[1] for b in per_rank[0]}) == 4  # one padded length per bin: 16, 32, 48, 64
  assert sum(b['input_ids'].shape[0] for b in per_rank[0]) == int(used.sum())


# ---- token plans -----------------------------------------------------------------------
def fewest_steps(w, seed, max_tokens=256, max_rows=8):
  """what the ranks' all_reduce(MIN) would give for epoch 1, and every rank's own count"""
  from lddl_amd.loader import RowBatches, plan_token_batches_dp
  local = []
  for r, t in enumerate(w.tables):
    lengths = RowBatches(t, max_tokens=max_tokens, max_rows=max_rows, rank=r, world_size=w.world, steps=0).lengths
    local.append(len(plan_token_batches_dp(lengths, r, max_tokens, max_rows, seed, 1)))
  return min(local), local


@pytest.mark.parametrize('world', [2, 3])
def test_token_plans_unpadded(tok, dirs, world):
  w = world_of(tok, dirs, 'plain', world)
  steps, local = fewest_steps(w, 31)
  assert steps > 0
  per_rank = identity(w, lambda: bert_collate(tok, base_seed=5),
                      lambda r: dict(max_tokens=256, max_rows=8, steps=steps), 'collate_rows_unpadded', modes=(0, 2))
  assert all(len(b) == steps for b in per_rank)
  for batches in per_rank:
    assert all(b['input_ids'].numel() <= 256 and b['cu_seqlens'].numel() <= 9 for b in batches)


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('kind,modes', [('plain', (2, 0)), ('static', (1,))])
def test_token_plans_fixed(tok, dirs, kind, modes, world):
  from lddl_amd.loader import fixed_seq_cap
  w = world_of(tok, dirs, kind, world)
  steps, _ = fewest_steps(w, 31)
  shape = dict(max_tokens=256, max_seqs=fixed_seq_cap(256, 8, 64), max_seqlen=64)
  per_rank = identity(w, lambda: bert_collate(tok, base_seed=5, compact_mlm=96),
                      lambda r: dict(max_tokens=256, max_rows=8, steps=steps), 'collate_rows_fixed', shape, modes)
  assert all(len(b) == steps for b in per_rank)
  first = per_rank[0][0]
  for batches in per_rank:  # one shape per tensor, on every rank and at every step
    for b in batches:
      assert {k: tuple(v.shape) for k, v in b.items() if torch.is_tensor(v)} == \
             {k: tuple(v.shape) for k, v in first.items() if torch.is_tensor(v)}
  assert tuple(first['input_ids'].shape) == (256,) and tuple(first['masked_lm_positions'].shape) == (96,)


# ---- dynamic masks -----------------------------------------------------------------------
def test_rank_seeds_give_each_rank_its_own_masks(tok, dirs):
  from lddl_amd.loader import RowBatches, rank_seed
  w = world_of(tok, dirs, 'plain', 2)

  def epoch(seeds):
    out = []
    for r, t in enumerate(w.tables):
      col = bert_collate(tok, base_seed=seeds[r])
      out.append([(col.collate_rows(t, idx, mode=2)['labels'] != -1,
                   col.collate_rows(t, idx, mode=0)['special_tokens_mask'] == 0)
                  for idx in RowBatches(t, 8, seed=3, rank=r, world_size=2, counts=w.counts)])
    return out
  a, b = epoch([rank_seed(1234, 0), rank_seed(1234, 1)])
  assert len(a) == len(b) > 8 and all(x.shape == y.shape for (x, _), (y, _) in zip(a, b))
  full = [(x, y) for (x, _), (y, _) in zip(a, b) if x.numel() >= 128]  # 8 rows of 16 columns at least
  assert len(full) > 8 and all(bool(x.any()) and not torch.equal(x, y) for x, y in full)
  # the draw is keyed by (seed, counter, batch row, column): with one seed a cell that holds an ordinary token on
  # both ranks is picked on both or on neither
  a, b = epoch([1234, 1234])
  for (x, tx), (y, ty) in zip(a, b):
    both = tx & ty
    assert bool(both.any()) and torch.equal(x[both], y[both])


def test_resume_in_the_middle_of_an_epoch(tok, dirs):
  from lddl_amd.loader import RowBatches, rank_seed
  w = world_of(tok, dirs, 'plain', 2)
  t, k = w.tables[1], 5
  kw = dict(seed=3, rank=1, world_size=2, counts=w.counts)
  col = bert_collate(tok, base_seed=rank_seed(1234, 1))
  batches = RowBatches(t, 8, **kw)
  batches.set_epoch(2)
  full = [col.collate_rows(t, idx) for idx in batches]  # mode 2: the table has no static masks
  assert col.counter == len(full) == len(batches) > k + 3
  again = bert_collate(tok, base_seed=rank_seed(1234, 1))  # the restarted job
  again.counter = k
  batches = RowBatches(t, 8, **kw)
  batches.set_epoch(2, start_step=k)
  assert len(batches) == len(full)
  tail = [again.collate_rows(t, idx) for idx in batches]
  assert len(tail) == len(full) - k
  for step, (got, want) in enumerate(zip(tail, full[k:])):
    assert_same(got, want, step)
  assert any(bool((b['labels'] != -1).any()) for b in tail)
  stale = bert_collate(tok, base_seed=rank_seed(1234, 1))  # without the counter the rows are right, the masks are not
  got = stale.collate_rows(t, next(iter(batches)))
  assert torch.equal(got['attention_mask'], full[k]['attention_mask'])
  assert not torch.equal(got['labels'], full[k]['labels'])


# ---- the other loaders -------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['code', 'mlm'])
def test_code_and_mlm_loaders(gpu, tok, dirs, kind):
  from lddl_amd.loader import CodeCollate, MlmCollate
  if kind == 'code':
    base = CodeCollate(device=0, sequence_length_alignment=BIN)
    make = lambda: CodeCollate(tokenizer=base.tok, sequence_length_alignment=BIN, base_seed=5)  # noqa: E731
  else:
    base = MlmCollate(tokenizer=tok, sequence_length_alignment=BIN)
    make = lambda: MlmCollate(tokenizer=tok, sequence_length_alignment=BIN, base_seed=5)  # noqa: E731
  w = World(base, dirs[kind], 2)
  n = sum(11 + 3 * b + (k < 1 + b) for k in range(4) for b in range(2))
  assert w.whole.n_pairs == n == sum(t.n_pairs for t in w.tables)
  assert w.whole.kind == ('codebert' if kind == 'code' else 'mlm')
  assert [sorted(set(t.part[:t.n_pairs].tolist())) for t in w.tables] == [[0, 2], [1, 3]]
  flags = w.whole.flags[:n].cpu().numpy()
  assert bool((flags & 2).any()) == (kind == 'code') and bool(((flags & 2) == 0).any())
  per_rank = identity(w, make, lambda r: dict(batch_size=4, counts=w.counts), 'collate_rows', modes=(0, 2))
  assert len(per_rank[0]) == len(per_rank[1]) == sum(-(-int(c) // 4) for c in w.counts.min(axis=0))
  assert all(x['input_ids'].shape == y['input_ids'].shape for x, y in zip(*per_rank))
  assert 'next_sentence_labels' not in per_rank[0][0]
  steps, _ = fewest_steps(w, 31, 96, None)
  per_rank = identity(w, make, lambda r: dict(max_tokens=96, steps=steps), 'collate_rows_unpadded', modes=(2,))
  assert len(per_rank[0]) == len(per_rank[1]) == steps
