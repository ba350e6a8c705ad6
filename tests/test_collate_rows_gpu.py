"""lddl_collate_rows (BertCollate.collate_rows): training batches straight from
a pack result's spans, against

* the parquet route on the same rows (writer.write_shards -> read back ->
  lddl_collate_bert): every tensor equal, all three label modes;
* an independent numpy model of bert.py:69-153 over the host copy of the rows
  (PackResult.rows());
* mode 0 followed by lddl_mask_tokens (mode 2 is that, fused);

over a small synthetic corpus and over hand-made span tables that put rows at
the shapes where the kernel changes path: 63 / 64 / 65 / 128 / 129 / 512
columns (odd lengths take the 8-B store path at alignment 1, even ones the
16-B path), a = b = 1, odd span offsets, a span that ends at the last id,
static masks at positions 1 and n - 2, one row, 257 rows, and more rows than
one pass of the grid.  Bad input sets the error word and never faults."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 4242
KEYS = ('input_ids', 'token_type_ids', 'attention_mask', 'next_sentence_labels')


@functools.lru_cache(maxsize=None)
def packed(masking):
  """(packer, result, host rows) of a few hundred sentences: 3 partitions, seq 128, bin 32, dup 2"""
  from lddl_amd import pipeline, synth
  c = synth.make_wiki(40_000, seed=SEED)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0, masking=masking)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 3), torch.device('cuda', 0))
  res = pk.run(sh, target_seq_length=128, bin_size=32, duplicate_factor=2, seed=SEED, masking=masking, spans=True)
  torch.cuda.synchronize()
  assert res.spans and 100 < res.n_pairs < 5000
  return pk, res, res.rows()


def collate_for(pk, align=8, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=pk.tok, sequence_length_alignment=align, **kw)


@functools.lru_cache(maxsize=None)
def full_range(masking, mode, align):
  """collate_rows over every row (shared by the tests; not modified)"""
  pk, res, _ = packed(masking)
  return collate_for(pk, align, base_seed=77).collate_rows(res, mode=mode)


def label_key(mode):
  return 'special_tokens_mask' if mode == 0 else 'labels'


def model(rows, idx, align, mode, ignore=-1):
  """bert.py:69-153 in numpy over PackResult.rows(): modes 0 and 1"""
  idx = [int(g) for g in idx]
  S = max(len(rows[g][5]) for g in idx)
  S = ((S - 1) // align + 1) * align
  n = len(idx)
  out = {k: np.zeros((n, S), np.int64) for k in KEYS[:3]}
  out['next_sentence_labels'] = np.zeros(n, np.int64)
  lab = np.zeros((n, S), np.int64) if mode == 0 else np.full((n, S), ignore, np.int64)
  for r, g in enumerate(idx):
    row = rows[g]
    a, tok = len(row[1]), row[5]
    m = len(tok)
    assert m == a + len(row[2]) + 3
    out['input_ids'][r, :m] = tok
    out['token_type_ids'][r, a + 2:m] = 1
    out['attention_mask'][r, :m] = 1
    out['next_sentence_labels'][r] = row[3] & 1
    if mode == 0:
      lab[r, 0] = lab[r, a + 1] = 1
      lab[r, m - 1:] = 1
    else:
      lab[r, row[6]] = row[7]
  out[label_key(mode)] = lab
  return out


def assert_model(out, exp):
  assert set(out) == set(exp)
  for k, v in exp.items():
    got = out[k].cpu().numpy()
    assert got.shape == v.shape and got.dtype == np.int64, (k, got.shape, v.shape)
    assert np.array_equal(got, v), k


def assert_same(a, b):
  assert set(a) == set(b)
  for k in a:
    assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ---- 1. memory equals disk ---------------------------------------------------
@pytest.mark.parametrize('masking', [False, True])
def test_memory_equals_disk(gpu, tmp_path, masking):
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd import writer
  pk, res, _ = packed(masking)
  writer.write_shards(pk, res, str(tmp_path), bin_size=32, masking=masking)
  table = pa.concat_tables([pq.read_table(os.path.join(str(tmp_path), 'part.%d.parquet_%d' % (p, b)))
                            for p in range(3) for b in range(res.nbins)])
  assert table.num_rows == res.n_pairs
  for align in (1, 8, 64):
    if masking:
      disk = collate_for(pk, align).collate_arrow(table)
      assert_same(disk, full_range(True, 1, align))
      assert 'labels' in disk and bool((disk['labels'] != -1).any())
      continue
    d = table.to_pydict()
    enc = collate_for(pk, align).to_encoded_inputs(list(zip(d['A'], d['B'], d['is_random_next'])))
    assert_same(enc, full_range(False, 0, align))
    dyn = collate_for(pk, align, base_seed=77).collate_arrow(table)
    mem = full_range(False, 2, align)
    assert_same(dyn, mem)
    assert bool((mem['labels'] != -1).any())


# ---- 2. index list -----------------------------------------------------------
@pytest.mark.parametrize('masking,mode', [(False, 0), (True, 1)])
@pytest.mark.parametrize('as_tensor', [False, True])
def test_index_list(gpu, masking, mode, as_tensor):
  pk, res, rows = packed(masking)
  n = res.n_pairs
  rng = np.random.default_rng(3)
  idx = rng.permutation(n)[:41].tolist() + [0, n - 1]
  idx.append(idx[5])  # one repeated row
  idx = [idx[i] for i in rng.permutation(len(idx))]
  full = full_range(masking, mode, 8)
  arg = torch.tensor(idx, dtype=torch.int64, device=gpu) if as_tensor else idx
  out = collate_for(pk, 8).collate_rows(res, arg, mode=mode)
  S = out['input_ids'].shape[1]
  assert S == (max(len(rows[g][5]) for g in idx) + 7) // 8 * 8
  pick = torch.tensor(idx, dtype=torch.int64, device=gpu)
  pad = {'input_ids': 0, 'token_type_ids': 0, 'attention_mask': 0, 'special_tokens_mask': 1, 'labels': -1}
  for k in out:
    want = full[k][pick]
    if want.dim() == 2:
      assert bool((want[:, S:] == pad[k]).all()), k  # what the re-padding drops is padding
      want = want[:, :S]
    assert torch.equal(out[k], want), k


def test_row_range(gpu):
  pk, res, _ = packed(False)
  full = full_range(False, 0, 8)
  out = collate_for(pk, 8).collate_rows(res, row0=5, n_rows=37, mode=0)
  S = out['input_ids'].shape[1]
  for k in out:
    want = full[k][5:42]
    assert torch.equal(out[k], want[:, :S] if want.dim() == 2 else want), k
  tail = collate_for(pk, 8).collate_rows(res, row0=res.n_pairs - 3, mode=0)
  assert tail['input_ids'].shape[0] == 3 and torch.equal(tail['next_sentence_labels'], full['next_sentence_labels'][-3:])


# ---- 3. independent checker --------------------------------------------------
@pytest.mark.parametrize('masking,mode', [(False, 0), (True, 1)])
@pytest.mark.parametrize('align', [1, 8])
def test_against_numpy_model(gpu, masking, mode, align):
  pk, res, rows = packed(masking)
  assert_model(full_range(masking, mode, align), model(rows, range(res.n_pairs), align, mode))
  if mode == 1:  # another ignore_index
    out = collate_for(pk, align, ignore_index=-100).collate_rows(res, [3, 1, 2])
    assert_model(out, model(rows, [3, 1, 2], align, 1, ignore=-100))


# ---- 4. mode 2 ---------------------------------------------------------------
def test_mode2_is_mode0_then_mask_tokens(gpu):
  pk, res, _ = packed(False)
  col = collate_for(pk, 8, base_seed=99)
  col.counter = 5
  fused = col.collate_rows(res)  # no static masks: dynamic by default
  assert col.counter == 6
  enc = col.collate_rows(res, mode=0)
  assert col.counter == 6  # mode 0 draws nothing
  ids, labels = col.mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], counter=5)
  assert torch.equal(fused['input_ids'], ids) and torch.equal(fused['labels'], labels)
  for k in KEYS[1:]:
    assert torch.equal(fused[k], enc[k]), k
  again = col.collate_rows(res)
  assert col.counter == 7 and not torch.equal(again['labels'], fused['labels'])


def test_mode2_probability_edges(gpu):
  pk, res, _ = packed(False)
  z = collate_for(pk, 8, mlm_probability=0.0).collate_rows(res)
  assert bool((z['labels'] == -1).all())
  one = collate_for(pk, 8, mlm_probability=1.0)
  enc = one.collate_rows(res, mode=0)
  full = one.collate_rows(res)
  assert torch.equal(full['labels'] != -1, enc['special_tokens_mask'] == 0)


def test_static_default_and_counter(gpu):
  pk, res, _ = packed(True)
  col = collate_for(pk, 8)
  out = col.collate_rows(res, row0=0, n_rows=4)
  assert 'labels' in out and col.counter == 1  # static by default, one count per batch as __call__


# ---- 5. smallest shapes that can go wrong --------------------------------------
N_IDS = 601  # odd, so that a span can end at the last id from an odd offset
# (src0, a, src1, b, is_random_next): n = a + b + 3
SHAPES = [
    (1, 30, 41, 30, 0),      # 63, both offsets odd
    (0, 31, 100, 30, 1),     # 64
    (7, 31, 101, 31, 0),     # 65
    (3, 60, N_IDS - 65, 65, 1),   # 128, B ends at the last id
    (2, 61, 301, 65, 0),     # 129
    (N_IDS - 1, 1, 11, 1, 1),     # a = b = 1, A is the last id
    (5, 254, 346, 255, 0),   # 512, B ends at the last id
    (9, 1, 20, 40, 1),
    (10, 40, 55, 1, 0),
]
ROW512 = 6
SHORT = [0, 1, 2, 5, 7, 8]  # rows of at most 65 columns


@functools.lru_cache(maxsize=None)
def hand_made():
  """a PackResult over hand-made ids and span tables, with static masks at
  positions 1 and n - 2 of every row (one position when they coincide)"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  ids = np.concatenate([1000 + np.arange(N_IDS), np.zeros(16, np.int64)]).astype(np.uint16)
  sp = np.asarray(SHAPES, np.int64)
  n = len(SHAPES)
  lens = sp[:, 1] + sp[:, 3] + 3
  assert sorted(lens.tolist())[-6:] == [63, 64, 65, 128, 129, 512]
  assert all(s0 + a <= N_IDS and s1 + b <= N_IDS for s0, a, s1, b, _ in SHAPES)
  pos, off = [], [0]
  for m in lens:
    pos.extend(sorted({1, int(m) - 2}))
    off.append(len(pos))
  pos = np.asarray(pos, np.uint16)
  lab = (2000 + np.arange(len(pos))).astype(np.uint16)
  tok = np.where(np.arange(len(pos)) % 3 == 0, 3000 + np.arange(len(pos)), pk.tok.mask_id).astype(np.uint16)

  def t(a, dt=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.astype(dt or a.dtype)).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t(sp[:, 1].astype(np.uint16)), t(sp[:, 3].astype(np.uint16)), t((sp[:, 4] | 2).astype(np.uint8)),
      t(np.zeros(n, np.uint8)), t(np.zeros(n, np.int64)), t(np.asarray([[n]], np.int64)))
  res.ids, res.src0, res.src1 = t(ids), t(sp[:, 0]), t(sp[:, 2])
  res.cls_id, res.sep_id = pk.tok.cls_id, pk.tok.sep_id
  plain = res.rows()  # before the masks are attached: what mode 0 / 2 collate
  res.n_masked, res.mlm_off = len(pos), t(np.asarray(off, np.int64))
  res.mlm_pos, res.mlm_label, res.mlm_token = t(pos), t(lab), t(tok)
  return pk, res, (plain, res.rows())


def check_batch(pk, res, rows, idx, align, seq=None):
  for mode in (0, 1):
    out = collate_for(pk, align).collate_rows(res, idx, mode=mode)
    if seq is not None:
      assert out['input_ids'].shape[1] == seq
    assert_model(out, model(rows[mode], idx, align, mode))
  col = collate_for(pk, align, base_seed=31)
  col.counter = 9
  fused = col.collate_rows(res, idx, mode=2)
  enc = col.collate_rows(res, idx, mode=0)
  ids, labels = col.mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], counter=9)
  assert torch.equal(fused['input_ids'], ids) and torch.equal(fused['labels'], labels)


@pytest.mark.parametrize('g', range(len(SHAPES)))
def test_one_row_batches(gpu, g):
  """a batch of one row at alignment 1: seq_len = the row's own length"""
  pk, res, rows = hand_made()
  s0, a, s1, b, _ = SHAPES[g]
  check_batch(pk, res, rows, [g], 1, seq=a + b + 3)
  assert rows[1][g][6] == sorted({1, a + b + 1})  # the static masks sit at 1 and n - 2


def test_row_of_512_is_not_padded_further(gpu):
  pk, res, rows = hand_made()
  for align in (8, 64, 512):
    check_batch(pk, res, rows, list(range(len(SHAPES))), align, seq=512)
  check_batch(pk, res, rows, [0, 4, 2], 8, seq=136)  # 129 -> 136
  check_batch(pk, res, rows, [0, 1], 64, seq=64)


def test_257_rows(gpu):
  pk, res, rows = hand_made()
  idx = [SHORT[i % len(SHORT)] for i in range(255)] + [3, 4]
  check_batch(pk, res, rows, idx, 1, seq=129)  # odd seq_len: odd rows are 8-B aligned only
  check_batch(pk, res, rows, idx, 8, seq=136)


def test_more_rows_than_one_pass_of_the_grid(gpu):
  """the grid is capped at 8 blocks of 4 rows per CU: beyond that a wave takes several rows"""
  pk, res, rows = hand_made()
  n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4 + 5
  idx = np.asarray(SHORT)[np.random.default_rng(1).integers(0, len(SHORT), n)]
  for mode in (0, 1):
    out = collate_for(pk, 8).collate_rows(res, torch.from_numpy(idx).to(gpu), mode=mode)
    small = model(rows[mode], SHORT, 8, mode)
    where = np.searchsorted(SHORT, idx)
    for k, v in small.items():
      assert np.array_equal(out[k].cpu().numpy(), v[where]), k


def test_seq_512_pack(gpu):
  """ids built by hand through Packer.pack at seq 512: documents of two
  sentences whose pair fills the row exactly"""
  from test_pack_gpu import shards_from_docs
  from lddl_amd import pipeline
  rng = np.random.default_rng(5)
  docs = [[rng.integers(1000, 30000, a).tolist(), rng.integers(1000, 30000, 509 - a).tolist()]
          for a in (254, 1, 508, 300)] * 3
  docs += [[rng.integers(1000, 30000, 7).tolist(), rng.integers(1000, 30000, 9).tolist()]] * 4
  sh, ids, ntok = shards_from_docs(docs)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  res = pk.pack(sh, ids, ntok, target_seq_length=512, short_seq_prob=0.0, duplicate_factor=2, seed=SEED, bin_size=64,
                spans=True)
  rows = res.rows()
  assert max(len(r[5]) for r in rows) == 512
  for align in (8, 64):
    for mode in (0, 2):
      out = collate_for(pk, align).collate_rows(res, mode=mode)
      assert out['input_ids'].shape == (res.n_pairs, 512)
    assert_model(collate_for(pk, align).collate_rows(res, mode=0), model(rows, range(res.n_pairs), align, 0))


# ---- 6. errors ---------------------------------------------------------------
def raw_collate(col, res, idx, seq_len, mode=0):
  """lddl_collate_rows itself, with a seq_len of the caller's choosing"""
  dev = res.len0.device
  rows = torch.tensor(idx, dtype=torch.int64, device=dev)
  n = rows.numel()
  out = torch.zeros((4, n, seq_len), dtype=torch.int64, device=dev)
  nsl = torch.zeros(n, dtype=torch.int64, device=dev)
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  rc = _lib.lib().lddl_collate_rows(col.tok.handle, p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1),
                                    p(res.flags), p(rows), 0, n, res.n_pairs, P(0), P(0), P(0), P(0), seq_len, mode,
                                    -1, 0.15, 1, 0, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(nsl),
                                    P(torch.cuda.current_stream().cuda_stream))
  return rc, out


def test_errors_leave_the_ctx_usable(gpu):
  from lddl_amd import pipeline
  pk, res, rows = packed(False)
  col = collate_for(pk, 8)
  n = res.n_pairs
  good = full_range(False, 0, 8)

  def still_good():
    out = col.collate_rows(res, [0, n - 1], mode=0)
    S = out['input_ids'].shape[1]
    pick = torch.tensor([0, n - 1], device=gpu)
    assert torch.equal(out['input_ids'], good['input_ids'][pick][:, :S])

  for bad in (-1, n, n + 12345, -(1 << 40), 1 << 40):
    with pytest.raises(IndexError):
      col.collate_rows(res, [1, bad, 2], mode=0)
    still_good()
    # the fill kernel's own bounds check (the length pass is skipped)
    rc, out = raw_collate(col, res, [1, bad, 2], 128)
    assert rc == -7, rc  # LDDL_EINDEX
    assert bool((out[:, 1] == 0).all())  # the bad row was not written
    still_good()
  with pytest.raises(IndexError):  # a range past the end
    col.collate_rows(res, row0=n - 2, n_rows=3, mode=0)
  still_good()
  longest = int(np.argmax([len(r[5]) for r in rows]))
  rc, _ = raw_collate(col, res, [0, longest], len(rows[longest][5]) - 1)
  assert rc == -6, rc  # LDDL_ECAPACITY
  assert 'longer than seq_len' in _lib.lib().lddl_last_error().decode()
  still_good()
  rc, _ = raw_collate(col, res, [0, longest], len(rows[longest][5]))
  assert rc == 0
  rc, _ = raw_collate(col, res, [0], 2049)
  assert rc == -6  # wider than COLLATE_MAX_LEN
  for empty in ([], torch.zeros(0, dtype=torch.int64, device=gpu)):
    with pytest.raises(ValueError):
      col.collate_rows(res, empty)
  with pytest.raises(ValueError):
    col.collate_rows(res, row0=n, mode=0)
  with pytest.raises(ValueError):  # static mode without static masks
    col.collate_rows(res, mode=1)
  still_good()
  # a materialised result has no spans
  c = pipeline.Packer(_lib.VOCAB_BERT, 0)
  from test_pack_gpu import shards_from_docs
  sh, ids, ntok = shards_from_docs([[[5, 6, 7], [8, 9]], [[10] * 40, [11] * 30]])
  mat = c.pack(sh, ids, ntok, target_seq_length=64, duplicate_factor=1, seed=7)
  with pytest.raises(ValueError):
    collate_for(c).collate_rows(mat)
  still_good()


def test_static_position_out_of_range(gpu):
  pk, res, rows = hand_made()
  col = collate_for(pk, 1)
  keep = res.mlm_pos.clone()
  try:
    res.mlm_pos[1] = 63  # row 0 has 63 columns: position 63 is one past its batch of one
    with pytest.raises(IndexError):
      col.collate_rows(res, [0], mode=1)
  finally:
    res.mlm_pos.copy_(keep)
  assert_model(col.collate_rows(res, [0], mode=1), model(rows[1], [0], 1, 1))


def test_codebert_rows_are_refused(gpu):
  from test_pack_gpu import shards_from_docs
  from lddl_amd import pipeline
  docs = [[[5, 6, 7], [8, 9, 10, 11]], [[12] * 9, [13] * 5, [14] * 6]] * 6
  sh, ids, ntok = shards_from_docs(docs, nseg=[0, 1] * 6)  # every other document has no docstring
  cpk = pipeline.Packer(_lib.VOCAB_CODEBERT, 0)
  res = cpk.pack(sh, ids, ntok, target_seq_length=64, duplicate_factor=2, seed=3, codebert=True, spans=True)
  flags = res.flags[:res.n_pairs].cpu().numpy()
  assert res.n_pairs > 0 and bool(((flags & 2) == 0).any())
  col = collate_for(cpk)
  with pytest.raises(RuntimeError, match='CodeBERT'):
    col.collate_rows(res, mode=0)
  with_doc = np.flatnonzero(flags & 2)
  if len(with_doc):  # rows with the [SEP] collate, and the ctx still works
    out = col.collate_rows(res, with_doc.tolist(), mode=0)
    assert_model(out, model(res.rows(), with_doc, 8, 0))


# ---- the feed ------------------------------------------------------------------
def test_row_batches_feed(gpu):
  from lddl_amd.loader import RowBatches
  pk, res, rows = packed(True)
  col = collate_for(pk, 8)
  bins = res.bins[:res.n_pairs].cpu().numpy()
  seen = []
  batches = RowBatches(res, 64, seed=1, epoch=0)
  for idx in batches:
    assert idx.is_cuda and idx.dtype == torch.int64
    h = idx.cpu().numpy()
    assert len(set(bins[h])) == 1
    batch = col.collate_rows(res, idx)
    b = int(bins[h[0]])
    S = batch['input_ids'].shape[1]
    assert batch['input_ids'].shape[0] == len(h) and 32 * b < S <= 32 * (b + 1)  # padded length tracks the bin
    seen.extend(h.tolist())
  assert sorted(seen) == list(range(res.n_pairs))
  assert col.counter == len(batches) >= res.n_pairs / 64
