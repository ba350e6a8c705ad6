"""lddl_collate_rows_cu_seqlens + lddl_collate_rows_unpadded
(BertCollate.collate_rows_unpadded): the padding-free batch, held to

* its definition: collate_rows at alignment 1, same seed and counter, with the
  pad columns dropped (input_ids[attention_mask.bool()] ...), bit for bit in
  all three label modes, over the whole range, an index list with a repeated
  row and row0 > 0;
* an independent numpy model over PackResult.rows() that concatenates rows
  instead of padding them (modes 0 and 1);
* hand-made span tables at the shapes where the kernel changes path: rows of
  3 .. 2048 tokens starting and ending at odd and even token offsets, odd span
  offsets, a span ending at the last id, static masks at 1 and n - 2, batches
  of 1 row, 257 rows and more rows than one pass of the grid, outputs at
  16-B-aligned bases and at bases one element off, sentinels around every
  output;
* bad input, which sets an error and never faults or writes out of place;
* the token-budget feed RowBatches(res, max_tokens=...)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 4242
EINVAL, ECAPACITY, EINDEX = -1, -6, -7
TOKEN_KEYS = ('input_ids', 'token_type_ids', 'position_ids')
SENTINEL = -7777
GUARD = 64


def label_key(mode):
  return 'special_tokens_mask' if mode == 0 else 'labels'


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


def collate_for(pk, align=1, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=pk.tok, sequence_length_alignment=align, **kw)


def model(rows, idx, mode, ignore=-1):
  """the padding-free batch in numpy over PackResult.rows(): modes 0 and 1"""
  ids, tt, pos, lab, nsl, cu = [], [], [], [], [], [0]
  for g in idx:
    row = rows[int(g)]
    a, tok = len(row[1]), np.asarray(row[5], np.int64)
    m = len(tok)
    assert m == a + len(row[2]) + 3
    ids.append(tok)
    tt.append((np.arange(m) >= a + 2).astype(np.int64))
    pos.append(np.arange(m, dtype=np.int64))
    if mode == 0:
      lb = np.zeros(m, np.int64)
      lb[[0, a + 1, m - 1]] = 1
    else:
      lb = np.full(m, ignore, np.int64)
      lb[row[6]] = row[7]
    lab.append(lb)
    nsl.append(row[3] & 1)
    cu.append(cu[-1] + m)
  return {'input_ids': np.concatenate(ids), 'token_type_ids': np.concatenate(tt), 'position_ids': np.concatenate(pos),
          label_key(mode): np.concatenate(lab), 'next_sentence_labels': np.asarray(nsl, np.int64),
          'cu_seqlens': np.asarray(cu, np.int32), 'max_seqlen': max(cu[i + 1] - cu[i] for i in range(len(idx)))}


def assert_model(out, exp):
  assert set(out) == set(exp)
  for k, v in exp.items():
    if k == 'max_seqlen':
      assert out[k] == v and isinstance(out[k], int)
      continue
    got = out[k].cpu().numpy() if torch.is_tensor(out[k]) else out[k]
    assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, got.dtype, v.shape)
    assert np.array_equal(got, v), k


def assert_padding_removed(pad, out, mode):
  """out is pad (collate_rows at alignment 1) with the pad columns dropped"""
  m = pad['attention_mask'].bool()
  n, S = m.shape
  for k in ('input_ids', 'token_type_ids', label_key(mode)):
    assert out[k].dtype == torch.int64 and torch.equal(pad[k][m], out[k]), k
  col = torch.arange(S, device=m.device).expand(n, S)
  assert out['position_ids'].dtype == torch.int64 and torch.equal(col[m], out['position_ids'])
  lens = m.sum(1)
  cu = torch.cat([torch.zeros(1, dtype=torch.int64, device=m.device), lens.cumsum(0)]).to(torch.int32)
  assert out['cu_seqlens'].dtype == torch.int32 and torch.equal(out['cu_seqlens'], cu)
  assert out['max_seqlen'] == int(lens.max()) == S and isinstance(out['max_seqlen'], int)
  assert torch.equal(out['next_sentence_labels'], pad['next_sentence_labels'])
  assert set(out) == {'input_ids', 'token_type_ids', 'position_ids', label_key(mode), 'next_sentence_labels',
                      'cu_seqlens', 'max_seqlen'}


# ---- 1. padding removed ------------------------------------------------------
def selections(n):
  rng = np.random.default_rng(3)
  idx = rng.permutation(n)[:41].tolist() + [0, n - 1]
  idx.append(idx[5])  # one repeated row
  idx = [idx[i] for i in rng.permutation(len(idx))]
  return {'all': {}, 'list': {'rows': idx}, 'row0': {'row0': 5, 'n_rows': 37}, 'tail': {'row0': n - 3}}


@pytest.mark.parametrize('masking,mode', [(False, 0), (True, 1), (False, 2)])
@pytest.mark.parametrize('which', ['all', 'list', 'row0', 'tail'])
def test_padding_removed(gpu, masking, mode, which):
  pk, res, _ = packed(masking)
  sel = selections(res.n_pairs)[which]
  a, b = collate_for(pk, base_seed=77), collate_for(pk, base_seed=77)
  a.counter = b.counter = 3
  pad = a.collate_rows(res, mode=mode, **sel)
  out = b.collate_rows_unpadded(res, mode=mode, **sel)
  assert a.counter == b.counter == (3 if mode == 0 else 4)
  assert_padding_removed(pad, out, mode)
  if mode == 2:
    assert bool((out['labels'] != -1).any())  # the comparison is not vacuous
    again = b.collate_rows_unpadded(res, mode=2, **sel)  # the next counter: other draws
    assert not torch.equal(again['labels'], out['labels'])


def test_defaults_and_alignment(gpu):
  """mode defaults as collate_rows; sequence_length_alignment has no effect"""
  pk, res, _ = packed(True)
  one, eight = collate_for(pk, 1), collate_for(pk, 64)
  x, y = one.collate_rows_unpadded(res, row0=0, n_rows=9), eight.collate_rows_unpadded(res, row0=0, n_rows=9)
  assert 'labels' in x and one.counter == 1  # static by default, one count per batch
  for k in x:
    assert x[k] == y[k] if k == 'max_seqlen' else torch.equal(x[k], y[k]), k
  pk, res, _ = packed(False)
  assert 'labels' in collate_for(pk).collate_rows_unpadded(res, [0, 1])  # dynamic by default
  with pytest.raises(ValueError):  # static mode without static masks
    collate_for(pk).collate_rows_unpadded(res, mode=1)
  with pytest.raises(ValueError):
    collate_for(pk).collate_rows_unpadded(res, mode=3)


# ---- 2. independent model -----------------------------------------------------
@pytest.mark.parametrize('masking,mode', [(False, 0), (True, 1)])
def test_against_numpy_model(gpu, masking, mode):
  pk, res, rows = packed(masking)
  assert_model(collate_for(pk, 8).collate_rows_unpadded(res, mode=mode), model(rows, range(res.n_pairs), mode))
  if mode == 1:  # another ignore_index
    out = collate_for(pk, ignore_index=-100).collate_rows_unpadded(res, [3, 1, 2])
    assert_model(out, model(rows, [3, 1, 2], 1, ignore=-100))


# ---- 3. hand-made span tables ---------------------------------------------------
N_IDS = 2101  # odd, so that a span can end at the last id from an odd offset
# (src0, a, src1, b, is_random_next): n = a + b + 3
SHAPES = [
    (0, 0, 0, 0, 1),          # 3: a = b = 0
    (3, 1, 11, 1, 0),         # 5
    (N_IDS - 1, 1, 20, 2, 1),      # 6, A is the last id
    (1, 30, 41, 30, 0),       # 63, both offsets odd
    (0, 31, 100, 30, 1),      # 64
    (7, 31, 101, 31, 0),      # 65
    (9, 62, 201, 62, 1),      # 127
    (3, 60, N_IDS - 65, 65, 1),    # 128, B ends at the last id
    (2, 61, 301, 65, 0),      # 129
    (13, 64, 401, 63, 1),     # 130
    (5, 255, N_IDS - 257, 257, 0),  # 515, B ends at the last id
    (17, 1022, 1041, 1023, 1),     # 2048 = COLLATE_MAX_LEN
]
LENS = [a + b + 3 for _, a, _, b, _ in SHAPES]
ROW515 = LENS.index(515)
SHORT = [g for g, m in enumerate(LENS) if m <= 65]
# every shape; odd-length rows in runs (3 5 63 65 127 129 515), which alternate the parity of the next start
MIXED = [0, 1, 3, 5, 6, 8, 10, 4, 2, 11, 7, 9, 1, 2, 5, 11, 0, 6, 6, 4, 3, 9]


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
  lens = np.asarray(LENS, np.int64)
  assert LENS == [3, 5, 6, 63, 64, 65, 127, 128, 129, 130, 515, 2048]
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


def guarded(n, dtype, dev, off):
  """(whole buffer, its n elements): GUARD sentinels in front and behind;
  off = 0: the n elements start 16-B aligned, off = 1: one element further"""
  whole = torch.full((off + GUARD + n + GUARD + 1,), SENTINEL, dtype=dtype, device=dev)
  assert whole.data_ptr() % 16 == 0
  return whole, whole[off + GUARD:off + GUARD + n]


def guards_intact(whole, n, off):
  return bool((whole[:off + GUARD] == SENTINEL).all()) and bool((whole[off + GUARD + n:] == SENTINEL).all())


P = ctypes.c_void_p


def ptr(t):
  return P(t.data_ptr() if t is not None else 0)


def stream():
  return P(torch.cuda.current_stream().cuda_stream)


def raw_cu(pk, res, rows, n=None, row0=0, cu=None):
  """lddl_collate_rows_cu_seqlens itself: rc, total, max_seqlen"""
  n = rows.numel() if n is None else n
  total, longest = ctypes.c_int64(-5), ctypes.c_int64(-5)
  rc = _lib.lib().lddl_collate_rows_cu_seqlens(pk.tok.handle, ptr(res.len0), ptr(res.len1), ptr(rows), row0, n,
                                               res.n_pairs, ptr(cu), ctypes.byref(total), ctypes.byref(longest),
                                               stream())
  return rc, total.value, longest.value


def raw_fill(pk, res, rows, cu, total, mode, outs, nsl, n=None, seed=31, counter=9):
  """lddl_collate_rows_unpadded itself; outs: input_ids, token_type_ids, position_ids, labels (or None)"""
  n = rows.numel() if n is None else n
  mlm = (res.mlm_off, res.mlm_pos, res.mlm_label, res.mlm_token) if mode == 1 else (None,) * 4
  return _lib.lib().lddl_collate_rows_unpadded(
      pk.tok.handle, ptr(res.ids), ptr(res.src0), ptr(res.src1), ptr(res.len0), ptr(res.len1), ptr(res.flags),
      ptr(rows), 0, n, res.n_pairs, ptr(mlm[0]), ptr(mlm[1]), ptr(mlm[2]), ptr(mlm[3]), ptr(cu), total, mode, -1,
      0.15, seed, counter, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(nsl), stream())


def raw_batch(pk, res, idx, mode, off):
  """both C calls over sentinel-guarded outputs at base offset off; checks the
  guards and returns the batch as collate_rows_unpadded does"""
  dev = res.len0.device
  rows = torch.as_tensor(np.asarray(idx, np.int64)).to(dev)
  n = rows.numel()
  cu_w, cu = guarded(n + 1, torch.int32, dev, off)
  rc, T, longest = raw_cu(pk, res, rows, cu=cu)
  assert rc == 0, _lib.lib().lddl_last_error()
  assert T == sum(LENS[g] for g in idx)
  bufs = [guarded(T, torch.int64, dev, off) for _ in range(4)]
  nsl_w, nsl = guarded(n, torch.int64, dev, off)
  rc = raw_fill(pk, res, rows, cu, T, mode, [b[1] for b in bufs], nsl)
  assert rc == 0, _lib.lib().lddl_last_error()
  assert guards_intact(cu_w, n + 1, off) and guards_intact(nsl_w, n, off)
  assert all(guards_intact(w, T, off) for w, _ in bufs)
  return {'input_ids': bufs[0][1], 'token_type_ids': bufs[1][1], 'position_ids': bufs[2][1],
          label_key(mode): bufs[3][1], 'next_sentence_labels': nsl, 'cu_seqlens': cu, 'max_seqlen': longest}


def check_batch(idx, off):
  pk, res, rows = hand_made()
  for mode in (0, 1):
    assert_model(raw_batch(pk, res, idx, mode, off), model(rows[mode], idx, mode))
  # mode 2: the padded batch at the same seed and counter, pad columns dropped
  col = collate_for(pk, base_seed=31)
  col.counter = 9
  pad = col.collate_rows(res, torch.as_tensor(np.asarray(idx, np.int64)), mode=2)
  assert_padding_removed(pad, raw_batch(pk, res, idx, 2, off), 2)


@pytest.mark.parametrize('off', [0, 1])
def test_one_row_batches(gpu, off):
  _, _, rows = hand_made()
  for g in range(len(SHAPES)):
    if LENS[g] == 2048 and off:
      continue  # below, in the mixed batch
    check_batch([g], off)
    assert rows[1][g][6] == sorted({1, LENS[g] - 2})  # the static masks sit at 1 and n - 2


@pytest.mark.parametrize('off', [0, 1])
def test_mixed_batch_starts_and_ends_at_both_parities(gpu, off):
  shifted = [0] + MIXED  # a 3-token row in front: every start changes parity
  seen = {}
  for batch in (MIXED, shifted):
    starts = np.concatenate([[0], np.cumsum([LENS[g] for g in batch])])[:-1]
    for s, g in zip(starts, batch):
      seen.setdefault(g, set()).add(int(s) & 1)
  # every shape starts at an odd and at an even token (so each ends at both, too), its static masks with it
  assert seen == {g: {0, 1} for g in range(len(SHAPES))}
  check_batch(MIXED, off)
  check_batch(shifted, off)


@pytest.mark.parametrize('off', [0, 1])
def test_257_rows(gpu, off):
  idx = [SHORT[i % len(SHORT)] for i in range(253)] + [7, 8, ROW515, 9]
  assert len(idx) == 257
  check_batch(idx, off)


@pytest.mark.parametrize('off', [0, 1])
def test_more_rows_than_one_pass_of_the_grid(gpu, off):
  """the fill grid is capped at 8 blocks of 4 rows per CU: beyond that a wave
  takes several rows; the offsets pass runs several chunks"""
  pk, res, rows = hand_made()
  n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 5
  idx = np.asarray(SHORT)[np.random.default_rng(1).integers(0, len(SHORT), n)].tolist()
  for mode in (0, 1):
    assert_model(raw_batch(pk, res, idx, mode, off), model(rows[mode], idx, mode))


# ---- 4. bad input ---------------------------------------------------------------
def still_good(col, res, rows):
  n = res.n_pairs
  assert_model(col.collate_rows_unpadded(res, [0, n - 1, 1], mode=0), model(rows, [0, n - 1, 1], 0))


def test_row_index_out_of_range(gpu):
  pk, res, rows = packed(False)
  col = collate_for(pk)
  n = res.n_pairs
  dev = res.len0.device
  for bad in (-1, n, n + 12345, -(1 << 40), 1 << 40):
    with pytest.raises(IndexError):
      col.collate_rows_unpadded(res, [1, bad, 2], mode=0)
    still_good(col, res, rows)
    idx = torch.tensor([1, bad, 2], dtype=torch.int64, device=dev)
    rc, _, _ = raw_cu(pk, res, idx, cu=torch.zeros(4, dtype=torch.int32, device=dev))
    assert rc == EINDEX
    # the fill kernel's own check: offsets that give the bad row no tokens
    l1, l2 = len(rows[1][5]), len(rows[2][5])
    cu = torch.tensor([0, l1, l1, l1 + l2], dtype=torch.int32, device=dev)
    bufs = [guarded(l1 + l2, torch.int64, dev, 0) for _ in range(4)]
    nsl_w, nsl = guarded(3, torch.int64, dev, 0)
    rc = raw_fill(pk, res, idx, cu, l1 + l2, 0, [b[1] for b in bufs], nsl)
    assert rc == EINDEX, rc
    assert all(guards_intact(w, l1 + l2, 0) for w, _ in bufs) and int(nsl[1]) == SENTINEL
    exp = model(rows, [1, 2], 0)
    assert np.array_equal(bufs[0][1].cpu().numpy(), exp['input_ids'])  # the rows around it are right
    still_good(col, res, rows)
  with pytest.raises(IndexError):  # a range past the end
    col.collate_rows_unpadded(res, row0=n - 2, n_rows=3, mode=0)
  still_good(col, res, rows)


def codebert_result():
  """a CodeBERT pack of pre-tokenised documents, every other one without docstring"""
  from lddl_amd import pipeline
  docs = [[[5, 6, 7], [8, 9, 10, 11]], [[12] * 9, [13] * 5, [14] * 6]] * 6
  sents = [s for d in docs for s in d]
  ntok = np.asarray([len(s) for s in sents], np.int32)
  off = np.concatenate([[0], np.cumsum(ntok)]).astype(np.int64)
  ids = np.asarray([t for s in sents for t in s] + [0] * 16, np.uint16)
  dso = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
  dev = 'cuda'
  sh = pipeline.ShardSet(torch.zeros(int(off[-1]) + 16, dtype=torch.uint8, device=dev), torch.from_numpy(off).to(dev),
                         torch.from_numpy(dso).to(dev), torch.tensor([0, len(docs)], dtype=torch.int64, device=dev),
                         torch.tensor([0, 1] * 6, dtype=torch.int32, device=dev), int(off[-1]))
  cpk = pipeline.Packer(_lib.VOCAB_CODEBERT, 0)
  res = cpk.pack(sh, torch.from_numpy(ids.view(np.int16)).to(dev), torch.from_numpy(ntok).to(dev),
                 target_seq_length=64, duplicate_factor=2, seed=3, codebert=True, spans=True)
  return cpk, res


def test_codebert_rows_are_refused(gpu):
  cpk, res = codebert_result()
  flags = res.flags[:res.n_pairs].cpu().numpy()
  assert res.n_pairs > 0 and bool(((flags & 2) == 0).any())
  col = collate_for(cpk)
  with pytest.raises(RuntimeError, match='CodeBERT'):
    col.collate_rows_unpadded(res, mode=0)
  with_doc = np.flatnonzero(flags & 2)
  assert len(with_doc)  # rows with the [SEP] collate, and the ctx still works
  assert_model(col.collate_rows_unpadded(res, with_doc.tolist(), mode=0), model(res.rows(), with_doc, 0))


def test_static_position_equal_to_row_length(gpu):
  pk, res, rows = hand_made()
  col = collate_for(pk)
  keep = res.mlm_pos.clone()
  g = 3  # 63 tokens; its masks are entries off[g], off[g] + 1
  k = int(res.mlm_off[g].item()) + 1
  try:
    res.mlm_pos[k] = LENS[g]  # a column of the padded row (next to a longer one), the next row's token here
    assert col.collate_rows(res, [g, 4], mode=1)['input_ids'].shape == (2, 64)  # the padded call takes it
    with pytest.raises(IndexError):
      col.collate_rows_unpadded(res, [g, 4], mode=1)
  finally:
    res.mlm_pos.copy_(keep)
  assert_model(col.collate_rows_unpadded(res, [g, 4], mode=1), model(rows[1], [g, 4], 1))


def test_total_and_cu_seqlens_are_checked(gpu):
  pk, res, rows = hand_made()
  dev = res.len0.device
  idx = [3, 1, 5, 4, 2]
  rows_t = torch.tensor(idx, dtype=torch.int64, device=dev)
  cu = torch.empty(len(idx) + 1, dtype=torch.int32, device=dev)
  rc, T, longest = raw_cu(pk, res, rows_t, cu=cu)
  assert rc == 0 and T == sum(LENS[g] for g in idx) and longest == 65
  exp = model(rows[0], idx, 0)
  h = exp['cu_seqlens']

  def run(cu_dev, total):
    bufs = [guarded(T, torch.int64, dev, 0) for _ in range(4)]
    nsl_w, nsl = guarded(len(idx), torch.int64, dev, 0)
    rc = raw_fill(pk, res, rows_t, cu_dev, total, 0, [b[1] for b in bufs], nsl)
    assert all(guards_intact(w, T, 0) for w, _ in bufs) and guards_intact(nsl_w, len(idx), 0)
    return rc, [b[1].cpu().numpy() for b in bufs]

  # total one less than T: the last row does not fit and is left unwritten
  rc, outs = run(cu, T - 1)
  assert rc == EINVAL and 'cu_seqlens' in _lib.lib().lddl_last_error().decode()
  for o, k in zip(outs, ('input_ids', 'token_type_ids', 'position_ids', 'special_tokens_mask')):
    assert np.array_equal(o[:h[-2]], exp[k][:h[-2]]) and bool((o[h[-2]:] == SENTINEL).all()), k
  rc, outs = run(cu, T)
  assert rc == 0 and np.array_equal(outs[0], exp['input_ids'])
  # one entry altered by 1 on the host: the rows on both sides of it no longer hold their tokens
  for delta in (1, -1):
    bad = h.copy()
    bad[2] += delta
    rc, outs = run(torch.from_numpy(bad).to(dev), T)
    assert rc == EINVAL
    for o, k in zip(outs, ('input_ids', 'token_type_ids', 'position_ids', 'special_tokens_mask')):
      assert bool((o[h[1]:h[3]] == SENTINEL).all()), k  # rows 1 and 2 unwritten
      assert np.array_equal(o[:h[1]], exp[k][:h[1]]) and np.array_equal(o[h[3]:], exp[k][h[3]:]), k
  neg = h.copy()
  neg[0] = -1
  rc, outs = run(torch.from_numpy(neg).to(dev), T)
  assert rc == EINVAL and bool((outs[0][:h[1]] == SENTINEL).all())
  rc, outs = run(cu, T)  # and right again on the same ctx
  assert rc == 0
  for o, k in zip(outs, ('input_ids', 'token_type_ids', 'position_ids', 'special_tokens_mask')):
    assert np.array_equal(o, exp[k]), k


def test_bad_arguments(gpu):
  pk, res, rows = hand_made()
  dev = res.len0.device
  col = collate_for(pk)
  idx = torch.tensor([1, 2], dtype=torch.int64, device=dev)
  cu = torch.empty(3, dtype=torch.int32, device=dev)
  rc, T, _ = raw_cu(pk, res, idx, cu=cu)
  assert rc == 0 and T == 11
  outs = [torch.full((T,), SENTINEL, dtype=torch.int64, device=dev) for _ in range(4)]
  nsl = torch.full((2,), SENTINEL, dtype=torch.int64, device=dev)
  assert raw_fill(pk, res, idx, cu, T, 3, outs, nsl) == EINVAL  # mode 3
  assert raw_fill(pk, res, idx, cu, T, -1, outs, nsl) == EINVAL
  for k in range(4):  # null outputs
    assert raw_fill(pk, res, idx, cu, T, 0, [None if i == k else o for i, o in enumerate(outs)], nsl) == EINVAL
  assert raw_fill(pk, res, idx, cu, T, 0, outs, None) == EINVAL
  assert raw_fill(pk, res, idx, None, T, 0, outs, nsl) == EINVAL
  assert raw_fill(pk, res, idx, cu, -1, 0, outs, nsl) == EINVAL
  assert raw_fill(pk, res, idx, cu, 1 << 31, 0, outs, nsl) == ECAPACITY
  assert raw_cu(pk, res, idx, cu=None)[0] == EINVAL
  # n_rows = 0: no max() of an empty batch; the fill call has nothing to do
  assert raw_cu(pk, res, idx, n=0, cu=cu)[0] == EINVAL
  assert raw_fill(pk, res, idx, cu, T, 0, outs, nsl, n=0) == 0
  assert all(bool((o == SENTINEL).all()) for o in outs + [nsl])  # nothing was written by any of these
  for empty in ([], torch.zeros(0, dtype=torch.int64, device=dev)):
    with pytest.raises(ValueError):
      col.collate_rows_unpadded(res, empty)
  with pytest.raises(ValueError):
    col.collate_rows_unpadded(res, row0=res.n_pairs, mode=0)
  assert raw_fill(pk, res, idx, cu, T, 0, outs, nsl) == 0
  assert np.array_equal(outs[0].cpu().numpy(), model(rows[0], [1, 2], 0)['input_ids'])


def test_2_to_the_31_tokens_are_refused(gpu):
  """the offsets call alone over an index list that repeats a 515-token row
  past 2^31 tokens: summed in 64 bits, refused before anything is narrowed"""
  pk, res, rows = hand_made()
  dev = res.len0.device
  n = (1 << 31) // 515 + 1
  assert n * 515 >= 1 << 31 > (n - 1) * 515
  idx = torch.full((n,), ROW515, dtype=torch.int64, device=dev)
  cu = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=dev)
  rc, _, _ = raw_cu(pk, res, idx, cu=cu)
  assert rc == ECAPACITY, rc
  assert bool((cu[1:] == SENTINEL).all())  # no narrowed offsets
  rc, T, longest = raw_cu(pk, res, idx[:n - 1], cu=cu)  # one row fewer fits
  assert rc == 0 and T == (n - 1) * 515 and longest == 515
  assert int(cu[n - 1]) == T and int(cu[n]) == SENTINEL
  step = cu[1:n].to(torch.int64) - cu[:n - 1].to(torch.int64)
  assert bool((step == 515).all())
  still_good_hand = collate_for(pk).collate_rows_unpadded(res, [1, 2], mode=0)
  assert_model(still_good_hand, model(rows[0], [1, 2], 0))


# ---- 5. token-budget batches ---------------------------------------------------
def test_token_budget_feed(gpu):
  from lddl_amd.loader import RowBatches
  pk, res, rows = packed(True)
  col = collate_for(pk)
  batches = RowBatches(res, max_tokens=2048, seed=1, epoch=0)
  seen = []
  for idx in batches:
    assert idx.is_cuda and idx.dtype == torch.int64
    out = col.collate_rows_unpadded(res, idx)
    cu = out['cu_seqlens'].cpu().numpy()
    ids = out['input_ids'].cpu().numpy()
    assert 0 < cu[-1] <= 2048 and len(ids) == cu[-1]
    for r, g in enumerate(idx.cpu().tolist()):
      seen.append((g, tuple(ids[cu[r]:cu[r + 1]].tolist())))
  assert sorted(seen) == sorted((g, tuple(row[5])) for g, row in enumerate(rows))
  assert col.counter == len(batches) >= sum(len(r[5]) for r in rows) / 2048
  few = RowBatches(res, max_tokens=2048, max_rows=3)
  assert max(len(b) for b in few.plan()) == 3
