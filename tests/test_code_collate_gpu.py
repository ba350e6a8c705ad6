"""CodeCollate on the GPU: lddl_collate_code_rows[_seq_len],
lddl_collate_code_rows_cu_seqlens / _unpadded and lddl_code_rows_from_strings[_len],
held to the numpy model of tests/code_collate_model.py (built from
PackResult.rows() and tests/mask_model.py, never from a kernel's output).
Every comparison is exact.

1. a hand-made row table over the CodeBERT vocabulary: the three regimes
   (s = 0; s = 1, a = 0; s = 1, a > 0) at row lengths 3 .. 130 around the wave
   and pair boundaries, padded at alignment 8 and at alignment 1 with an odd
   seq_len, into outputs whose base is 8 bytes off, through a row list with
   repeats in reversed order and through row0 / n_rows, modes 0 and 2;
2. the padding-free batch against the padded one and against the model, once
   over more rows than one chunk of the offsets scan;
3. bad input, one call each, between guard words;
4. a CodeBERT pack with spans, and BertCollate on its rows that have the [SEP];
5. CodeBERT shards, written by the writer and by hand, into a row table;
6. RowBatches(max_tokens=) over rows of both kinds."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import code_collate_model as cm
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, EFORMAT, ECAPACITY, EINDEX = -1, -3, -6, -7
SENTINEL, GUARD = -7777, 64
P = ctypes.c_void_p
SEEDS, COUNTERS, PROBS = (11, (1 << 63) + 5), (0, 7), (0.0, 0.15, 1.0)


def label_key(mode):
  return 'special_tokens_mask' if mode == 0 else 'labels'


def ptr(t):
  return P(t.data_ptr() if t is not None else 0)


def stream():
  return P(torch.cuda.current_stream().cuda_stream)


def last_error():
  return _lib.lib().lddl_last_error().decode()


def dev_of(a, dt=None):
  """numpy -> cuda (uint16 as the int16 view the PackResult fields are)"""
  a = np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))
  return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to('cuda')


def draw_kw(col, seed, counter, p):
  return dict(seed=seed, counter=counter, p=p, mask_id=col.tok.mask_id, n_random=col.tok.vocab_size,
              ignore=col.ignore_index)


def assert_model(out, exp):
  assert set(out) == set(exp), (sorted(out), sorted(exp))
  for k, v in exp.items():
    if k == 'max_seqlen':
      assert out[k] == v and isinstance(out[k], int)
      continue
    got = out[k].cpu().numpy()
    assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, got.dtype, v.shape, v.dtype)
    assert np.array_equal(got, v), k


# ---- the hand-made table ---------------------------------------------------------
LENGTHS = [3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 130]


def hand_rows():
  """(a, b, s) of every row: each regime at each length it can have, then one
  row that no packer makes (s = 0 with a > 0), which only the error test picks"""
  out = []
  for n in LENGTHS:
    out.append((0, n - 2, 0))
    out.append((0, n - 3, 1))
    if n >= 4:
      a = max(1, (n - 3) // 2)
      out.append((a, n - 3 - a, 1))
  assert (0, 1, 0) in out and (0, 1, 1) in out  # b = 1
  return out + [(2, 3, 0)]


HAND = hand_rows()
BAD_ROW = len(HAND) - 1
GOOD = list(range(BAD_ROW))
HAND_LEN = [a + b + 2 + s for a, b, s in HAND]
REGIME = [(0 if s == 0 else 1 if a == 0 else 2) for a, b, s in HAND]


@functools.lru_cache(maxsize=None)
def hand_made():
  """(CodeCollate, table, rows()): spans at odd and even offsets with one id of
  gap between them, the last one ending at the last id"""
  from lddl_amd import pipeline
  from lddl_amd.loader import CodeCollate
  col = CodeCollate(sequence_length_alignment=8)
  src0, src1, cur = [], [], 0
  for a, b, s in HAND:
    src0.append(cur)
    cur += a + 1
    src1.append(cur)
    cur += b + 1
  n_ids = cur - 1
  assert src1[-1] + HAND[-1][1] == n_ids and any(x & 1 for x in src1) and any(not x & 1 for x in src1)
  ids = np.concatenate([1000 + np.arange(n_ids), np.zeros(16, np.int64)]).astype(np.uint16)
  n = len(HAND)
  sp = np.asarray(HAND, np.int64)
  lens = np.asarray(HAND_LEN, np.int64)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, dev_of(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      dev_of(sp[:, 0], np.uint16), dev_of(sp[:, 1], np.uint16), dev_of(sp[:, 2] << 1, np.uint8),
      dev_of(np.zeros(n, np.uint8)), dev_of(np.zeros(n, np.int64)), dev_of(np.asarray([[n]], np.int64)))
  res.ids, res.src0, res.src1 = dev_of(ids), dev_of(src0, np.int64), dev_of(src1, np.int64)
  res.cls_id, res.sep_id = col.tok.cls_id, col.tok.sep_id
  rows = res.rows()
  assert [len(r[5]) for r in rows] == HAND_LEN and sorted(set(HAND_LEN[:BAD_ROW])) == LENGTHS
  assert {(REGIME[g], HAND_LEN[g]) for g in GOOD} == {(k, n) for n in LENGTHS for k in (0, 1, 2) if (k, n) != (2, 3)}
  return col, res, rows


def selections():
  """name -> (collate_rows keywords, the same rows as a list)"""
  odd = [g for g in GOOD if HAND_LEN[g] != 130]  # the longest is 129: an odd seq_len at alignment 1
  rep = GOOD[::-1] + [GOOD[5], GOOD[5], GOOD[0]]  # reversed, with repeats
  return {'all': (dict(row0=0, n_rows=BAD_ROW), GOOD), 'list': (dict(rows=rep), rep), 'odd': (dict(rows=odd), odd),
          'range': (dict(row0=7, n_rows=12), list(range(7, 19)))}


def fresh(col, seed, counter, p, align=None):
  """a collate on the same ctx with its own seed, counter and probability"""
  from lddl_amd.loader import CodeCollate
  return_col = CodeCollate(tokenizer=col.tok, sequence_length_alignment=align or col.sequence_length_alignment,
                           mlm_probability=p, base_seed=seed, ignore_index=col.ignore_index)
  return_col.counter = counter
  return return_col


def padded_model(col, rows, idx, align, mode, seed=0, counter=0, p=0.15):
  return cm.padded(rows, idx, align, mode, col.tok.cls_id, col.tok.sep_id, **draw_kw(col, seed, counter, p))


def unpadded_model(col, rows, idx, mode, seed=0, counter=0, p=0.15):
  return cm.unpadded(rows, idx, mode, col.tok.cls_id, col.tok.sep_id, **draw_kw(col, seed, counter, p))


# ---- 1. padded -----------------------------------------------------------------------
@pytest.mark.parametrize('align', [8, 1])
@pytest.mark.parametrize('which', ['all', 'list', 'odd', 'range'])
def test_padded_equals_model(gpu, align, which):
  col, res, rows = hand_made()
  kw, idx = selections()[which]
  c = fresh(col, 1, 0, 0.15, align)
  out = c.collate_rows(res, mode=0, **kw)
  assert c.counter == 0
  S = out['input_ids'].shape[1]
  if align == 1:
    assert S == max(HAND_LEN[g] for g in idx) and (which != 'odd' or S == 129)
  assert_model(out, padded_model(col, rows, idx, align, 0))
  for seed in SEEDS:
    for counter in COUNTERS:
      for p in PROBS:
        c = fresh(col, seed, counter, p, align)
        out = c.collate_rows(res, **kw)  # dynamic by default
        assert c.counter == counter + 1
        assert_model(out, padded_model(col, rows, idx, align, 2, seed, counter, p))


def test_mode_2_is_mode_0_then_mask_tokens(gpu):
  col, res, rows = hand_made()
  for seed, counter, p in ((SEEDS[0], COUNTERS[1], 0.15), (SEEDS[1], COUNTERS[0], 1.0)):
    plain = fresh(col, seed, counter, p).collate_rows(res, GOOD, mode=0)
    both = fresh(col, seed, counter, p).collate_rows(res, GOOD, mode=2)
    ids, labels = fresh(col, seed, counter, p).mask_tokens(plain['input_ids'].clone(), plain['special_tokens_mask'],
                                                           counter=counter)
    assert torch.equal(ids, both['input_ids']) and torch.equal(labels, both['labels'])
    assert bool((labels != -1).any())
    for k in ('token_type_ids', 'attention_mask'):
      assert torch.equal(plain[k], both[k])


def test_probability_1_selects_every_token_and_no_special_column(gpu):
  col, res, rows = hand_made()
  plain = fresh(col, 3, 1, 1.0).collate_rows(res, GOOD, mode=0)
  out = fresh(col, 3, 1, 1.0).collate_rows(res, GOOD, mode=2)
  special = plain['special_tokens_mask'].cpu().numpy().astype(bool)
  labels = out['labels'].cpu().numpy()
  ids = plain['input_ids'].cpu().numpy()
  for k in (0, 1, 2):  # each regime: [CLS], every [SEP] and the padding keep ignore_index, every other column is drawn
    pick = [r for r, g in enumerate(GOOD) if REGIME[g] == k]
    assert pick
    for r in pick:
      a, b, s = HAND[GOOD[r]]
      n = a + b + 2 + s
      want = np.ones(special.shape[1], bool)
      want[1:n - 1] = False
      if s:
        want[a + 1] = True
      assert np.array_equal(special[r], want), (k, r)
      assert bool((labels[r][want] == -1).all()) and np.array_equal(labels[r][~want], ids[r][~want]), (k, r)


def guarded(shape, dtype, off):
  """(whole buffer, the tensor of `shape` inside it): GUARD sentinels in front
  and behind; off = 0: the tensor starts 16-B aligned, off = 1: one element further"""
  n = int(np.prod(shape))
  whole = torch.full((off + GUARD + n + GUARD + 1,), SENTINEL, dtype=dtype, device='cuda')
  assert whole.data_ptr() % 16 == 0
  return whole, whole[off + GUARD:off + GUARD + n].view(*shape)


def guards_intact(whole, inner, off):
  n = inner.numel()
  return bool((whole[:off + GUARD] == SENTINEL).all()) and bool((whole[off + GUARD + n:] == SENTINEL).all())


def raw_seq_len(col, res, rows_t, n=None, row0=0, align=1):
  n = rows_t.numel() if n is None else n
  seq = ctypes.c_int64(-5)
  rc = _lib.lib().lddl_collate_code_rows_seq_len(col.tok.handle, ptr(res.len0), ptr(res.len1), ptr(res.flags),
                                                 ptr(rows_t), row0, n, res.n_pairs, align, ctypes.byref(seq), stream())
  return rc, seq.value


def raw_padded(col, res, rows_t, S, mode, off=0, n=None, seed=31, counter=9, p=0.15):
  """lddl_collate_code_rows itself over guarded outputs -> rc, the four tensors, guards intact"""
  n_out = rows_t.numel() if n is None or n <= 0 else n
  bufs = [guarded((n_out, S), torch.int64, off) for _ in range(4)]
  n = rows_t.numel() if n is None else n
  rc = _lib.lib().lddl_collate_code_rows(
      col.tok.handle, ptr(res.ids), ptr(res.src0), ptr(res.src1), ptr(res.len0), ptr(res.len1), ptr(res.flags),
      ptr(rows_t), 0, n, res.n_pairs, S, mode, -1, p, seed, counter, *[ptr(b[1]) for b in bufs], stream())
  return rc, [b[1] for b in bufs], all(guards_intact(w, t, off) for w, t in bufs)


PADDED_KEYS = ('input_ids', 'token_type_ids', 'attention_mask')


@pytest.mark.parametrize('S', [130, 131])
def test_outputs_8_bytes_off_a_16_byte_boundary(gpu, S):
  """the lane = column path, taken for a misaligned base at an even and at an odd seq_len"""
  col, res, rows = hand_made()
  idx = GOOD[::-1]
  rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
  for mode in (0, 2):
    rc, outs, intact = raw_padded(col, res, rows_t, S, mode, off=1)
    assert rc == 0 and intact, last_error()
    assert outs[0].data_ptr() % 16 == 8
    exp = cm.padded(rows, idx, 1, mode, col.tok.cls_id, col.tok.sep_id, **draw_kw(col, 31, 9, 0.15))
    for k, o in zip(PADDED_KEYS + (label_key(mode),), outs):
      got = o.cpu().numpy()
      assert np.array_equal(got[:, :130], exp[k]), (mode, k)
      if S > 130:  # a pad column: id 0, type 0, attention 0, special (never drawn)
        assert bool((got[:, 130] == {'special_tokens_mask': 1, 'labels': -1}.get(k, 0)).all()), (mode, k)


# ---- 2. padding-free ---------------------------------------------------------------
def assert_padding_removed(pad, out, mode):
  m = pad['attention_mask'].bool()
  n, S = m.shape
  for k in ('input_ids', 'token_type_ids', label_key(mode)):
    assert out[k].dtype == torch.int64 and torch.equal(pad[k][m], out[k]), k
  col = torch.arange(S, device=m.device).expand(n, S)
  assert torch.equal(col[m], out['position_ids'])
  lens = m.sum(1)
  cu = torch.cat([torch.zeros(1, dtype=torch.int64, device=m.device), lens.cumsum(0)]).to(torch.int32)
  assert out['cu_seqlens'].dtype == torch.int32 and torch.equal(out['cu_seqlens'], cu)
  assert out['max_seqlen'] == int(lens.max()) == S
  assert set(out) == {'input_ids', 'token_type_ids', 'position_ids', label_key(mode), 'cu_seqlens', 'max_seqlen'}


@pytest.mark.parametrize('which', ['all', 'list', 'odd', 'range'])
@pytest.mark.parametrize('mode', [0, 2])
def test_unpadded_is_padded_without_padding(gpu, which, mode):
  col, res, rows = hand_made()
  kw, idx = selections()[which]
  for seed, counter in ((SEEDS[0], COUNTERS[0]), (SEEDS[1], COUNTERS[1])):
    a, b = fresh(col, seed, counter, 0.15, 1), fresh(col, seed, counter, 0.15, 64)
    pad = a.collate_rows(res, mode=mode, **kw)
    out = b.collate_rows_unpadded(res, mode=mode, **kw)
    assert a.counter == b.counter == counter + (mode == 2)
    assert_padding_removed(pad, out, mode)
    assert_model(out, unpadded_model(col, rows, idx, mode, seed, counter, 0.15))


def test_more_rows_than_one_chunk_of_the_scan(gpu):
  """2048 + 301 rows of 3 - 6 tokens: the offsets pass runs two chunks and the second scan level adds the first's sum"""
  col, res, rows = hand_made()
  short = [g for g in GOOD if HAND_LEN[g] <= 6]
  assert sorted({HAND_LEN[g] for g in short}) == [3, 4, 5, 6] and {REGIME[g] for g in short} == {0, 1, 2}
  idx = np.asarray(short)[np.random.default_rng(5).integers(0, len(short), 2048 + 301)].tolist()
  for mode in (0, 2):
    a, b = fresh(col, 9, 2, 0.15, 1), fresh(col, 9, 2, 0.15)
    out = b.collate_rows_unpadded(res, idx, mode=mode)
    assert_model(out, unpadded_model(col, rows, idx, mode, 9, 2, 0.15))
    assert_padding_removed(a.collate_rows(res, idx, mode=mode), out, mode)


def raw_cu(col, res, rows_t, cu, n=None):
  n = rows_t.numel() if n is None else n
  total, longest = ctypes.c_int64(-5), ctypes.c_int64(-5)
  rc = _lib.lib().lddl_collate_code_rows_cu_seqlens(col.tok.handle, ptr(res.len0), ptr(res.len1), ptr(res.flags),
                                                    ptr(rows_t), 0, n, res.n_pairs, ptr(cu), ctypes.byref(total),
                                                    ctypes.byref(longest), stream())
  return rc, total.value, longest.value


def raw_unpadded(col, res, rows_t, cu, total, mode, off=0, n=None, T=None, seed=31, counter=9, p=0.15):
  bufs = [guarded((total if T is None else T,), torch.int64, off) for _ in range(4)]
  n = rows_t.numel() if n is None else n
  rc = _lib.lib().lddl_collate_code_rows_unpadded(
      col.tok.handle, ptr(res.ids), ptr(res.src0), ptr(res.src1), ptr(res.len0), ptr(res.len1), ptr(res.flags),
      ptr(rows_t), 0, n, res.n_pairs, ptr(cu), total, mode, -1, p, seed, counter, *[ptr(b[1]) for b in bufs], stream())
  return rc, [b[1] for b in bufs], all(guards_intact(w, t, off) for w, t in bufs)


UNPADDED_KEYS = ('input_ids', 'token_type_ids', 'position_ids')


@pytest.mark.parametrize('off', [0, 1])
def test_unpadded_between_guards(gpu, off):
  """rows that start and end at both parities, at aligned outputs and at outputs 8 bytes off"""
  col, res, rows = hand_made()
  for idx in (GOOD, [GOOD[0]] + GOOD[::-1]):  # a 3-token row in front: every start changes parity
    rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
    cu_w, cu = guarded((len(idx) + 1,), torch.int32, off)
    rc, T, longest = raw_cu(col, res, rows_t, cu)
    assert rc == 0 and T == sum(HAND_LEN[g] for g in idx) and longest == 130 and guards_intact(cu_w, cu, off)
    for mode in (0, 2):
      rc, outs, intact = raw_unpadded(col, res, rows_t, cu, T, mode, off)
      assert rc == 0 and intact, last_error()
      exp = unpadded_model(col, rows, idx, mode, 31, 9, 0.15)
      assert np.array_equal(cu.cpu().numpy(), exp['cu_seqlens'])
      for k, o in zip(UNPADDED_KEYS + (label_key(mode),), outs):
        assert np.array_equal(o.cpu().numpy(), exp[k]), (mode, k)


# ---- 3. bad input, one call each ---------------------------------------------------
def still_good(col, res, rows):
  idx = [GOOD[-1], GOOD[0], GOOD[3]]
  assert_model(fresh(col, 1, 0, 0.15).collate_rows(res, idx, mode=0), padded_model(col, rows, idx, 8, 0))
  assert_model(fresh(col, 1, 0, 0.15).collate_rows_unpadded(res, idx, mode=0), unpadded_model(col, rows, idx, 0))


def written(outs, r):
  return [bool((o[r] != SENTINEL).any()) for o in outs]


@pytest.mark.parametrize('bad', [-1, len(HAND)])
def test_row_index_out_of_range(gpu, bad):
  col, res, rows = hand_made()
  idx = [1, bad, 2]
  rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
  assert raw_seq_len(col, res, rows_t)[0] == EINDEX
  rc, outs, intact = raw_padded(col, res, rows_t, 8, 0)
  assert rc == EINDEX and intact and written(outs, 1) == [False] * 4  # the bad row is left unwritten
  exp = padded_model(col, rows, [1, 2], 8, 0)
  for k, o in zip(PADDED_KEYS + ('special_tokens_mask',), outs):
    assert np.array_equal(o[[0, 2]].cpu().numpy(), exp[k]), k  # the rows around it are right
  cu = torch.full((4,), SENTINEL, dtype=torch.int32, device='cuda')
  assert raw_cu(col, res, rows_t, cu)[0] == EINDEX
  # the fill kernel's own check: offsets that give the bad row no tokens
  l1, l2 = HAND_LEN[1], HAND_LEN[2]
  cu = torch.tensor([0, l1, l1, l1 + l2], dtype=torch.int32, device='cuda')
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, l1 + l2, 0)
  assert rc == EINDEX and intact
  assert np.array_equal(outs[0].cpu().numpy(), unpadded_model(col, rows, [1, 2], 0)['input_ids'])
  with pytest.raises(IndexError):
    fresh(col, 1, 0, 0.15).collate_rows(res, idx, mode=0)
  still_good(col, res, rows)


@pytest.mark.parametrize('mode', [1, 3])
def test_modes_other_than_0_and_2(gpu, mode):
  col, res, rows = hand_made()
  rows_t = torch.tensor([1, 2], dtype=torch.int64, device='cuda')
  rc, outs, intact = raw_padded(col, res, rows_t, 8, mode)
  assert rc == EINVAL and intact and not any(written(outs, slice(None)))
  assert 'no static masks' in last_error()
  cu = torch.empty(3, dtype=torch.int32, device='cuda')
  rc, T, _ = raw_cu(col, res, rows_t, cu)
  assert rc == 0
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, T, mode)
  assert rc == EINVAL and intact and not any(written(outs, slice(None)))
  assert 'no static masks' in last_error()
  with pytest.raises(ValueError):
    fresh(col, 1, 0, 0.15).collate_rows(res, [1, 2], mode=mode)
  with pytest.raises(ValueError):
    fresh(col, 1, 0, 0.15).collate_rows_unpadded(res, [1, 2], mode=mode)
  still_good(col, res, rows)


def test_row_without_sep_that_has_doc_tokens(gpu):
  col, res, rows = hand_made()
  assert HAND[BAD_ROW] == (2, 3, 0) and HAND_LEN[BAD_ROW] == 7
  idx = [1, BAD_ROW, 2]
  rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
  rc, outs, intact = raw_padded(col, res, rows_t, 8, 0)
  assert rc == EINVAL and intact and written(outs, 1) == [False] * 4, last_error()
  assert 'batch row 1 ' in last_error()
  assert np.array_equal(outs[0][[0, 2]].cpu().numpy(), padded_model(col, rows, [1, 2], 8, 0)['input_ids'])
  cu = torch.empty(4, dtype=torch.int32, device='cuda')
  rc, T, _ = raw_cu(col, res, rows_t, cu)  # the offsets pass only adds lengths
  assert rc == 0 and T == HAND_LEN[1] + 7 + HAND_LEN[2]
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, T, 2)
  c = cu.cpu().numpy()
  assert rc == EINVAL and intact and not any(written(outs, slice(int(c[1]), int(c[2]))))
  assert all(written(outs, slice(0, int(c[1])))) and all(written(outs, slice(int(c[2]), T)))
  with pytest.raises(RuntimeError):
    fresh(col, 1, 0, 0.15).collate_rows(res, idx)
  still_good(col, res, rows)


def test_seq_len_one_short_of_the_longest_row(gpu):
  col, res, rows = hand_made()
  long = HAND_LEN.index(65)
  idx = [1, long, 2]
  rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
  assert raw_seq_len(col, res, rows_t) == (0, 65)
  rc, outs, intact = raw_padded(col, res, rows_t, 64, 0)
  assert rc == ECAPACITY and intact and written(outs, 1) == [False] * 4
  assert written(outs, 0) == written(outs, 2) == [True] * 4
  rc, outs, intact = raw_padded(col, res, rows_t, 65, 0)
  assert rc == 0 and intact
  assert np.array_equal(outs[0].cpu().numpy(), padded_model(col, rows, idx, 1, 0)['input_ids'])
  rc, outs, intact = raw_padded(col, res, rows_t, 2049, 0)
  assert rc == ECAPACITY and intact and not any(written(outs, slice(None)))
  still_good(col, res, rows)


def test_altered_cu_seqlens(gpu):
  col, res, rows = hand_made()
  idx = [3, 1, 5, 4, 2]
  rows_t = torch.tensor(idx, dtype=torch.int64, device='cuda')
  cu = torch.empty(len(idx) + 1, dtype=torch.int32, device='cuda')
  rc, T, _ = raw_cu(col, res, rows_t, cu)
  exp = unpadded_model(col, rows, idx, 0)
  h = exp['cu_seqlens']
  assert rc == 0 and np.array_equal(cu.cpu().numpy(), h)
  bad = h.copy()
  bad[2] += 1  # rows 1 and 2 no longer hold their tokens
  rc, outs, intact = raw_unpadded(col, res, rows_t, torch.from_numpy(bad).to('cuda'), T, 0)
  assert rc == EINVAL and intact and 'cu_seqlens' in last_error()
  for o, k in zip(outs, UNPADDED_KEYS + ('special_tokens_mask',)):
    o = o.cpu().numpy()
    assert bool((o[h[1]:h[3]] == SENTINEL).all()), k
    assert np.array_equal(o[:h[1]], exp[k][:h[1]]) and np.array_equal(o[h[3]:], exp[k][h[3]:]), k
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, T - 1, 0, T=T)  # the last row does not fit the total
  assert rc == EINVAL and intact and not any(written(outs, slice(int(h[-2]), T)))
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, 1 << 31, 0, T=T)
  assert rc == ECAPACITY and intact and not any(written(outs, slice(None)))
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, T, 0)
  assert rc == 0 and intact and np.array_equal(outs[0].cpu().numpy(), exp['input_ids'])
  still_good(col, res, rows)


def test_empty_batch(gpu):
  col, res, rows = hand_made()
  rows_t = torch.tensor([1, 2], dtype=torch.int64, device='cuda')
  assert raw_seq_len(col, res, rows_t, n=0)[0] == EINVAL
  rc, outs, intact = raw_padded(col, res, rows_t, 8, 0, n=0)
  assert rc == EINVAL and intact and not any(written(outs, slice(None)))
  cu = torch.full((3,), SENTINEL, dtype=torch.int32, device='cuda')
  assert raw_cu(col, res, rows_t, cu, n=0)[0] == EINVAL and bool((cu == SENTINEL).all())
  rc, outs, intact = raw_unpadded(col, res, rows_t, cu, 11, 0, n=0)
  assert rc == EINVAL and intact and not any(written(outs, slice(None)))
  for call in (col.collate_rows, col.collate_rows_unpadded):
    with pytest.raises(ValueError):
      call(res, [])
  still_good(col, res, rows)


# ---- 4. from the packer -------------------------------------------------------------
N_DOCS = 12
KEEP_ALIVE = []


@functools.lru_cache(maxsize=None)
def codebert_pack(bin_size):
  """(packer, result): a CodeBERT pack with spans of pre-tokenised documents,
  every other one without docstring, at target_seq_length 64"""
  from lddl_amd import pipeline
  docs = [[[5, 6, 7], [8, 9, 10, 11]], [[12] * 9, [13] * 5, [14] * 6]] * (N_DOCS // 2)
  sents = [s for d in docs for s in d]
  ntok = np.asarray([len(s) for s in sents], np.int32)
  off = np.concatenate([[0], np.cumsum(ntok)]).astype(np.int64)
  ids = np.asarray([t for s in sents for t in s] + [0] * 16, np.uint16)
  dso = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
  dev = 'cuda'
  sh = pipeline.ShardSet(torch.zeros(int(off[-1]) + 16, dtype=torch.uint8, device=dev), torch.from_numpy(off).to(dev),
                         torch.from_numpy(dso).to(dev), torch.tensor([0, len(docs)], dtype=torch.int64, device=dev),
                         torch.tensor([0, 1] * (N_DOCS // 2), dtype=torch.int32, device=dev), int(off[-1]))
  cpk = pipeline.Packer(_lib.VOCAB_CODEBERT, 0)
  inputs = (sh, torch.from_numpy(ids.view(np.int16)).to(dev), torch.from_numpy(ntok).to(dev))
  res = cpk.pack(*inputs, target_seq_length=64, duplicate_factor=2, seed=3, codebert=True, spans=True,
                 bin_size=bin_size)
  torch.cuda.synchronize()
  flags = res.flags[:res.n_pairs].cpu().numpy()
  assert res.n_pairs > 0 and bool(((flags & 2) == 0).any()) and bool((flags & 2).any())
  # the pack keeps the addresses of its inputs and lddl_row_docs (the writer's id column) reads the shard set's
  # offsets through them: the inputs live as long as the cached result does
  KEEP_ALIVE.append(inputs)
  return cpk, res


def code_collate(pk, **kw):
  from lddl_amd.loader import CodeCollate
  return CodeCollate(tokenizer=pk.tok, **kw)


@pytest.mark.parametrize('mode', [0, 2])
def test_pack_result_equals_model(gpu, mode):
  pk, res = codebert_pack(None)
  rows, idx = res.rows(), list(range(res.n_pairs))
  col = code_collate(pk, base_seed=21, mlm_probability=0.3)
  col.counter = 4
  assert_model(col.collate_rows(res, mode=mode), padded_model(col, rows, idx, 8, mode, 21, 4, 0.3))
  col.counter = 4
  assert_model(col.collate_rows_unpadded(res, mode=mode), unpadded_model(col, rows, idx, mode, 21, 4, 0.3))


def test_bert_collate_agrees_on_rows_with_sep(gpu):
  from lddl_amd.loader import BertCollate
  pk, res = codebert_pack(None)
  with_sep = np.flatnonzero(res.flags[:res.n_pairs].cpu().numpy() & 2).tolist()
  assert 0 < len(with_sep) < res.n_pairs
  code = code_collate(pk).collate_rows(res, with_sep, mode=0)
  bert = BertCollate(tokenizer=pk.tok).collate_rows(res, with_sep, mode=0)
  for k in ('input_ids', 'token_type_ids', 'attention_mask', 'special_tokens_mask'):
    assert torch.equal(code[k], bert[k]), k
  assert 'next_sentence_labels' not in code


# ---- 5. shards ----------------------------------------------------------------------
@pytest.mark.parametrize('bin_size', [None, 16])
def test_written_shards_load_into_the_pack_results_rows(gpu, tmp_path, bin_size):
  from lddl_amd import writer
  from lddl_amd.loader import load_shards
  pk, res = codebert_pack(bin_size)
  out = str(tmp_path / 'shards')
  writer.write_shards(pk, res, out, bin_size=bin_size, codebert=True, doc_ids=['py_%d' % d for d in range(N_DOCS)])
  col = code_collate(pk, base_seed=5)
  table = load_shards(col, out)
  assert table.spans and table.n_pairs == res.n_pairs and table.n_tokens == res.n_tokens
  assert table.nbins == (res.nbins if bin_size else 1)
  assert len({r[4] for r in res.rows()}) > 1 or not bin_size
  for g, (got, want) in enumerate(zip(table.rows(), res.rows())):
    p, a, b, fl, bn, tok = want
    assert got == (p, a, b, fl, bn if bin_size else 0, tok), g
  for mode in (0, 2):
    col.counter = 6
    want = col.collate_rows(res, mode=mode)
    col.counter = 6
    got = col.collate_rows(table, mode=mode)
    for k in want:
      assert torch.equal(got[k], want[k]), (mode, k)


def vocab_tokens(path):
  with open(path, 'rb') as f:
    lines = f.read().decode('utf-8').split('\n')
  toks = [l.rstrip() for l in lines]
  return toks, {t: i for i, t in enumerate(toks) if t}


def hand_table(large):
  """a CodeBERT shard by hand -> (pyarrow table, expected (doc ids, code ids, flags) per row)"""
  import pyarrow as pa
  toks, ids = vocab_tokens(_lib.VOCAB_CODEBERT)
  pick = [t for t in toks[2000:2400] if t and not t.isspace() and len(t.split()) == 1 and ids[t] >= 2000][:40]
  assert len(pick) == 40 and 'zz_not_a_token_zz' not in ids
  w = lambda k: pick[k % 40]  # noqa: E731
  doc = [' '.join(w(k) for k in range(3)), '', '', ' '.join([w(5), 'zz_not_a_token_zz', w(6)]), '  ']
  code = [' '.join(w(k) for k in range(10, 17)), ' '.join(w(k) for k in range(20, 24)), w(30) + '  ' + w(31),
          'zz_not_a_token_zz', '\t' + w(33) + ' \n']
  # an empty doc with the [SEP] (b + 3) and without it (b + 2); whitespace alone is an empty doc too
  num_tokens = [3 + 7 + 3, 4 + 3, 2 + 2, 3 + 1 + 3, 1 + 3]
  st = pa.large_string() if large else pa.string()
  t = pa.table({'id': pa.array(['x%d' % k for k in range(5)]), 'doc': pa.array(doc, st), 'code': pa.array(code, st),
                'num_tokens': pa.array(num_tokens, pa.uint16())})
  return t, doc, code, num_tokens, ids


@pytest.mark.parametrize('large', [False, True])
def test_hand_made_shard(gpu, large):
  col, _, _ = hand_made()
  t, doc, code, num_tokens, ids = hand_table(large)
  unk = col.tok.unk_id
  table = col.load_rows(t)
  rows = table.rows()
  assert table.n_pairs == 5 and table.n_tokens == sum(num_tokens)
  for g, row in enumerate(rows):
    a = [ids.get(x, unk) for x in doc[g].split()]
    b = [ids.get(x, unk) for x in code[g].split()]
    s = num_tokens[g] - len(a) - len(b) - 2
    assert row[1:4] == (a, b, s << 1), g
    assert len(row[5]) == num_tokens[g]
  assert unk in rows[3][1] and rows[3][2] == [unk]
  assert [r[3] for r in rows] == [2, 2, 0, 2, 2]
  idx = list(range(5))
  assert_model(fresh(col, 1, 0, 0.15).collate_rows(table, mode=0), padded_model(col, rows, idx, 8, 0))
  assert_model(fresh(col, 8, 2, 0.5).collate_rows_unpadded(table), unpadded_model(col, rows, idx, 2, 8, 2, 0.5))


def staged(doc, code, num_tokens):
  from lddl_amd.loader import _column
  out = []
  for col in (doc, code):
    data, off = _column(col, True)
    out += [torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to('cuda'), torch.from_numpy(off).to('cuda')]
  return out + [dev_of(np.asarray(num_tokens, np.uint16))]


def raw_len(col, cols, n):
  L = _lib.lib()
  len0, len1 = (torch.full((n,), 77, dtype=torch.int16, device='cuda') for _ in range(2))
  src0, src1 = (torch.full((n,), SENTINEL, dtype=torch.int64, device='cuda') for _ in range(2))
  tok_off = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device='cuda')
  tot = (ctypes.c_int64 * 2)(-5, -5)
  rc = L.lddl_code_rows_from_strings_len(col.tok.handle, *[ptr(c) for c in cols], n, ptr(len0), ptr(len1), ptr(src0),
                                         ptr(src1), ptr(tok_off), tot, stream())
  return rc, (len0, len1, src0, src1), tok_off, list(tot)


def raw_fill(col, cols, n, spans, n_ids, cap):
  ids_w, ids = guarded((n_ids,), torch.int16, 0)
  flags = torch.full((n,), 99, dtype=torch.uint8, device='cuda')
  rc = _lib.lib().lddl_code_rows_from_strings(col.tok.handle, *[ptr(c) for c in cols], n, *[ptr(s) for s in spans],
                                              ptr(ids), cap, ptr(flags), stream())
  return rc, ids, flags, guards_intact(ids_w, ids, 0)


@pytest.mark.parametrize('wrong', ['a+b+1', 'a+b+4', 'a+b+2 with a > 0'])
def test_num_tokens_that_fits_no_row(gpu, wrong):
  col, _, _ = hand_made()
  _, doc, code, num_tokens, _ = hand_table(False)
  good = staged(doc, code, num_tokens)
  rc, spans, tok_off, tot = raw_len(col, good, 5)
  assert rc == 0 and tot == [sum(num_tokens) - 2 * 5 - 4, sum(num_tokens)], last_error()
  assert tok_off.cpu().tolist() == np.concatenate([[0], np.cumsum(num_tokens)]).tolist()
  row, nt = {'a+b+1': (1, 4 + 1), 'a+b+4': (2, 2 + 4), 'a+b+2 with a > 0': (3, 3 + 1 + 2)}[wrong]
  bad_nt = list(num_tokens)
  bad_nt[row] = nt
  bad = staged(doc, code, bad_nt)
  rc = raw_len(col, bad, 5)[0]
  assert rc == EFORMAT and ('row %d:' % row) in last_error(), (rc, last_error())
  # the fill pass checks again: the lengths of the good columns, the altered num_tokens
  rc, ids, flags, intact = raw_fill(col, bad, 5, spans, tot[0], tot[0])
  assert rc == EFORMAT and intact and ('row %d:' % row) in last_error()
  s0 = spans[2].cpu().numpy()
  l0, l1 = spans[0].cpu().numpy(), spans[1].cpu().numpy()
  ids_h, flags_h = ids.cpu().numpy(), flags.cpu().numpy()
  for g in range(5):
    span = ids_h[s0[g]:s0[g] + l0[g] + l1[g]]
    if g == row:
      assert bool((span == SENTINEL).all()) and flags_h[g] == 99  # nothing written for it
    else:
      assert not bool((span == SENTINEL).any()) and flags_h[g] != 99, g
  with pytest.raises(RuntimeError):
    import pyarrow as pa
    col.load_rows(pa.table({'doc': pa.array(doc), 'code': pa.array(code), 'num_tokens': pa.array(bad_nt, pa.uint16())}))
  assert col.load_rows(hand_table(False)[0]).n_pairs == 5  # and right again on the same ctx


def test_capacity_one_short(gpu):
  col, _, _ = hand_made()
  _, doc, code, num_tokens, _ = hand_table(False)
  cols = staged(doc, code, num_tokens)
  rc, spans, _, tot = raw_len(col, cols, 5)
  assert rc == 0
  rc, ids, flags, intact = raw_fill(col, cols, 5, spans, tot[0], tot[0] - 1)
  assert rc == ECAPACITY and intact, last_error()
  assert bool((ids == SENTINEL).all()) and bool((flags == 99).all())  # nothing written
  rc, ids, flags, intact = raw_fill(col, cols, 5, spans, tot[0], tot[0])
  assert rc == 0 and intact and not bool((ids == SENTINEL).any()) and flags.cpu().tolist() == [2, 2, 0, 2, 2]


def test_shards_of_the_other_kind(gpu, tmp_path):
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd.loader import BertCollate, load_shards
  col, _, _ = hand_made()
  bert_dir, code_dir = str(tmp_path / 'bert'), str(tmp_path / 'code')
  os.makedirs(bert_dir)
  os.makedirs(code_dir)
  bert = pa.table({'A': pa.array(['a b']), 'B': pa.array(['c']), 'is_random_next': pa.array([False]),
                   'num_tokens': pa.array([6], pa.uint16())})
  pq.write_table(bert, os.path.join(bert_dir, 'part.0.parquet'))
  pq.write_table(hand_table(False)[0], os.path.join(code_dir, 'part.0.parquet'))
  with pytest.raises(ValueError, match='BertCollate'):
    load_shards(col, bert_dir)
  with pytest.raises(ValueError):
    col.load_rows(bert)
  with pytest.raises(ValueError, match='CodeBERT'):
    load_shards(BertCollate(tokenizer=col.tok), code_dir)
  assert load_shards(col, code_dir).n_pairs == 5


# ---- 6. token-budget batches --------------------------------------------------------
def test_row_batches_count_a_row_by_its_flags(gpu):
  from lddl_amd.loader import RowBatches, plan_token_batches
  col, res, rows = hand_made()
  import dataclasses
  short = [g for g in GOOD if HAND_LEN[g] <= 6]
  pick = torch.tensor(short, dtype=torch.int64, device='cuda')
  sub = dataclasses.replace(res, n_pairs=len(short), len0=res.len0[pick], len1=res.len1[pick], flags=res.flags[pick],
                            src0=res.src0[pick], src1=res.src1[pick])
  lens = np.asarray([HAND_LEN[g] for g in short])
  old = lens + np.asarray([1 - HAND[g][2] for g in short])  # what len0 + len1 + 3 counted
  M = 24
  batches = RowBatches(sub, max_tokens=M, seed=2)
  plan = batches.plan()
  # on the host first: rows of both kinds, and a batch that the old count would have had to cut
  assert {HAND[g][2] for g in short} == {0, 1} and batches.lengths.tolist() == lens.tolist()
  assert all(lens[b].sum() <= M for b in plan) and any(old[b].sum() > M for b in plan)
  assert [b.tolist() for b in plan] == [b.tolist() for b in plan_token_batches(lens, M, seed=2)]
  sub_rows = [rows[g] for g in short]
  seen = []
  for idx in batches:
    out = col.collate_rows_unpadded(sub, idx, mode=0)
    cu = out['cu_seqlens'].cpu().numpy()
    assert 0 < cu[-1] <= M
    assert_model(out, unpadded_model(col, sub_rows, idx.cpu().tolist(), 0))
    seen += idx.cpu().tolist()
  assert sorted(seen) == list(range(len(short)))
