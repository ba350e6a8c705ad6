"""lddl_collate_rows_fixed / lddl_collate_code_rows_fixed
(collate_rows_fixed): the padding-free batch at fixed shapes, held to

* collate_rows_unpadded on the same rows, seed and counter for [0, total),
  cu_seqlens[0 .. n] and next_sentence_labels[0 .. n), bit for bit, and to the
  numpy model of tests/collate_fixed_model.py for the slack, the cu_seqlens
  tail, the label tail and the counts;
* hand-made row tables at the shapes where the kernel changes path: rows that
  start and end at both parities, every slack regime at a small max_seqlen,
  outputs at 16-B aligned bases and one element off, 1 row, 257 rows, more rows
  than one pass of the grid, a run of rows longer than one scan step, sentinels
  around every output;
* refusals, which set an error and never fault or write out of place;
* compact_mlm and the shapes over an epoch of RowBatches."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import collate_fixed_model as fm
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEED, COUNTER = 31, 9
EINVAL, ECAPACITY, EINDEX = -1, -6, -7
SENTINEL = -7777
GUARD = 64
P = ctypes.c_void_p


def ptr(t):
  return P(t.data_ptr() if t is not None else 0)


def stream():
  return P(torch.cuda.current_stream().cuda_stream)


def last_error():
  return _lib.lib().lddl_last_error().decode()


def to_np(batch):
  return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in batch.items()}


def reference(col, res, mode, T, N, S, **sel):
  """collate_rows_unpadded at (SEED, COUNTER) on the same rows, extended by the numpy model"""
  col.counter = COUNTER
  unp = to_np(col.collate_rows_unpadded(res, mode=mode, **sel))
  del unp['max_seqlen']
  return fm.fixed_batch(unp, T, N, S, col.ignore_index, mode)


def assert_fixed(out, exp):
  assert set(out) == set(exp), (sorted(out), sorted(exp))
  for k, v in exp.items():
    if not isinstance(v, np.ndarray):
      assert isinstance(out[k], int) and out[k] == v, (k, out[k], v)
      continue
    got = out[k].cpu().numpy()
    assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, got.dtype, v.shape, v.dtype)
    assert np.array_equal(got, v), (k, np.flatnonzero(got != v)[:8])


# ---- 1. equality with the unpadded route, on packed text --------------------------
@functools.lru_cache(maxsize=None)
def packed(masking):
  """(packer, result) of a few hundred sentences: 3 partitions, seq 128, bin 32, dup 2"""
  from lddl_amd import pipeline, synth
  c = synth.make_wiki(40_000, seed=4242)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0, masking=masking)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 3), torch.device('cuda', 0))
  res = pk.run(sh, target_seq_length=128, bin_size=32, duplicate_factor=2, seed=4242, masking=masking, spans=True)
  torch.cuda.synchronize()
  assert res.spans and 100 < res.n_pairs < 5000
  return pk, res


def bert_collate(pk, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=pk.tok, sequence_length_alignment=1, base_seed=SEED, **kw)


def selections(n):
  rng = np.random.default_rng(3)
  idx = rng.permutation(n)[:41].tolist() + [0, n - 1]
  idx.append(idx[5])  # one repeated row
  return {'all': {}, 'list': {'rows': idx}, 'row0': {'row0': 5, 'n_rows': 37}}


@pytest.mark.parametrize('masking,mode,wwm', [(False, 0, False), (True, 1, False), (False, 2, False), (False, 2, True)])
@pytest.mark.parametrize('which', ['all', 'list', 'row0'])
def test_equals_unpadded_route(gpu, masking, mode, wwm, which):
  pk, res = packed(masking)
  sel = selections(res.n_pairs)[which]
  try:
    col = bert_collate(pk, whole_word_mask=wwm)
    col.counter = COUNTER
    total = int(col.collate_rows_unpadded(res, mode=mode, **sel)['cu_seqlens'][-1])
    n = {'all': res.n_pairs, 'list': 44, 'row0': 37}[which]
    S = 131
    T = (total + 2 * S + 38) | 1  # odd: the rows of the output tensor alternate between the two store paths
    N = n + 3 + 7
    exp = reference(col, res, mode, T, N, S, **sel)
    col.counter = COUNTER
    out = col.collate_rows_fixed(res, mode=mode, max_tokens=T, max_seqs=N, max_seqlen=S, **sel)
    assert col.counter == (COUNTER if mode == 0 else COUNTER + 1)  # as the unpadded route
    assert_fixed(out, exp)
    assert out['num_rows'] == n and out['num_seqs'] == n + 3 and out['max_seqlen'] == S
    if mode == 2:
      assert bool((out['labels'][:total] != -1).any())  # the comparison is not vacuous
      if wwm:  # and whole-word selection differs from token selection at the same draw
        plain = bert_collate(pk)
        plain.counter = COUNTER
        other = plain.collate_rows_fixed(res, mode=2, max_tokens=T, max_seqs=N, max_seqlen=S, **sel)
        assert not torch.equal(other['labels'], out['labels'])
  finally:
    bert_collate(pk)  # the ctx's switch off again


# ---- 2. hand-made BERT rows and the raw C call -----------------------------------
LENS = [3, 4, 5, 6, 7, 8, 16, 63, 64, 65, 127, 128, 129, 130, 515]


def row_of(m):
  return LENS.index(m)


def dev_of(a, dt=None):
  a = np.ascontiguousarray(np.asarray(a).astype(dt) if dt is not None else np.asarray(a))
  return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to('cuda')


def table(spec, kind):
  """a PackResult over (a, b, flags) rows: spans one after the other with one id of gap, at odd and even offsets"""
  from lddl_amd import pipeline
  src0, src1, cur = [], [], 0
  for a, b, _ in spec:
    src0.append(cur)
    cur += a + 1
    src1.append(cur)
    cur += b + 1
  ids = np.concatenate([1000 + np.arange(cur), np.zeros(16, np.int64)]).astype(np.uint16)
  sp = np.asarray(spec, np.int64)
  n = len(spec)
  lens = sp[:, 0] + sp[:, 1] + 2 + ((sp[:, 2] >> 1) & 1)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, dev_of(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      dev_of(sp[:, 0], np.uint16), dev_of(sp[:, 1], np.uint16), dev_of(sp[:, 2], np.uint8),
      dev_of(np.zeros(n, np.uint8)), dev_of(np.zeros(n, np.int64)), dev_of(np.asarray([[n]], np.int64)))
  res.ids, res.src0, res.src1 = dev_of(ids), dev_of(src0, np.int64), dev_of(src1, np.int64)
  res.kind = kind
  return res, lens.tolist()


@functools.lru_cache(maxsize=None)
def hand_made():
  """(packer, BERT table) with static masks at positions 1 and n - 2 of every row"""
  from lddl_amd import pipeline
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  res, lens = table([((m - 3) // 2, m - 3 - (m - 3) // 2, 2 | (g & 1)) for g, m in enumerate(LENS)], 'bert')
  assert lens == LENS
  res.cls_id, res.sep_id = pk.tok.cls_id, pk.tok.sep_id
  pos, off = [], [0]
  for m in LENS:
    pos.extend(sorted({1, m - 2}))
    off.append(len(pos))
  k = np.arange(len(pos))
  res.n_masked, res.mlm_off = len(pos), dev_of(off, np.int64)
  res.mlm_pos, res.mlm_label = dev_of(pos, np.uint16), dev_of(2000 + k, np.uint16)
  res.mlm_token = dev_of(np.where(k % 3 == 0, 3000 + k, pk.tok.mask_id), np.uint16)
  return pk, res


def guarded(n, dtype, off):
  """(whole buffer, its n elements): GUARD sentinels in front and behind;
  off = 0: the n elements start 16-B aligned, off = 1: one element further"""
  whole = torch.full((off + GUARD + n + GUARD + 1,), SENTINEL, dtype=dtype, device='cuda')
  assert whole.data_ptr() % 16 == 0
  return whole, whole[off + GUARD:off + GUARD + n]


def guards_intact(whole, n, off):
  return bool((whole[:off + GUARD] == SENTINEL).all()) and bool((whole[off + GUARD + n:] == SENTINEL).all())


class Raw:
  """one lddl_collate_rows_fixed call over sentinel-guarded outputs at base offset off"""

  def __init__(self, pk, res, idx, mode, T, N, S, off=0, override=()):
    override = dict(override)
    rows = torch.as_tensor(np.asarray(idx, np.int64)).to('cuda')
    self.T, self.N, self.off, self.mode = T, N, off, mode
    self.tok = [guarded(max(T, 0), torch.int64, off) for _ in range(4)]
    self.cu, self.nsl = guarded(N + 1, torch.int32, off), guarded(N, torch.int64, off)
    self.status = guarded(4, torch.int32, 0)
    self.counts = [ctypes.c_int64(-5) for _ in range(3)]
    mlm = (res.mlm_off, res.mlm_pos, res.mlm_label, res.mlm_token) if mode == 1 else (None,) * 4
    a = dict(ids=ptr(res.ids), src0=ptr(res.src0), src1=ptr(res.src1), len0=ptr(res.len0), len1=ptr(res.len1),
             flags=ptr(res.flags), rows=ptr(rows), row0=0, n=rows.numel(), n_total=res.n_pairs, mlm_off=ptr(mlm[0]),
             mlm_pos=ptr(mlm[1]), mlm_label=ptr(mlm[2]), mlm_token=ptr(mlm[3]), cu=ptr(self.cu[1]), T=T, N=N, S=S,
             mode=mode, ignore=-1, p=0.15, seed=SEED, counter=COUNTER, input_ids=ptr(self.tok[0][1]),
             token_type_ids=ptr(self.tok[1][1]), position_ids=ptr(self.tok[2][1]), labels=ptr(self.tok[3][1]),
             nsl=ptr(self.nsl[1]), status=ptr(self.status[1]), out_total=ctypes.byref(self.counts[0]),
             out_n_rows=ctypes.byref(self.counts[1]), out_n_seqs=ctypes.byref(self.counts[2]))
    assert set(override) <= set(a), set(override) - set(a)
    a.update(override)
    self.rc = _lib.lib().lddl_collate_rows_fixed(pk.tok.handle, *a.values(), stream())
    self.message = last_error() if self.rc else ''

  def intact(self):
    return (all(guards_intact(w, max(self.T, 0), self.off) for w, _ in self.tok) and
            guards_intact(self.cu[0], self.N + 1, self.off) and guards_intact(self.nsl[0], self.N, self.off) and
            guards_intact(self.status[0], 4, 0))

  def untouched(self):
    """nothing at all was written"""
    return self.intact() and all(bool((v == SENTINEL).all()) for _, v in self.tok + [self.cu, self.nsl, self.status])

  def batch(self):
    total, n, seqs = (int(c.value) for c in self.counts)
    return {'input_ids': self.tok[0][1], 'token_type_ids': self.tok[1][1], 'position_ids': self.tok[2][1],
            fm.label_key(self.mode): self.tok[3][1], 'next_sentence_labels': self.nsl[1], 'cu_seqlens': self.cu[1],
            'status': self.status[1], 'max_seqlen': int(self.status[1][3]), 'num_tokens': total, 'num_rows': n,
            'num_seqs': seqs}


def check_raw(idx, T, N, S, off, modes=(0, 1, 2)):
  pk, res = hand_made()
  col = bert_collate(pk)
  for mode in modes:
    exp = reference(col, res, mode, T, N, S, rows=torch.as_tensor(np.asarray(idx, np.int64)))
    call = Raw(pk, res, idx, mode, T, N, S, off)
    assert call.rc == 0, call.message
    assert call.intact()
    assert_fixed(call.batch(), exp)


# rows of 3 .. 8 tokens at max_seqlen 8: (the rows' lengths, slack, slots beyond n + p)
SLACK = {
    'none_even_total': ([3, 4, 7, 8, 5, 5], 0, 0),
    'none_odd_total': ([3, 4, 8], 0, 2),
    'one_after_odd_total': ([3, 4, 8], 1, 1),
    'one_after_even_total': ([3, 5, 6, 8], 1, 1),
    'max_seqlen': ([4, 7, 3], 8, 2),
    'max_seqlen_and_one': ([4, 7, 3], 9, 2),
    'max_seqlen_and_one_odd_total': ([4, 7, 3, 5], 9, 2),
    'several': ([6, 3, 8, 8, 7], 8 * 5 + 3, 1),
    'slots_exactly': ([6, 3, 8, 8], 8 * 3 + 2, 0),
    'long_empty_tail': ([5, 3, 4, 8], 11, 1500),
}


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('regime', sorted(SLACK))
def test_slack_regimes(gpu, regime, off):
  lens, slack, spare = SLACK[regime]
  total = sum(lens)
  assert ('odd' in regime) == bool(total & 1) or 'total' not in regime
  check_raw([row_of(m) for m in lens], total + slack, len(lens) + fm.pad_seqs(total, total + slack, 8) + spare, 8, off)


@pytest.mark.parametrize('off', [0, 1])
def test_rows_start_and_end_at_both_parities(gpu, off):
  """every length, in runs of odd rows (3 5 7 63 65 127 129 515) that alternate the parity of the next start, and the
  same behind one 3-token row; pad sequences of an odd and an even max_seqlen"""
  order = [3, 4, 5, 7, 64, 63, 65, 8, 16, 127, 129, 128, 515, 130, 6, 129, 3, 65, 64, 515, 5, 128, 127, 130, 4, 63, 7]
  seen = {}
  for lens in (order, [3] + order):
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for s, m in zip(starts, lens):
      seen.setdefault(m, set()).add(int(s) & 1)
  assert seen == {m: {0, 1} for m in LENS}
  for lens, S in ((order, 515), ([3] + order, 516)):
    total = sum(lens)
    check_raw([row_of(m) for m in lens], total + 2 * S + 1, len(lens) + 3 + 2, S, off)


@pytest.mark.parametrize('off', [0, 1])
def test_one_row_batches(gpu, off):
  for m in LENS:
    check_raw([row_of(m)], m + 5, 3, max(m, 3), off)
  check_raw([row_of(8)], 8, 1, 8, off)  # exactly full: one slot, no slack


@pytest.mark.parametrize('off', [0, 1])
def test_257_rows(gpu, off):
  short = [row_of(m) for m in LENS if m <= 65]
  idx = [short[i % len(short)] for i in range(253)] + [row_of(m) for m in (128, 129, 515, 130)]
  assert len(idx) == 257
  total = sum(LENS[g] for g in idx)
  check_raw(idx, total + 515 + 4, 257 + 2 + 1, 515, off)


@pytest.mark.parametrize('off', [0, 1])
def test_more_rows_than_one_pass_of_the_grid(gpu, off):
  """the grid is capped at 8 blocks of 4 rows per CU: beyond that a block's run is several steps of four rows, and
  the blocks at the end of the batch sum a prefix of thousands of rows"""
  short = np.asarray([row_of(m) for m in LENS if m <= 65])
  n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 5
  idx = short[np.random.default_rng(1).integers(0, len(short), n)].tolist()
  total = sum(LENS[g] for g in idx)
  check_raw(idx, total + 65 * 3 + 2, n + 4 + 3, 65, off, modes=(0, 1))


def test_run_longer_than_one_scan_step(gpu):
  """more than 256 rows per block: the scan of a run takes several steps, with the carry between them"""
  n = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 5
  idx = np.asarray([row_of(3), row_of(4), row_of(5)])[np.random.default_rng(2).integers(0, 3, n)].tolist()
  total = sum(LENS[g] for g in idx)
  check_raw(idx, total + 8 * 4 + 3, n + 5 + 1, 8, 0, modes=(0, 2))


# ---- 3. other row kinds ------------------------------------------------------------
# (a, b, flags): CodeBERT rows with the [SEP] after doc (flags 2), and without docstring (flags 0, a = 0)
CODE_ROWS = [(0, 1, 0), (0, 1, 2), (0, 5, 0), (2, 3, 2), (0, 62, 0), (30, 31, 2), (0, 63, 2), (60, 66, 2), (0, 127, 0),
             (0, 2, 0), (1, 1, 2)]


@pytest.mark.parametrize('mode', [0, 2])
@pytest.mark.parametrize('kind', ['codebert', 'mlm'])
def test_code_and_mlm_rows(gpu, kind, mode):
  from lddl_amd.loader import CodeCollate, MlmCollate
  if kind == 'codebert':
    col = CodeCollate(sequence_length_alignment=1, base_seed=SEED)
    res, lens = table(CODE_ROWS, kind)
    assert lens == [3, 4, 7, 8, 64, 64, 66, 129, 129, 4, 5] and any(f == 0 for _, _, f in CODE_ROWS)
  else:
    col = MlmCollate(tokenizer=hand_made()[0].tok, sequence_length_alignment=1, base_seed=SEED)
    res, lens = table([(0, m - 2, 0) for m in LENS[:-2]], kind)
    assert lens == LENS[:-2] and max(lens) == 129
  res.cls_id, res.sep_id = col.tok.cls_id, col.tok.sep_id
  n = len(lens)
  for sel, k in (({}, n), ({'rows': [1, 0, 3, 3, 2, n - 1]}, 6), ({'row0': 2, 'n_rows': 5}, 5)):
    for S, extra in ((130, 130 + 9), (129, 2 * 129)):
      col.counter = COUNTER
      total = int(col.collate_rows_unpadded(res, mode=mode, **sel)['cu_seqlens'][-1])
      T, N = total + extra, k + 2 + 3
      exp = reference(col, res, mode, T, N, S, **sel)
      col.counter = COUNTER
      out = col.collate_rows_fixed(res, mode=mode, max_tokens=T, max_seqs=N, max_seqlen=S, **sel)
      assert col.counter == (COUNTER if mode == 0 else COUNTER + 1)
      assert 'next_sentence_labels' not in out and out['num_seqs'] == k + 2
      assert_fixed(out, exp)
  with pytest.raises(RuntimeError, match='max_seqlen'):  # a CodeBERT row has two tokens at least
    col.collate_rows_fixed(res, [0], mode=mode, max_tokens=8, max_seqs=8, max_seqlen=1)
  with pytest.raises(ValueError):
    col.collate_rows_fixed(res, [0], mode=1, max_tokens=8, max_seqs=8, max_seqlen=8)  # no static masks


# ---- 4. refusals -------------------------------------------------------------------
def still_good(off=0):
  check_raw([row_of(4), row_of(7), row_of(3)], 14 + 9, 3 + 2, 8, off, modes=(0,))


def test_capacity_refusals(gpu):
  pk, res = hand_made()
  idx = [row_of(m) for m in (4, 7, 3, 8)]  # 22 tokens
  for off in (0, 1):
    for mode in (0, 1, 2):
      call = Raw(pk, res, idx, mode, 21, 9, 8, off)  # total == T + 1
      assert call.rc == ECAPACITY and 'tok_cap' in call.message and call.intact()
      assert call.counts[0].value == 22 and call.counts[1].value == 4
      for k in range(4):  # the rows that fit are stored, the one that would pass T is not
        assert bool((call.tok[k][1][14:] == SENTINEL).all())
      call = Raw(pk, res, idx, mode, 22 + 9, 5, 8, off)  # two pad sequences: n + p == N + 1
      assert call.rc == ECAPACITY and 'seq_cap' in call.message and call.intact()
      assert [c.value for c in call.counts] == [22, 4, 6]
      call = Raw(pk, res, idx, mode, 22 + 9, 6, 8, off)
      assert call.rc == 0 and call.intact()
      call = Raw(pk, res, idx, mode, 64, 16, 7, off)  # a row of S + 1 tokens
      assert call.rc == ECAPACITY and 'batch row 3 longer than 7' in call.message and call.intact()
      call = Raw(pk, res, idx, mode, 21, 9, 7, off)  # that row and total == T + 1: the row's error is reported
      assert call.rc == ECAPACITY and 'batch row 3 longer than 7' in call.message and call.intact()
      assert call.counts[0].value == 22
      call = Raw(pk, res, idx, mode, 22, 3, 8, off)  # n > N: on the host
      assert call.rc == ECAPACITY and call.untouched()
    still_good(off)
  col = bert_collate(pk)
  with pytest.raises(RuntimeError, match='tok_cap'):
    col.collate_rows_fixed(res, idx, mode=0, max_tokens=21, max_seqs=9, max_seqlen=8)
  with pytest.raises(RuntimeError, match='seq_cap'):
    col.collate_rows_fixed(res, idx, mode=0, max_tokens=31, max_seqs=5, max_seqlen=8)
  with pytest.raises(ValueError):
    col.collate_rows_fixed(res, idx, mode=0, max_tokens=0, max_seqs=5, max_seqlen=8)
  still_good()


def test_row_index_out_of_range(gpu):
  pk, res = hand_made()
  col = bert_collate(pk)
  n = res.n_pairs
  for bad in (-1, n, -(1 << 40), 1 << 40):
    with pytest.raises(IndexError):
      col.collate_rows_fixed(res, [1, bad, 2], mode=0, max_tokens=64, max_seqs=16, max_seqlen=8)
    for off in (0, 1):
      call = Raw(pk, res, [1, bad, 2], 0, 64, 16, 8, off)
      assert call.rc == EINDEX and call.intact()
    still_good()
  with pytest.raises(IndexError):  # a range past the end
    col.collate_rows_fixed(res, row0=n - 2, n_rows=3, mode=0, max_tokens=2048, max_seqs=16, max_seqlen=515)
  still_good()


def test_static_position_equal_to_row_length(gpu):
  pk, res = hand_made()
  col = bert_collate(pk)
  keep = res.mlm_pos.clone()
  g = row_of(7)
  k = int(res.mlm_off[g].item()) + 1
  try:
    res.mlm_pos[k] = 7  # the next row's first token here
    with pytest.raises(IndexError):
      col.collate_rows_fixed(res, [g, row_of(8)], mode=1, max_tokens=32, max_seqs=8, max_seqlen=8)
    call = Raw(pk, res, [g, row_of(8)], 1, 32, 8, 8)
    assert call.rc == EINDEX and call.intact()
  finally:
    res.mlm_pos.copy_(keep)
  check_raw([g, row_of(8)], 32, 8, 8, 0, modes=(1,))


def test_codebert_rows_are_refused_by_the_bert_call(gpu):
  from lddl_amd.loader import BertCollate, CodeCollate
  code = CodeCollate(sequence_length_alignment=1, base_seed=SEED)
  res, lens = table(CODE_ROWS, 'codebert')
  res.cls_id, res.sep_id = code.tok.cls_id, code.tok.sep_id
  col = BertCollate(tokenizer=code.tok, sequence_length_alignment=1, base_seed=SEED)
  with pytest.raises(RuntimeError, match='CodeBERT'):
    col.collate_rows_fixed(res, mode=0, max_tokens=1024, max_seqs=32, max_seqlen=129)
  with_doc = [g for g, (_, _, f) in enumerate(CODE_ROWS) if f & 2]  # rows with the [SEP] collate, and the ctx still works
  total = sum(lens[g] for g in with_doc)
  exp = reference(col, res, 0, total + 70, len(with_doc) + 1, 129, rows=with_doc)
  assert_fixed(col.collate_rows_fixed(res, with_doc, mode=0, max_tokens=total + 70, max_seqs=len(with_doc) + 1,
                                      max_seqlen=129), exp)


def test_bad_arguments(gpu):
  """the host-side refusals, through the raw C call: nothing is launched, nothing is written"""
  pk, res = hand_made()
  idx = [row_of(4), row_of(7)]
  null = P(0)
  none64 = ctypes.POINTER(ctypes.c_int64)()
  cases = [(dict(mode=3), EINVAL), (dict(mode=-1), EINVAL), (dict(p=1.5), EINVAL), (dict(p=-0.1), EINVAL),
           (dict(n=0), EINVAL), (dict(n=-1), EINVAL), (dict(n_total=-1), EINVAL),
           (dict(T=-1), EINVAL), (dict(T=1 << 31), ECAPACITY),
           (dict(N=0), ECAPACITY), (dict(N=(1 << 20) + 1), ECAPACITY), (dict(N=1), ECAPACITY),
           (dict(S=2), ECAPACITY), (dict(S=0), ECAPACITY), (dict(S=2049), ECAPACITY),
           (dict(out_total=none64), EINVAL), (dict(out_n_rows=none64), EINVAL), (dict(out_n_seqs=none64), EINVAL)]
  cases += [({k: null}, EINVAL) for k in ('ids', 'src0', 'src1', 'len0', 'len1', 'flags', 'cu', 'input_ids',
                                          'token_type_ids', 'position_ids', 'labels', 'nsl', 'status')]
  for override, rc in cases:
    call = Raw(pk, res, idx, 0, 32, 8, 8, override=override)
    assert call.rc == rc and call.message, (override, call.rc)
    assert call.untouched(), override
  for k in ('mlm_off', 'mlm_pos', 'mlm_label', 'mlm_token'):  # static masking needs its arrays
    call = Raw(pk, res, idx, 1, 32, 8, 8, override={k: null})
    assert call.rc == EINVAL and call.untouched()
  call = Raw(pk, res, idx, 0, 32, 8, 8, override=dict(S=3))  # the smallest max_seqlen: these rows are longer
  assert call.rc == ECAPACITY and 'longer than 3' in call.message and call.intact()
  col = bert_collate(pk)
  for empty in ([], torch.zeros(0, dtype=torch.int64, device='cuda')):
    with pytest.raises(ValueError):
      col.collate_rows_fixed(res, empty, max_tokens=32, max_seqs=8, max_seqlen=8)
  still_good()


# ---- 5. compact targets and shapes over an epoch ------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
def test_compact_mlm(gpu, mode):
  pk, res = packed(mode == 1)
  K = 2000
  idx = list(range(3, 40))
  plain = bert_collate(pk, mlm_probability=0.3)
  plain.counter = COUNTER
  unp = plain.collate_rows_unpadded(res, idx, mode=mode)
  total = int(unp['cu_seqlens'][-1])
  pos, lab, off = plain.mlm_targets(unp['labels'], unp['cu_seqlens'], capacity=K)
  M = int(off[-1])
  assert 0 < M < K
  T, N, S = total + 300, len(idx) + 3 + 4, 128
  col = bert_collate(pk, mlm_probability=0.3, compact_mlm=K)
  col.counter = COUNTER
  out = col.collate_rows_fixed(res, idx, mode=mode, max_tokens=T, max_seqs=N, max_seqlen=S)
  assert col.counter == COUNTER + 1
  assert torch.equal(out['labels'][:total], unp['labels'])
  # the real tokens come first: the positions are those of the unpadded batch
  assert out['masked_lm_positions'].shape == (K,) and torch.equal(out['masked_lm_positions'], pos)
  assert out['masked_lm_labels'].shape == (K,) and torch.equal(out['masked_lm_labels'], lab)
  mo = out['masked_lm_offsets']
  assert mo.shape == (N + 1,) and mo.dtype == torch.int32
  assert torch.equal(mo[:len(idx) + 1], off) and bool((mo[len(idx):] == M).all())  # pad and empty slots add none
  assert 'masked_lm_positions' not in col.collate_rows_fixed(res, idx, mode=0, max_tokens=T, max_seqs=N, max_seqlen=S)


def test_shapes_over_an_epoch(gpu):
  from lddl_amd.loader import RowBatches, fixed_seq_cap
  pk, res = packed(False)
  T, R, S = 2048, 24, 131
  N = fixed_seq_cap(T, R, S)
  fixed, plain = bert_collate(pk, compact_mlm=400), bert_collate(pk)
  shapes, real = None, {k: [] for k in ('input_ids', 'token_type_ids', 'position_ids', 'labels')}
  want = {k: [] for k in real}
  batches = RowBatches(res, max_tokens=T, max_rows=R, seed=1, epoch=0)
  assert len(batches) > 3
  for idx in batches:
    out = fixed.collate_rows_fixed(res, idx, max_tokens=T, max_seqs=N, max_seqlen=S)
    unp = plain.collate_rows_unpadded(res, idx)
    got = {k: (tuple(v.shape), v.dtype) for k, v in out.items() if torch.is_tensor(v)}
    shapes = shapes or got
    assert got == shapes  # every batch has the shapes of the first
    n, total = idx.numel(), int(unp['cu_seqlens'][-1])
    assert (out['num_rows'], out['num_tokens'], out['max_seqlen']) == (n, total, S)
    assert out['num_seqs'] == n + fm.pad_seqs(total, T, S) <= N
    assert out['status'].tolist() == [total, n, out['num_seqs'], S]
    assert torch.equal(out['cu_seqlens'][:n + 1], unp['cu_seqlens']) and int(out['cu_seqlens'][N]) == T
    assert torch.equal(out['next_sentence_labels'][:n], unp['next_sentence_labels'])
    for k in real:
      real[k].append(out[k][:total])
      want[k].append(unp[k])
  assert shapes['input_ids'] == ((T,), torch.int64) and shapes['cu_seqlens'] == ((N + 1,), torch.int32)
  assert shapes['next_sentence_labels'] == ((N,), torch.int64) and shapes['masked_lm_positions'] == ((400,), torch.int64)
  assert shapes['masked_lm_offsets'] == ((N + 1,), torch.int32) and shapes['status'] == ((4,), torch.int32)
  assert fixed.counter == plain.counter == len(batches)
  for k in real:  # the real parts, one after the other, are the unpadded epoch
    assert torch.equal(torch.cat(real[k]), torch.cat(want[k])), k
