"""lddl_rows_from_strings_len + lddl_rows_from_strings (BertCollate.load_rows,
loader.load_shards): the string columns of parquet shards into the GPU row
table that lddl_row_spans + lddl_masked_lm_spans leave behind, against

* the pack result the shards were written from (disk equals memory);
* the string route on the same rows (collate_arrow / to_encoded_inputs);
* the reference's own collate outputs (tests/golden/collate_bert.json.gz);
* a numpy model of str.split() + dict lookup over hand-made columns that put
  tokens and separators on the 64-byte step of the scan;
* lddl_collate_bert under the synthetic vocabularies (ids up to 65535).

Bad input sets the error word, faults nothing and leaves the ctx usable.

Where a masked shard is compared with its pack result, the dense ids are
compared outside the masked positions only: A and B of a masked shard hold
the masked tokens, the packer's dense ids the original ones.  host_tokens()
(which applies mlm_token in both) covers the masked positions.
"""
import ctypes
import functools
import gzip
import io
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEED = 4242
KEYS = ('input_ids', 'token_type_ids', 'attention_mask', 'next_sentence_labels')
EINVAL, EFORMAT, ECAPACITY, EINDEX = -1, -3, -6, -7
S16, S64, S8 = 0x5A5A, 0x5A5A5A5A5A5A5A5A, 0x5A
GUARD = 64
_TMP = {}  # masking -> the directory of its shards


def u16(t):
  return t.cpu().numpy().view(np.uint16).astype(np.int64)


@functools.lru_cache(maxsize=None)
def packed(masking, bin_size=32):
  """the pack of test_collate_rows_gpu.packed: 3 partitions, seq 128, bin 32, dup 2"""
  from lddl_amd import pipeline, synth
  c = synth.make_wiki(40_000, seed=SEED)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0, masking=masking)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 3), torch.device('cuda', 0))
  res = pk.run(sh, target_seq_length=128, bin_size=bin_size, duplicate_factor=2, seed=SEED, masking=masking, spans=True)
  torch.cuda.synchronize()
  assert res.spans and 100 < res.n_pairs < 5000
  return pk, res


def collate_for(tok, align=8, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=tok, sequence_length_alignment=align, **kw)


@functools.lru_cache(maxsize=None)
def loaded(masking):
  """(tokenizer, pack result, the table load_shards makes of its shards, the shards as one Arrow table)"""
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd import writer
  from lddl_amd.loader import load_shards
  pk, res = packed(masking)
  d = tempfile.TemporaryDirectory(prefix='rows_from_strings_')
  _TMP[masking] = d
  writer.write_shards(pk, res, d.name, bin_size=32, masking=masking)
  table = pa.concat_tables([pq.read_table(os.path.join(d.name, 'part.%d.parquet_%d' % (p, b)))
                            for p in range(3) for b in range(res.nbins)])
  got = load_shards(collate_for(pk.tok), d.name)
  return pk.tok, res, got, table


def assert_same(a, b):
  assert set(a) == set(b)
  for k in a:
    assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


# ---- 1. disk equals memory -----------------------------------------------------
@pytest.mark.parametrize('masking', [False, True])
def test_disk_equals_memory(gpu, masking):
  tok, res, got, table = loaded(masking)
  n = res.n_pairs
  assert got.n_pairs == n == table.num_rows and got.n_tokens == res.n_tokens and got.nbins == res.nbins
  assert got.spans and got.tokens is None and got.ntok is None and got.ids_off is None and got.pack is None
  assert (got.cls_id, got.sep_id) == (res.cls_id, res.sep_id)
  for name in ('len0', 'len1', 'flags', 'bins', 'part'):
    a, b = getattr(got, name), getattr(res, name)
    assert a.dtype == b.dtype, name
    assert torch.equal(a[:n], b[:n]), name
  assert torch.equal(got.tok_off[:n + 1], res.tok_off[:n + 1])
  assert torch.equal(got.bin_count, res.bin_count)
  assert np.array_equal(got.host_tokens(), res.host_tokens())
  # the ids the spans select
  l0, l1 = u16(res.len0[:n]), u16(res.len1[:n])
  gi, ri = u16(got.ids), u16(res.ids)
  assert got.ids.dtype == torch.int16 and gi.size == int((l0 + l1).sum()) + 16 and not gi[-16:].any()
  keep = None
  if masking:
    assert got.n_masked == res.n_masked > 0
    assert torch.equal(got.mlm_off[:n + 1], res.mlm_off[:n + 1])
    for name in ('mlm_pos', 'mlm_label', 'mlm_token'):
      assert getattr(got, name).dtype == torch.int16
      assert torch.equal(getattr(got, name)[:res.n_masked], getattr(res, name)[:res.n_masked]), name
    moff, mpos = res.mlm_off[:n + 1].cpu().numpy(), u16(res.mlm_pos[:res.n_masked])
  else:
    assert got.mlm_off is None and got.mlm_token is None and got.n_masked == 0
  gs0, gs1 = got.src0[:n].cpu().numpy(), got.src1[:n].cpu().numpy()
  rs0, rs1 = res.src0[:n].cpu().numpy(), res.src1[:n].cpu().numpy()
  assert np.array_equal(gs1, gs0 + l0) and np.array_equal(gs0, np.concatenate([[0], np.cumsum(l0 + l1)[:-1]]))
  for g in range(n):
    a, b = gi[gs0[g]:gs0[g] + l0[g]], gi[gs1[g]:gs1[g] + l1[g]]
    ea, eb = ri[rs0[g]:rs0[g] + l0[g]], ri[rs1[g]:rs1[g] + l1[g]]
    if masking:  # the shard shows the masked tokens at the masked positions
      keep = np.ones(l0[g] + l1[g] + 3, bool)
      keep[mpos[moff[g]:moff[g + 1]]] = False
      ka, kb = keep[1:1 + l0[g]], keep[2 + l0[g]:2 + l0[g] + l1[g]]
      a, b, ea, eb = a[ka], b[kb], ea[ka], eb[kb]
    assert np.array_equal(a, ea) and np.array_equal(b, eb), g


# ---- 2. the same batches as the string route -----------------------------------
def selections(n):
  rng = np.random.default_rng(5)
  idx = rng.permutation(n)[:45].tolist()
  idx.append(idx[7])  # one repeated row
  return [('all', None, 0, None), ('list', idx, 0, None), ('row0', None, 37, 50)]


@pytest.mark.parametrize('align', [1, 8, 64])
@pytest.mark.parametrize('masking', [False, True])
def test_same_batches_as_strings(gpu, masking, align):
  tok, _, got, table = loaded(masking)
  for name, idx, row0, m in selections(got.n_pairs):
    sub = table.take(idx) if idx is not None else table.slice(row0, m)
    arg = dict(rows=idx) if idx is not None else dict(row0=row0, n_rows=m)
    if masking:
      assert_same(collate_for(tok, align).collate_rows(got, mode=1, **arg), collate_for(tok, align).collate_arrow(sub))
      continue
    d = sub.to_pydict()
    enc = collate_for(tok, align).to_encoded_inputs(list(zip(d['A'], d['B'], d['is_random_next'])))
    assert_same(collate_for(tok, align).collate_rows(got, mode=0, **arg), enc)
    dyn = collate_for(tok, align, base_seed=77).collate_arrow(sub)
    mem = collate_for(tok, align, base_seed=77).collate_rows(got, mode=2, **arg)
    assert_same(mem, dyn)
    assert bool((mem['labels'] != -1).any())


@pytest.mark.parametrize('masking,mode', [(False, 0), (False, 2), (True, 1)])
def test_unpadded_equals_padded(gpu, masking, mode):
  tok, _, got, _ = loaded(masking)
  for name, idx, row0, m in selections(got.n_pairs):
    arg = dict(rows=idx) if idx is not None else dict(row0=row0, n_rows=m)
    pad = collate_for(tok, 1, base_seed=9).collate_rows(got, mode=mode, **arg)
    unp = collate_for(tok, 1, base_seed=9).collate_rows_unpadded(got, mode=mode, **arg)
    keep = pad['attention_mask'].bool()
    lab = 'special_tokens_mask' if mode == 0 else 'labels'
    for k in ('input_ids', 'token_type_ids', lab):
      assert torch.equal(unp[k], pad[k][keep]), (name, k)
    assert torch.equal(unp['next_sentence_labels'], pad['next_sentence_labels'])
    assert torch.equal(unp['cu_seqlens'][1:].long(), keep.sum(1).cumsum(0))


@pytest.mark.parametrize('masking', [False, True])
def test_row_batches_cover_every_row(gpu, masking):
  from lddl_amd.loader import RowBatches
  tok, _, got, _ = loaded(masking)
  n = got.n_pairs
  lens = (u16(got.len0[:n]) + u16(got.len1[:n]) + 3)
  nsl = (got.flags[:n] & 1).long()
  col = collate_for(tok, 8)
  seen = []
  for idx in RowBatches(got, 64):
    out = col.collate_rows(got, idx)
    assert torch.equal(out['next_sentence_labels'], nsl[idx])
    assert np.array_equal(out['attention_mask'].sum(1).cpu().numpy(), lens[idx.cpu().numpy()])
    seen.append(idx.cpu().numpy())
  assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))
  seen = []
  for idx in RowBatches(got, max_tokens=2048):
    out = col.collate_rows_unpadded(got, idx)
    assert out['input_ids'].numel() == int(lens[idx.cpu().numpy()].sum()) <= 2048
    assert torch.equal(out['next_sentence_labels'], nsl[idx])
    seen.append(idx.cpu().numpy())
  assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))


# ---- 3. the reference's own goldens ----------------------------------------------
def golden_cases():
  with gzip.open(os.path.join(GOLDEN, 'collate_bert.json.gz'), 'rt', encoding='utf-8') as f:
    return json.load(f)


CASES = golden_cases()


@functools.lru_cache(maxsize=None)
def tokenizer(vocab_file):
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(vocab_file, 0)


def test_goldens_cover_both_vocabularies():
  assert len(CASES) == 10 and {c['vocab'] for c in CASES} == {'bert', 'codebert'}
  assert any(c['static'] for c in CASES) and any(not c['static'] for c in CASES)


@pytest.mark.parametrize('k', range(len(CASES)))
def test_reference_goldens(gpu, k):
  c = CASES[k]
  tok = tokenizer({'bert': _lib.VOCAB_BERT, 'codebert': _lib.VOCAB_CODEBERT}[c['vocab']])
  if c['static']:
    batch = [(a, b, rn, bytes.fromhex(p), l) for a, b, rn, p, l in
             zip(c['A'], c['B'], c['is_random_next'], c['positions_npy'], c['labels_str'])]
  else:
    batch = list(zip(c['A'], c['B'], c['is_random_next']))
  col = collate_for(tok, c['align'], ignore_index=c['ignore_index'])
  table = col.load_rows(batch)
  out = col.collate_rows(table, mode=1 if c['static'] else 0)
  for key in KEYS + ('labels' if c['static'] else 'special_tokens_mask',):
    assert np.array_equal(out[key].cpu().numpy(), np.asarray(c[key], np.int64)), key


# ---- 4. hand-made columns against str.split() + dict lookup ----------------------
def npy(positions):
  f = io.BytesIO()
  np.save(f, np.asarray(positions, np.uint16))
  return f.getvalue()


def model(tok, rows):
  """rows: (A, B, is_random_next[, np.save bytes of the positions, labels string]) -> the table as numpy arrays"""
  ids_of = lambda s: [tok.vocab.get(t, tok.unk_id) for t in s.split()]  # noqa: E731
  out = {k: [] for k in ('len0', 'len1', 'flags', 'ids', 'mlm_k', 'mlm_pos', 'mlm_label', 'mlm_token')}
  for row in rows:
    a, b = ids_of(row[0]), ids_of(row[1])
    out['len0'].append(len(a))
    out['len1'].append(len(b))
    out['flags'].append((1 if row[2] else 0) | 2)
    out['ids'] += a + b
    if len(row) > 3:
      shown = [tok.cls_id] + a + [tok.sep_id] + b + [tok.sep_id]
      lab = ids_of(row[4])
      pos = np.load(io.BytesIO(row[3])).tolist()  # lddl/utils.py deserialize_np_array
      assert len(lab) == len(pos)
      out['mlm_k'].append(len(lab))
      out['mlm_pos'] += pos
      out['mlm_label'] += lab
      out['mlm_token'] += [shown[p] for p in pos]
  o = {k: np.asarray(v, np.int64) for k, v in out.items()}
  ab = o['len0'] + o['len1']
  o['src0'] = np.concatenate([[0], np.cumsum(ab)[:-1]])
  o['src1'] = o['src0'] + o['len0']
  o['tok_off'] = np.concatenate([[0], np.cumsum(ab + 3)])
  if len(rows[0]) > 3:
    o['mlm_off'] = np.concatenate([[0], np.cumsum(o['mlm_k'])])
  return o


class Guarded:
  """n elements between GUARD sentinel elements on each side (pad more zeroed elements behind the n, in front
  of the back sentinels), at an aligned base (shift 0) or one element off"""

  def __init__(self, n, dtype, shift, pad=0):
    self.sent = {torch.int16: S16, torch.int64: S64, torch.uint8: S8}[dtype]
    self.n, self.pad, self.lo = n, pad, GUARD + shift
    self.full = torch.full((self.lo + n + pad + GUARD,), self.sent, dtype=dtype, device='cuda')
    assert self.full.data_ptr() % 16 == 0
    if pad:
      self.full[self.lo + n:self.lo + n + pad] = 0
    self.ptr = ctypes.c_void_p(self.full.data_ptr() + self.lo * self.full.element_size())

  def get(self):
    """the n elements, after checking the sentinels and the padding"""
    h = self.full.cpu().numpy()
    assert (h[:self.lo] == h.dtype.type(self.sent)).all() and (h[self.lo + self.n + self.pad:] == h.dtype.type(self.sent)).all()
    assert not h[self.lo + self.n:self.lo + self.n + self.pad].any()
    v = h[self.lo:self.lo + self.n]
    return v.view(np.uint16).astype(np.int64) if v.dtype == np.int16 else v.astype(np.int64)

  def untouched(self):
    h = self.full.cpu().numpy()
    keep = np.ones(h.size, bool)
    keep[self.lo + self.n:self.lo + self.n + self.pad] = False
    return bool((h[keep] == h.dtype.type(self.sent)).all())


def run_raw(tok, rows, shift=0, ids_short=0, mlm_short=0, tamper=None, n_rows=None, null_a=False, static_out=None):
  """both C calls over guarded outputs -> (rc of the length call, rc of the fill call or None, outputs)"""
  from lddl_amd import loader
  from lddl_amd.tokenizer import _stream
  L = _lib.lib()
  P = ctypes.c_void_p
  static = len(rows[0]) > 3
  cols = [loader._column([r[0] for r in rows], True), loader._column([r[1] for r in rows], True)]
  if static:
    cols += [loader._column([r[3] for r in rows], False), loader._column([r[4] for r in rows], True)]
  rn = np.asarray([1 if r[2] else 0 for r in rows], np.uint8)
  dev, host, ptrs = collate_for(tok)._upload(cols, rn)
  n = len(rows) if n_rows is None else n_rows
  inp = [P(x) for x in ptrs[:8]] if static else [P(x) for x in ptrs[:4]] + [P(0)] * 4
  if null_a:
    inp[0] = P(0)
  static_out = static if static_out is None else static_out
  m = len(rows)
  g = {'len0': Guarded(m, torch.int16, shift), 'len1': Guarded(m, torch.int16, shift),
       'src0': Guarded(m, torch.int64, shift), 'src1': Guarded(m, torch.int64, shift),
       'tok_off': Guarded(m + 1, torch.int64, shift)}
  if static_out:
    g['mlm_off'] = Guarded(m + 1, torch.int64, shift)
  tot = (ctypes.c_int64 * 3)(-1, -1, -1)
  moff = g['mlm_off'].ptr if static_out else P(0)
  rc = L.lddl_rows_from_strings_len(tok.handle, *inp, n, g['len0'].ptr, g['len1'].ptr, g['src0'].ptr, g['src1'].ptr,
                                    g['tok_off'].ptr, moff, tot, _stream())
  if rc:
    return rc, None, g, None
  n_ids, n_mask, n_tok = tot[0], tot[1], tot[2]
  if tamper:
    tamper(g)
  g['ids'] = Guarded(n_ids, torch.int16, shift, pad=16)
  g['flags'] = Guarded(m, torch.uint8, shift)
  mp = [P(0)] * 3
  if static_out:
    for k in ('mlm_pos', 'mlm_label', 'mlm_token'):
      g[k] = Guarded(n_mask, torch.int16, shift)
    mp = [g[k].ptr for k in ('mlm_pos', 'mlm_label', 'mlm_token')]
  rc2 = L.lddl_rows_from_strings(tok.handle, *inp, P(ptrs[-1]), n, g['len0'].ptr, g['len1'].ptr, g['src0'].ptr,
                                 g['src1'].ptr, moff, g['ids'].ptr, n_ids - ids_short, g['flags'].ptr, *mp,
                                 n_mask - mlm_short, _stream())
  torch.cuda.synchronize()
  del dev, host
  return rc, rc2, g, (n_ids, n_mask, n_tok)


def assert_raw(tok, rows, shift=0):
  rc, rc2, g, tot = run_raw(tok, rows, shift)
  assert (rc, rc2) == (0, 0), (rc, rc2, _lib.lib().lddl_last_error())
  exp = model(tok, rows)
  assert tot == (exp['ids'].size, exp['mlm_pos'].size, int(exp['tok_off'][-1]))
  for k, buf in g.items():
    assert np.array_equal(buf.get(), exp[k]), k


F15 = 'the ' * 15  # 60 bytes
SEPS = ([chr(c) for c in list(range(9, 14)) + list(range(0x1c, 0x21))] +
        ['\x85', '\xa0', '\u1680'] + [chr(c) for c in range(0x2000, 0x200b)] +
        ['\u2028', '\u2029', '\u202f', '\u205f', '\u3000'])  # every class py_space knows


def edge_rows():
  rows = []
  for pre in ('', ' ', '  '):  # 'and' ends at byte 63, 64, 65
    rows.append((pre + F15 + 'and of', 'world', 0))
  rows.append((F15 + 'hello world', F15 + 'hel' + 'lo', 1))  # a token across the 64-byte step
  rows.append(('the' + 'of'.join(SEPS) + 'and', ''.join('in' + s for s in SEPS), 0))  # every separator class
  for sep in ('\x85', '\xa0', '\u2028', '\u3000'):  # 2- and 3-byte separators across the step edge
    for fill in ('an', 'and', 'and.'):  # the separator starts at byte 62, 63, 64
      rows.append((F15 + fill + sep + 'of the', F15 + F15 + ' ' + fill + sep + sep + 'of', 1))
  rows.append(('  \t the   of \n ', '\u3000\u3000is\u2028', 0))  # leading, trailing, repeated whitespace
  rows += [('', 'the of', 0), ('the of', '', 1), ('', '', 0), (' \t\n', '\u3000 \x85', 1)]  # empty segments
  rows.append(('qzxvjkqq the ' + 'a' * 259 + ' of ' + 'b' * 300, 'x' * 256 + ' and', 0))  # misses, long tokens
  rows.append(('the [CLS] of [SEP] [MASK] [UNK] [PAD]', '[MASK] [SEP]', 1))
  rows.append(('the ' * 2045, 'of', 0))
  rows.append(('é\u3000日本 the\xa0naïve', 'ß of', 1))
  return rows


def short_rows(n, seed):
  words = ['the', 'of', 'and', 'hello', 'world', 'qqzz', 'in', '[MASK]', 'é', 'was']
  rng = np.random.default_rng(seed)
  pick = lambda k: ' '.join(words[j] for j in rng.integers(0, len(words), k))  # noqa: E731
  return [(pick(int(rng.integers(0, 7))), pick(int(rng.integers(0, 5))), int(rng.integers(0, 2))) for _ in range(n)]


def masked_rows():
  a, b = 'the of and in was', 'hello world is for'  # len0 5, len1 4, n 12
  n, l0 = 12, 5
  some = [0, 1, l0, l0 + 1, l0 + 2, n - 2, n - 1]
  lab = lambda k: ' '.join(['the', 'qqzz', 'of', '[MASK]', 'and', 'world'][j % 6] for j in range(k))  # noqa: E731
  rows = [(a, b, 0, npy(some), lab(len(some))),
          (a, b, 1, npy([]), ''),  # no positions between rows that have some
          (a, b, 0, npy(list(range(n))), lab(n)),  # every token of the row
          ('', '', 1, npy([2, 0, 1]), lab(3)),
          (F15 + 'and', 'of', 0, npy([16, 18, 3]), '  the \u3000 of\tand '),
          ('the', 'of', 1, npy([1]), 'hello')]
  rng = np.random.default_rng(11)
  for _ in range(70):  # more rows than one wave of the scan holds
    k = int(rng.integers(0, 6))
    rows.append((a, b, 0, npy(sorted(rng.permutation(n)[:k].tolist())), lab(k)))
  return rows


@pytest.mark.parametrize('shift', [0, 1])
def test_edge_rows(gpu, shift):
  assert_raw(tokenizer(_lib.VOCAB_BERT), edge_rows(), shift)


@pytest.mark.parametrize('shift', [0, 1])
def test_masked_rows(gpu, shift):
  assert_raw(tokenizer(_lib.VOCAB_BERT), masked_rows(), shift)


@pytest.mark.parametrize('n', [1, 257, -1])
def test_batch_sizes(gpu, n):
  if n < 0:  # more than one pass of the grid: n_cu * 8 blocks of four rows
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 5
  assert_raw(tokenizer(_lib.VOCAB_BERT), short_rows(n, n), 0)


def short_masked_rows(n, seed):
  """two or three tokens per segment, one or two masked positions, every seventh row none"""
  words = ['the', 'of', 'and', 'hello', 'world', 'qqzz', 'in', '[MASK]']
  rng = np.random.default_rng(seed)
  pick = lambda k: ' '.join(words[j] for j in rng.integers(0, len(words), k))  # noqa: E731
  rows = []
  for r in range(n):
    la, lb = int(rng.integers(2, 4)), int(rng.integers(2, 4))
    k = 0 if r % 7 == 3 else int(rng.integers(1, 3))
    rows.append((pick(la), pick(lb), r & 1, npy(sorted(rng.permutation(la + lb + 3)[:k].tolist())), pick(k)))
  return rows


def table_arrays(res):
  """a load_rows result as the arrays of model()"""
  n = res.n_pairs
  o = {k: u16(getattr(res, k)[:n]) for k in ('len0', 'len1')}
  o['flags'] = res.flags[:n].cpu().numpy().astype(np.int64)
  o['ids'] = u16(res.ids)[:int((o['len0'] + o['len1']).sum())]
  for k in ('src0', 'src1'):
    o[k] = getattr(res, k)[:n].cpu().numpy()
  for k in ('tok_off', 'mlm_off'):
    o[k] = getattr(res, k)[:n + 1].cpu().numpy()
  for k in ('mlm_pos', 'mlm_label', 'mlm_token'):
    o[k] = u16(getattr(res, k)[:res.n_masked])
  return o


@pytest.mark.parametrize('n', [2047, 2048, 2049])
def test_static_rows_across_a_scan_chunk(gpu, n):
  """both scanned quantities, ids and masked entries, up to and across the base of the scan's second chunk of
  2048 rows: the table of n rows against the host model and against the same rows loaded in two halves"""
  tok = tokenizer(_lib.VOCAB_BERT)
  rows = short_masked_rows(n, 5)
  col = collate_for(tok)
  exp = model(tok, rows)
  assert exp['mlm_off'][2047] > 0 and (exp['mlm_k'] == 0).sum() > 100
  whole = col.load_rows(rows)
  assert (whole.n_pairs, whole.n_tokens, whole.n_masked) == (n, int(exp['tok_off'][-1]), exp['mlm_pos'].size)
  got = table_arrays(whole)
  for k, v in got.items():
    assert np.array_equal(v, exp[k]), k
  h = n // 2
  lo, hi = table_arrays(col.load_rows(rows[:h])), table_arrays(col.load_rows(rows[h:]))
  for k in ('len0', 'len1', 'flags', 'ids', 'mlm_pos', 'mlm_label', 'mlm_token'):
    assert np.array_equal(got[k], np.concatenate([lo[k], hi[k]])), k
  for k, base in (('src0', lo['ids'].size), ('src1', lo['ids'].size), ('tok_off', lo['tok_off'][-1]),
                  ('mlm_off', lo['mlm_off'][-1])):
    first = lo[k] if k in ('src0', 'src1') else lo[k][:-1]
    assert np.array_equal(got[k], np.concatenate([first, hi[k] + base])), k


def test_segment_of_65535_tokens(gpu):
  tok = tokenizer(_lib.VOCAB_BERT)
  assert_raw(tok, [('the', 'of', 0), ('a ' * 65535, 'b\n' * 65535, 1), ('and', '', 0)])
  for rows in ([('the', 'of', 0), ('a ' * 65536, 'b', 1)], [('the', 'b ' * 65536, 1)]):
    rc, _, _, _ = run_raw(tok, rows)
    assert rc == ECAPACITY and b'65535' in _lib.lib().lddl_last_error()
  assert_raw(tok, edge_rows()[:6])


# ---- 5. refusals; the next call is right after each ------------------------------
def test_capacity_one_short(gpu):
  tok = tokenizer(_lib.VOCAB_BERT)
  rows = masked_rows()
  for short in (dict(ids_short=1), dict(mlm_short=1)):
    rc, rc2, g, _ = run_raw(tok, rows, **short)
    assert (rc, rc2) == (0, ECAPACITY)
    for k in ('ids', 'flags', 'mlm_pos', 'mlm_label', 'mlm_token'):
      assert g[k].untouched(), k
    assert_raw(tok, rows)
  rc, rc2, g, _ = run_raw(tok, edge_rows(), ids_short=1)
  assert (rc, rc2) == (0, ECAPACITY) and g['ids'].untouched() and g['flags'].untouched()
  assert_raw(tok, edge_rows())


def test_format_and_index_refusals(gpu):
  tok = tokenizer(_lib.VOCAB_BERT)
  good = masked_rows()[:6]
  a, b, n = good[0][0], good[0][1], 12
  ok = npy([1, 2])
  bad = [(EFORMAT, (a, b, 0, b'\x92' + ok[1:], 'the of')),   # magic broken
         (EFORMAT, (a, b, 0, ok + b'\x00', 'the of')),         # an odd payload
         (EFORMAT, (a, b, 0, ok[:8], 'the of')),               # shorter than its header
         (EFORMAT, (a, b, 0, ok, 'the')),                      # one label too few
         (EFORMAT, (a, b, 0, ok, 'the of and')),               # one too many
         (EINDEX, (a, b, 0, npy([1, n]), 'the of')),           # a position equal to n_r
         (EINDEX, ('', '', 0, npy([3]), 'the'))]
  for code, row in bad:
    rows = good[:3] + [row] + good[3:]
    rc, rc2, _, _ = run_raw(tok, rows)
    assert rc == code and rc2 is None, (rc, code, _lib.lib().lddl_last_error())
    assert b'row 3' in _lib.lib().lddl_last_error()
    assert_raw(tok, good)
  with pytest.raises(IndexError):
    collate_for(tok).load_rows([bad[5][1]])
  with pytest.raises(RuntimeError):
    collate_for(tok).load_rows([bad[0][1]])


def test_invalid_arguments(gpu):
  tok = tokenizer(_lib.VOCAB_BERT)
  rows, plain = masked_rows()[:6], edge_rows()[:6]
  for kw, r in ((dict(n_rows=0), plain), (dict(n_rows=-1), plain), (dict(null_a=True), plain),
                (dict(static_out=True), plain),    # static outputs without static inputs
                (dict(static_out=False), rows)):   # and the reverse
    rc, rc2, g, _ = run_raw(tok, r, **kw)
    assert rc == EINVAL and rc2 is None, kw
    for k, buf in g.items():
      assert buf.untouched(), k
    assert_raw(tok, r)
  with pytest.raises(ValueError):
    collate_for(tok).load_rows([])


@pytest.mark.parametrize('delta', [1, -1])
def test_fill_checks_the_length_pass(gpu, delta):
  """len0 of one row altered after the length pass: the fill refuses the row and leaves it unwritten"""
  tok = tokenizer(_lib.VOCAB_BERT)
  rows = masked_rows()
  victim = 4  # 16 + 1 tokens, three positions
  exp = model(tok, rows)

  def tamper(g):
    g['len0'].full[g['len0'].lo + victim] += delta
  rc, rc2, g, _ = run_raw(tok, rows, tamper=tamper)
  assert (rc, rc2) == (0, EINVAL) and b'row 4' in _lib.lib().lddl_last_error()
  ids, mpos, flags = g['ids'].get(), g['mlm_pos'].get(), g['flags'].get()
  s0, m0 = int(exp['src0'][victim]), int(exp['mlm_off'][victim])
  assert (ids[s0:s0 + 17] == S16).all() and (mpos[m0:m0 + 3] == S16).all() and flags[victim] == S8
  for r in (0, 2, 5, 40):  # the other rows hold their own
    s = int(exp['src0'][r])
    e = s + int(exp['len0'][r] + exp['len1'][r])
    assert np.array_equal(ids[s:e], exp['ids'][s:e]) and flags[r] == exp['flags'][r]
  assert_raw(tok, rows)


def test_codebert_shards_are_refused(gpu, tmp_path):
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd.loader import load_shards
  t = pa.table({'id': ['d0'], 'doc': ['the of'], 'code': ['x = 1'], 'num_tokens': pa.array([7], pa.uint16())})
  pq.write_table(t, str(tmp_path / 'part.0.parquet'))
  col = collate_for(tokenizer(_lib.VOCAB_BERT))
  with pytest.raises(ValueError, match='CodeBERT'):
    load_shards(col, str(tmp_path))
  with pytest.raises(ValueError, match='CodeBERT'):
    col.load_rows(t)


def test_balanced_directory(gpu, tmp_path):
  """the directory the load balancer makes of the shards (shard-<k>.parquet_<b>, what a training job reads)"""
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd import balance
  from lddl_amd.loader import load_shards
  from lddl_amd import writer
  pk, res = packed(True, 64)  # two bins, both with rows for two shards: the balancer refuses a bin it cannot spread
  tok = pk.tok
  src, bal = str(tmp_path / 'sink'), str(tmp_path / 'bal')
  writer.write_shards(pk, res, src, bin_size=64, masking=True)
  assert res.nbins == 2
  _, ns = balance.main(balance.attach_args().parse_args(['--indir', src, '--outdir', bal, '--num-shards', '2',
                                                         '--keep-orig']), rank=0, world=1)
  assert sorted(ns) == sorted('shard-%d.parquet_%d' % (k, b) for k in range(2) for b in range(res.nbins))
  assert os.path.exists(os.path.join(bal, '.num_samples.json'))
  got = load_shards(collate_for(tok), bal)
  order = [(k, b) for k in range(2) for b in range(res.nbins) if ns['shard-%d.parquet_%d' % (k, b)]]
  table = pa.concat_tables([pq.read_table(os.path.join(bal, 'shard-%d.parquet_%d' % kb)) for kb in order])
  n = res.n_pairs
  assert got.n_pairs == n == table.num_rows and got.nbins == res.nbins and got.n_masked == res.n_masked
  assert np.array_equal(got.part.cpu().numpy(), np.concatenate([np.full(ns['shard-%d.parquet_%d' % kb], kb[0]) for kb in order]))
  assert np.array_equal(got.bins.cpu().numpy(), np.concatenate([np.full(ns['shard-%d.parquet_%d' % kb], kb[1]) for kb in order]))
  assert np.array_equal(got.bin_count.cpu().numpy(), [[ns['shard-%d.parquet_%d' % (k, b)] for b in range(res.nbins)]
                                                      for k in range(2)])
  assert_same(collate_for(tok, 8).collate_rows(got, mode=1), collate_for(tok, 8).collate_arrow(table))
  # every row of the pack result once
  key = lambda r: (tuple(r[5]), r[3] & 1, r[4], tuple(r[6]), tuple(r[7]))  # noqa: E731
  assert sorted(key(r) for r in got.rows()) == sorted(key(r) for r in res.rows())


def test_arrow_inputs(gpu):
  """a table, a list of tables (large_string among them, one sliced) and the samples give one table"""
  import pyarrow as pa
  tok, _, got, table = loaded(True)
  col = collate_for(tok)
  n = 90
  sub = table.slice(0, n)
  whole = col.load_rows(sub)
  large = sub.slice(40, 50).cast(pa.schema([f.with_type(pa.large_string()) if f.type == pa.string() else f
                                            for f in sub.schema]))
  batch = large.combine_chunks().to_batches()[0]
  assert batch.num_rows == 50
  parts = col.load_rows([sub.slice(0, 40), batch])
  d = sub.to_pydict()
  tuples = col.load_rows(list(zip(d['A'], d['B'], d['is_random_next'], d['masked_lm_positions'], d['masked_lm_labels'])))
  for other in (parts, tuples):
    for name in ('len0', 'len1', 'flags', 'ids', 'src0', 'src1', 'tok_off', 'mlm_off', 'mlm_pos', 'mlm_label', 'mlm_token'):
      assert torch.equal(getattr(other, name), getattr(whole, name)), name
  assert whole.nbins == 1 and not whole.bins.any() and not whole.part.any()
  assert torch.equal(whole.len0[:n], got.len0[:n])


# ---- 6. synthetic vocabularies -----------------------------------------------------
@pytest.mark.parametrize('name', ['dupspecial', 'utf8', 'specials', 'v65536', 'v32769'])
def test_synthetic_vocabularies(gpu, name):
  import synth_vocab
  tok = tokenizer(synth_vocab.vocab_path(name))
  words = [w for w in tok.ids_to_tokens if w.split() == [w]] + ['notinvocab', 'zzqqé', 'a' * 300]
  per = 250
  segs = [' '.join(words[i:i + per]) for i in range(0, len(words), per)]
  if len(segs) % 2:
    segs.append('')
  batch = [(segs[i], segs[i + 1], (i // 2) & 1) for i in range(0, len(segs), 2)]
  col = collate_for(tok, 8)
  exp = col.to_encoded_inputs(batch)  # lddl_collate_bert mode 0
  out = col.collate_rows(col.load_rows(batch), mode=0)
  assert_same(out, exp)
  top = int(out['input_ids'].max())
  if name.startswith('v'):
    assert top == tok.vocab_size - 1 and top > 32767  # ids beyond int16 survive the int16 views
