"""Span dynamic masking (lddl_set_span_mask) on every route that masks
dynamically, bit for bit against tests/span_model.py: mode 2 of collate_rows,
collate_rows_unpadded and collate_rows_fixed (BERT, CodeBERT and MLM-only rows,
the wide and the narrow path of each), of the string route, and mask_tokens.

The rows are hand-made row tables (as tests/test_wwm_gpu.py builds its own),
mostly over the 'tiny65' vocabulary of tests/synth_vocab.py: ids 5..30 are the
letters, 31..56 their '##' forms, 63 and 64 '##ing' and '##ed'; [CLS] 2,
[SEP] 3, [MASK] 4, 65 entries.  'tiny6' has no '##' entry; the bundled BERT
vocabulary has thousands.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mask_model as mm
import span_model as sm
import synth_vocab as sv
import wwm_model as wm
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

VOCAB, V, CLS, SEP, MASK, IGNORE = 'tiny65', 65, 2, 3, 4, -1
SEED, COUNTER = 31, 0  # a draw at which every case of cases_covered occurs, under each of the four (law, p)
LAWS = [(10, 0.2), (3, 0.5)]  # (max_span, geo_p)
PS = [0.15, 0.5]
EINVAL = -1


def w(i):
  return 5 + i % 26


def c(i):
  return 31 + i % 26


def word(k, i=0):
  """a word of k pieces"""
  return [w(i)] + [c(i + t) for t in range(k - 1)]


def pieces(k, i=0):
  """k '##' pieces without the piece that heads them"""
  return [c(i + t) for t in range(k)]


def plain(k, i=0):
  return [w(i + t) for t in range(k)]


def mix(k, seed):
  """k tokens, about half of them '##' pieces: words of one to a few pieces"""
  rng = np.random.default_rng(seed)
  return [c(int(x)) if y < 0.5 else w(int(x)) for x, y in zip(rng.integers(0, 26, k), rng.random(k))]


def sized(n, seed):
  """a BERT row of n columns"""
  a = (n - 3) * 2 // 3
  return (mix(a, seed), mix(n - 3 - a, seed + 100), 1, seed & 1)


SIZES = [3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 257, 512]
# (A / doc, B / code, s, is_random_next).  Columns: [CLS] 0, A 1 .. a, [SEP] a + 1, B from a + 2.
ROWS = [sized(n, k) for k, n in enumerate(SIZES)] + [
    # 12: words over columns 62..65 and 126..129: across 63/64 and 127/128
    (plain(61) + word(4, 3) + plain(60, 7) + word(4, 11) + plain(3), word(2, 5) + plain(1), 1, 0),
    # 13: a = 1 and b = 1
    (plain(1, 3), plain(1, 8), 1, 1),
    # 14: every token a '##' piece: each segment is one word
    (pieces(40, 2), pieces(30, 9), 1, 0),
    # 15, 16: every token its own word: heads in every lane, spans from one step into the next, past both [SEP]s
    (plain(200, 1), plain(100, 4), 1, 1),
    (plain(129, 6), plain(3, 2), 1, 0),
    # 17: one word of 509 pieces
    (word(509, 1), [], 1, 0),
    # 18: CodeBERT with docstring, the code begins with '##' pieces
    (word(3, 2) + plain(2), pieces(3, 7) + mix(70, 50), 1, 0),
    # 19 .. 22: CodeBERT without docstring / MLM-only rows ([CLS] tokens [SEP]): 104, 8, 64 and 129 columns
    ([], pieces(2, 3) + mix(100, 51), 0, 0),
    ([], plain(6, 4), 0, 0),
    ([], mix(62, 52), 0, 0),
    ([], mix(127, 53), 0, 0),
    # 23: the same, 63 columns
    ([], mix(61, 54), 0, 0),
]
BERT = list(range(18))
WIDE = BERT                              # with alignment 8: seq_len 512, even
NARROW = [10, 12, 0, 15, 16, 1, 14, 7]   # with alignment 1: seq_len 303, odd
CODE_ROWS = [18, 19, 20, 16, 21, 22, 13, 4]  # an odd total, an even one without the last row; the longest is odd
MLM_ROWS = [23, 19, 23, 20, 21, 22]          # likewise


def row_len(rows, g):
  a, b, s, _ = rows[g]
  return len(a) + len(b) + 2 + s


@functools.lru_cache(maxsize=None)
def _tok(vocab):
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(_lib.VOCAB_BERT if vocab == 'bert' else sv.vocab_path(vocab), 0)


def tok(vocab=VOCAB):
  """one Tokenizer, and so one ctx with its switches, per vocabulary"""
  return _tok(vocab)


@functools.lru_cache(maxsize=None)
def cont_table(vocab=VOCAB):
  return wm.cont_table(tok(vocab).ids_to_tokens)


def make_table(rows, cls, sep):
  """rows as a PackResult with spans"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  n = len(rows)
  ids, src0, src1 = [0], [], []  # (an id in front: no span starts at 0)
  for a, b, _, _ in rows:
    src0.append(len(ids))
    ids += a
    src1.append(len(ids))
    ids += b
  lens = np.asarray([row_len(rows, g) for g in range(n)], np.int64)

  def t(a, dt):
    a = np.ascontiguousarray(np.asarray(a, dt))
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t([len(r[0]) for r in rows], np.uint16), t([len(r[1]) for r in rows], np.uint16),
      t([r[2] * 2 + r[3] for r in rows], np.uint8), t(np.zeros(n), np.uint8), t(np.zeros(n), np.int64),
      t([[n]], np.int64))
  res.ids, res.src0, res.src1 = t(ids + [0] * 16, np.uint16), t(src0, np.int64), t(src1, np.int64)
  res.cls_id, res.sep_id = cls, sep
  return res


@functools.lru_cache(maxsize=None)
def table():
  assert tok().vocab_size == V and (tok().cls_id, tok().sep_id, tok().mask_id) == (CLS, SEP, MASK)
  assert np.flatnonzero(cont_table()).tolist() == list(range(31, 57)) + [63, 64]
  return make_table(ROWS, CLS, SEP)


def planes(idx, S, rows=ROWS, cls=CLS, sep=SEP):
  """the unmasked batch: ids, special (the special tokens and the padding), token_type_ids, attention_mask"""
  n = len(idx)
  ids, sp, tt, am = (np.zeros((n, S), np.int64) for _ in range(4))
  sp[:] = 1
  for r, g in enumerate(idx):
    a, b, s, _ = rows[g]
    row = [cls] + a + [sep] * s + b + [sep]
    ids[r, :len(row)] = row
    am[r, :len(row)] = 1
    sp[r, 1:1 + len(a)] = 0
    sp[r, 1 + len(a) + s:len(row) - 1] = 0
    if s:
      tt[r, len(a) + 2:len(row)] = 1
  return ids, sp, tt, am


def collate(kind, span, p=0.15, seed=SEED, counter=COUNTER, align=8, vocab=VOCAB, **kw):
  from lddl_amd import loader
  cls = {'bert': loader.BertCollate, 'code': loader.CodeCollate, 'mlm': loader.MlmCollate}[kind]
  col = cls(tokenizer=tok(vocab), sequence_length_alignment=align, base_seed=seed, mlm_probability=p, span_mask=span,
            **kw)
  col.counter = counter
  return col


@functools.lru_cache(maxsize=None)
def expect(idx, S, p, law, seed=SEED, counter=COUNTER):
  """the model's batch of ROWS[idx] padded to S, computed once and shared (nobody writes to it)"""
  ids, sp, tt, am = planes(idx, S)
  return sm.mask(ids, sp, cont_table(), seed, counter, p, law[0], law[1], MASK, V, IGNORE), (ids, sp, tt, am)


def host(t):
  return t.cpu().numpy()


def check_padded(out, idx, S, p, law, nsl=True):
  m, (ids, sp, tt, am) = expect(tuple(idx), S, p, law)
  assert tuple(out['input_ids'].shape) == (len(idx), S)
  assert np.array_equal(host(out['labels']), m.labels)
  assert np.array_equal(host(out['input_ids']), m.input_ids)
  assert np.array_equal(host(out['token_type_ids']), tt) and np.array_equal(host(out['attention_mask']), am)
  if nsl:
    assert host(out['next_sentence_labels']).tolist() == [ROWS[g][3] for g in idx]
  return m, am != 0


def check_stream(flat, pad, keep, lens):
  """a padding-free batch is the padded one with its pad columns dropped"""
  assert np.array_equal(np.diff(host(flat['cu_seqlens'])), lens)
  assert np.array_equal(host(flat['input_ids']), host(pad['input_ids'])[keep])
  assert np.array_equal(host(flat['labels']), host(pad['labels'])[keep])
  assert np.array_equal(host(flat['token_type_ids']), host(pad['token_type_ids'])[keep])
  assert np.array_equal(host(flat['position_ids']), np.concatenate([np.arange(n) for n in lens]))


def cases_covered(m, idx):
  """what the rows are there for happens at this draw (the model says so; the kernels are then held to it)"""
  r12, r14 = idx.index(12), idx.index(14)
  sel, op, ln, wd = m.select, m.open, m.length, m.word
  # an open head in the last lane of a step (column 63 or 127) whose span ends in the next step, over another word
  assert any(op[r, j] and ln[r, j] >= 2 and wd[r, j + 1] == wd[r, j] + 1 and sel[r, j + 1] for r in range(len(idx))
             for j in (63, 127))
  # a word across 63/64 or 127/128 selected as a whole, and one left whole
  for lo in (62, 126):
    assert sel[r12, lo:lo + 4].all() or not sel[r12, lo:lo + 4].any()
  # spans clipped at the [SEP] after A and at the final [SEP]: the head's length passes the words that are left
  clipped = [0, 0]
  for r, g in enumerate(idx):
    a, n = len(ROWS[g][0]), row_len(ROWS, g)
    for j in np.flatnonzero(op[r]):
      last = a if j <= a else n - 2
      clipped[int(j > a)] += bool(wd[r, j] + ln[r, j] - 1 > wd[r, last])
  assert clipped[0] and clipped[1]
  assert not sel[:, 0].any() and all(not sel[r, len(ROWS[g][0]) + 1] for r, g in enumerate(idx))
  # each all-'##' segment is one word: selected as a whole or not at all
  for lo, hi in ((1, 41), (42, 72)):
    assert sel[r14, lo:hi].all() or not sel[r14, lo:hi].any()
  # overlapping spans: an open head inside the span of the open head before it, in one segment
  overlaps = 0
  for r, g in enumerate(idx):
    heads, a = np.flatnonzero(op[r]), len(ROWS[g][0])
    overlaps += sum(1 for h, j in zip(heads, heads[1:]) if (h <= a) == (j <= a) and wd[r, j] < wd[r, h] + ln[r, h])
  assert overlaps


@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('law', LAWS)
def test_bert_routes(gpu, law, p):
  """collate_rows wide and narrow, collate_rows_unpadded (pairs and lane = token), collate_rows_fixed, mask_tokens"""
  res = table()
  pad = collate('bert', law, p).collate_rows(res, WIDE)
  m, keep = check_padded(pad, WIDE, 512, p, law)
  cases_covered(m, WIDE)
  assert (m.select & ~m.open).any() and m.select.mean() > 0.02
  narrow = collate('bert', law, p, align=1).collate_rows(res, NARROW)
  check_padded(narrow, NARROW, 303, p, law)
  lens = [row_len(ROWS, g) for g in WIDE]
  # an even total: the four outputs are 16-B aligned and rows start at even and odd offsets (both halves of a pair)
  flat = collate('bert', law, p).collate_rows_unpadded(res, WIDE)
  cu = host(flat['cu_seqlens'])
  assert cu[-1] % 2 == 0 and {int(x) % 2 for x in cu[:-1]} == {0, 1}
  check_stream(flat, pad, keep, lens)
  # an odd total (without the last two rows): lane = token
  odd = collate('bert', law, p).collate_rows_unpadded(res, WIDE[:-2])
  assert int(odd['cu_seqlens'][-1]) % 2 == 1
  keep1 = keep.copy()
  keep1[-2:] = False
  check_stream(odd, pad, keep1, lens[:-2])
  # fixed shapes: the real tokens first, then pad sequences that nothing selects
  T = int(cu[-1])
  fx = collate('bert', law, p).collate_rows_fixed(res, WIDE, max_tokens=T + 700, max_seqs=len(WIDE) + 3, max_seqlen=512)
  assert fx['num_tokens'] == T and fx['num_rows'] == len(WIDE) and fx['num_seqs'] == len(WIDE) + 2
  for k in ('input_ids', 'labels', 'token_type_ids', 'position_ids'):
    assert torch.equal(fx[k][:T], flat[k]), k
  assert bool((fx['labels'][T:] == IGNORE).all()) and not bool(fx['input_ids'][T:].any())
  assert torch.equal(fx['cu_seqlens'][:len(WIDE) + 1], flat['cu_seqlens'])
  # mask_tokens over the unmasked batch
  col = collate('bert', law, p)
  raw = col.collate_rows(res, WIDE, mode=0)
  x, lab = col.mask_tokens(raw['input_ids'].clone(), raw['special_tokens_mask'], counter=COUNTER)
  assert torch.equal(x, pad['input_ids']) and torch.equal(lab, pad['labels'])


@pytest.mark.parametrize('law,p', [(LAWS[0], 0.5), (LAWS[1], 0.15)])
def test_unpadded_narrow_path_at_an_even_total(gpu, law, p):
  """lddl_collate_rows_unpadded itself into outputs one element off a 16-B boundary: lane = token, rows at even and
  odd offsets"""
  res = table()
  dev = res.len0.device
  col = collate('bert', law, p)
  pad = col.collate_rows(res, WIDE)
  flat = collate('bert', law, p).collate_rows_unpadded(res, WIDE)
  T, n = int(flat['cu_seqlens'][-1]), len(WIDE)
  whole = torch.full((4, T + 3), -7, dtype=torch.int64, device=dev)
  assert whole.data_ptr() % 16 == 0 and (T + 3) % 2 == 1
  outs = [whole[0, 1:T + 1], whole[1, 2:T + 2], whole[2, 1:T + 1], whole[3, 2:T + 2]]
  assert all(o.data_ptr() % 16 == 8 for o in outs)
  nsl = torch.empty(n, dtype=torch.int64, device=dev)
  P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
  rows = torch.as_tensor(WIDE, dtype=torch.int64, device=dev)
  rc = _lib.lib().lddl_collate_rows_unpadded(
      tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, n,
      res.n_pairs, None, None, None, None, P(flat['cu_seqlens']), T, 2, IGNORE, p, SEED, COUNTER, P(outs[0]), P(outs[1]),
      P(outs[2]), P(outs[3]), P(nsl), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == 0, _lib.lib().lddl_last_error()
  for o, k in zip(outs, ('input_ids', 'token_type_ids', 'position_ids', 'labels')):
    assert torch.equal(o, flat[k]), k
  assert int((whole == -7).sum()) == 4 * 3
  assert pad['labels'].ne(IGNORE).any()


@pytest.mark.parametrize('law,p', [(LAWS[0], 0.15), (LAWS[1], 0.5)])
def test_string_route(gpu, law, p):
  """the same rows rendered into a small Arrow table: BertCollate.__call__ / collate_arrow == collate_rows"""
  import pyarrow as pa
  idx = [12, 0, 1, 13, 14, 16, 9, 17]
  names = tok().ids_to_tokens
  text = lambda ids: ' '.join(names[i] for i in ids)  # noqa: E731
  t = pa.table({'A': [text(ROWS[g][0]) for g in idx], 'B': [text(ROWS[g][1]) for g in idx],
                'is_random_next': [bool(ROWS[g][3]) for g in idx]})
  out = collate('bert', law, p)(t)
  check_padded(out, idx, 512, p, law)
  rows = collate('bert', law, p).collate_rows(table(), idx)
  assert all(torch.equal(out[k], rows[k]) for k in out)
  samples = [(text(ROWS[g][0]), text(ROWS[g][1]), bool(ROWS[g][3])) for g in idx[:-1]]
  out = collate('bert', law, p, align=1)(samples)
  check_padded(out, idx[:-1], 138, p, law)


@pytest.mark.parametrize('law,p', [(LAWS[0], 0.5), (LAWS[1], 0.15)])
@pytest.mark.parametrize('kind', ['code', 'mlm'])
def test_code_and_mlm_rows(gpu, kind, law, p):
  res = table()
  idx = CODE_ROWS if kind == 'code' else MLM_ROWS
  lens = [row_len(ROWS, g) for g in idx]
  for align in (8, 1):
    S = max(lens) if align == 1 else (max(lens) + 7) // 8 * 8
    assert S % 2 == (1 if align == 1 else 0)
    pad = collate(kind, law, p, align=align).collate_rows(res, idx)
    m, keep = check_padded(pad, idx, S, p, law, nsl=False)
    assert m.select.any()
    # all rows: an odd total, lane = token; without the last: an even one, pairs at even and odd offsets
    flat = collate(kind, law, p, align=align).collate_rows_unpadded(res, idx)
    assert int(flat['cu_seqlens'][-1]) % 2 == 1
    check_stream(flat, pad, keep, lens)
    flat = collate(kind, law, p, align=align).collate_rows_unpadded(res, idx[:-1])
    cu = host(flat['cu_seqlens'])
    assert cu[-1] % 2 == 0 and {int(x) % 2 for x in cu[:-1]} == {0, 1}
    keep[-1] = False
    check_stream(flat, pad, keep, lens[:-1])
    T = int(cu[-1])
    fx = collate(kind, law, p).collate_rows_fixed(res, idx[:-1], max_tokens=T + 9, max_seqs=len(idx), max_seqlen=S)
    assert torch.equal(fx['input_ids'][:T], flat['input_ids']) and torch.equal(fx['labels'][:T], flat['labels'])
    assert bool((fx['labels'][T:] == IGNORE).all())


def mask_case(n, S, seed, lo=-6, hi=V + 6, cont=(31, 57)):
  """ids in [lo, hi) with many '##' ids, and a special mask that falls inside words, in mid-row and at column 0"""
  rng = np.random.default_rng(seed)
  ids = np.where(rng.random((n, S)) < 0.5, rng.integers(*cont, (n, S)), rng.integers(lo, hi, (n, S))).astype(np.int64)
  sp = (rng.random((n, S)) < 0.08).astype(np.int64)
  sp[0, 0], sp[n - 1, 0] = 1, 0
  ids[n - 1, 0] = cont[0]  # a '##' id at column 0 heads a word
  return ids, sp


def run_mask_tokens(col, ids, sp, counter=COUNTER):
  x = torch.from_numpy(ids.copy()).cuda()
  out, lab = col.mask_tokens(x, torch.from_numpy(sp).cuda(), counter=counter)
  assert out is x
  return host(out), host(lab)


@pytest.mark.parametrize('law,p', [(LAWS[0], 0.15), (LAWS[1], 0.5)])
@pytest.mark.parametrize('S', [1, 64, 65, 2048])
def test_mask_tokens(gpu, S, law, p):
  ids, sp = mask_case(3 if S == 2048 else 9, S, S)
  assert ((ids >= V) | (ids < 0)).any() or S == 1
  got, lab = run_mask_tokens(collate('bert', law, p), ids, sp)
  m = sm.mask(ids, sp, cont_table(), SEED, COUNTER, p, law[0], law[1], MASK, V, IGNORE)
  assert np.array_equal(lab, m.labels) and np.array_equal(got, m.input_ids)
  assert S == 1 or (m.select.any() and (lab[sp != 0] == IGNORE).all())


def test_mask_tokens_more_rows_than_one_pass_of_the_grid(gpu):
  n = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
  ids, sp = mask_case(n, 8, 77)
  x = torch.from_numpy(ids.copy()).cuda()
  _, full = collate('bert', LAWS[1], 0.5).mask_tokens(x, torch.from_numpy(sp).cuda(), counter=COUNTER)
  m = sm.mask(ids[-40:], sp[-40:], cont_table(), SEED, COUNTER, 0.5, 3, 0.5, MASK, V, IGNORE, rows=np.arange(n - 40, n))
  # (the model's share: the last rows)
  assert np.array_equal(host(full)[-40:], m.labels) and np.array_equal(host(x)[-40:], m.input_ids)
  assert m.select[-5:].any()


def test_bert_vocabulary(gpu):
  """rows of random ids of the bundled vocabulary, a third of them '##' entries"""
  t = tok('bert')
  table_ = cont_table('bert')
  cont_ids, other = np.flatnonzero(table_), np.flatnonzero(~table_)
  other = other[other > 999]
  rng = np.random.default_rng(5)

  def seg(k):
    return [int(rng.choice(cont_ids) if rng.random() < 0.35 else rng.choice(other)) for _ in range(k)]
  rows = [(seg(a), seg(b), 1, 0) for a, b in ((20, 17), (80, 46), (200, 100), (1, 1), (125, 0))]
  res = make_table(rows, t.cls_id, t.sep_id)
  idx = list(range(len(rows)))
  col = collate('bert', True, 0.15, vocab='bert')  # True: max_span 10, geo_p 0.2
  assert col.span_mask == (10, 0.2)
  pad = col.collate_rows(res, idx)
  ids, sp, tt, am = planes(idx, 304, rows, t.cls_id, t.sep_id)
  m = sm.mask(ids, sp, table_, SEED, COUNTER, 0.15, 10, 0.2, t.mask_id, t.vocab_size, IGNORE)
  assert np.array_equal(host(pad['labels']), m.labels) and np.array_equal(host(pad['input_ids']), m.input_ids)
  assert m.random.any() and m.masked.any()
  flat = collate('bert', True, 0.15, vocab='bert').collate_rows_unpadded(res, idx)
  check_stream(flat, pad, am != 0, [row_len(rows, g) for g in idx])
  collate('bert', None, vocab='bert')  # (the shared ctx: off again)


def test_vocabulary_without_continuations(gpu):
  """'tiny6' holds the special tokens and 'a': every token is a word, spans are runs of tokens"""
  t = tok('tiny6')
  assert not cont_table('tiny6').any()
  rows = [([5] * 70, [5] * 60, 1, 0), ([5] * 3, [5], 1, 1)]
  res = make_table(rows, t.cls_id, t.sep_id)
  for law, p in ((LAWS[0], 0.15), (LAWS[1], 0.5)):
    pad = collate('bert', law, p, vocab='tiny6').collate_rows(res, [0, 1])
    ids, sp, _, _ = planes([0, 1], 136, rows, t.cls_id, t.sep_id)
    m = sm.mask(ids, sp, None, SEED, COUNTER, p, law[0], law[1], t.mask_id, 6, IGNORE)
    assert np.array_equal(host(pad['labels']), m.labels) and np.array_equal(host(pad['input_ids']), m.input_ids)
    x, spm = mask_case(3, 70, 1, lo=-2, hi=9, cont=(5, 6))
    got, lab = run_mask_tokens(collate('bert', law, p, vocab='tiny6'), x, spm)
    m = sm.mask(x, spm, None, SEED, COUNTER, p, law[0], law[1], t.mask_id, 6, IGNORE)
    assert np.array_equal(got, m.input_ids) and np.array_equal(lab, m.labels) and (m.select & ~m.open).any()


# ---- the switch -------------------------------------------------------------------
def batch_of(col, idx=WIDE):
  col.counter = COUNTER
  a = col.collate_rows(table(), idx)
  col.counter = COUNTER
  b = col.collate_rows_unpadded(table(), idx)
  return [a['input_ids'], a['labels'], b['input_ids'], b['labels']]


def test_max_span_1_is_whole_word_masking(gpu):
  word_ = batch_of(collate('bert', None, 0.15, whole_word_mask=True))
  for g in (0.2, 1.0):
    one = batch_of(collate('bert', (1, g), 0.15))
    assert all(torch.equal(x, y) for x, y in zip(one, word_))
  ids, sp, _, _ = planes(WIDE, 512)
  m = wm.mask(ids, sp, cont_table(), SEED, COUNTER, 0.15, MASK, V, IGNORE)
  assert np.array_equal(host(word_[1]), m.labels) and np.array_equal(host(word_[0]), m.input_ids)
  x, spm = mask_case(5, 130, 3)
  a = run_mask_tokens(collate('bert', {'max_span': 1, 'geo_p': 0.5}, 0.15), x, spm)
  b = run_mask_tokens(collate('bert', None, 0.15, whole_word_mask=True), x, spm)
  assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
  collate('bert', None)


def test_switching_off_restores_token_and_whole_word_output(gpu):
  token = batch_of(collate('bert', None, 0.15))
  word_ = batch_of(collate('bert', None, 0.15, whole_word_mask=True))
  span = batch_of(collate('bert', LAWS[0], 0.15))
  assert not torch.equal(span[1], token[1]) and not torch.equal(span[1], word_[1])
  # the whole-word switch is ignored while span masking is on
  h, L = tok().handle, _lib.lib()
  col = collate('bert', LAWS[0], 0.15)
  assert L.lddl_set_whole_word_mask(h, 1) == 0
  assert all(torch.equal(x, y) for x, y in zip(batch_of(col), span))
  # off: whole-word output (that switch is still on), then token output, on the same ctx
  assert L.lddl_set_span_mask(h, 0, 0.0) == 0
  assert all(torch.equal(x, y) for x, y in zip(batch_of(col), word_))
  assert L.lddl_set_whole_word_mask(h, 0) == 0
  assert all(torch.equal(x, y) for x, y in zip(batch_of(col), token))
  ids, sp, _, _ = planes(WIDE, 512)
  m = mm.mask(ids, sp, SEED, COUNTER, 0.15, MASK, V, IGNORE)
  assert np.array_equal(host(token[1]), m.labels) and np.array_equal(host(token[0]), m.input_ids)
  # a collate constructed without span_mask switches a shared ctx off
  collate('bert', LAWS[1], 0.15)
  assert all(torch.equal(x, y) for x, y in zip(batch_of(collate('bert', None, 0.15)), token))


@pytest.mark.parametrize('mode', [0, 1])
def test_modes_0_and_1_ignore_the_switch(gpu, mode):
  res, n = make_table(ROWS, CLS, SEP), len(ROWS)  # its own table, with one static mask per row
  t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).cuda()  # noqa: E731
  res.n_masked, res.mlm_off = n, t(np.arange(n + 1), np.int64)
  res.mlm_pos, res.mlm_label, res.mlm_token = t([1] * n, np.int16), t([30] * n, np.int16), t([MASK] * n, np.int16)
  outs = []
  for span in (None, LAWS[0]):
    col = collate('bert', span)
    a = col.collate_rows(res, WIDE, mode=mode)
    b = col.collate_rows_unpadded(res, WIDE, mode=mode)
    outs.append([a[k] for k in sorted(a)] + [b[k] for k in sorted(b) if k != 'max_seqlen'])
    if mode == 0:
      outs[-1] += list(collate('code', span).collate_rows(res, CODE_ROWS, mode=0).values())
  assert len(outs[0]) == len(outs[1]) and all(torch.equal(x, y) for x, y in zip(*outs))
  collate('bert', None)


def test_compact_mlm_lists_the_selected_positions(gpu):
  law, p = LAWS[1], 0.5
  out = collate('bert', law, p, compact_mlm=True).collate_rows(table(), WIDE)
  m, _ = expect(tuple(WIDE), 512, p, law)
  assert np.array_equal(host(out['masked_lm_positions']), np.flatnonzero(m.select.reshape(-1)))
  assert np.array_equal(host(out['masked_lm_labels']), m.labels.reshape(-1)[m.select.reshape(-1)])
  assert np.array_equal(host(out['masked_lm_offsets']), np.concatenate([[0], np.cumsum(m.select.sum(1))]))
  collate('bert', None)


def test_arguments(gpu):
  from lddl_amd.loader import BertCollate, CodeCollate, MlmCollate
  for cls in (BertCollate, CodeCollate, MlmCollate):
    with pytest.raises(ValueError, match='whole_word_mask'):
      cls(tokenizer=tok(), span_mask=True, whole_word_mask=True)
    for bad in ((17, 0.2), (10, 0.0), (0, 0.2), (10, 1.5), 'x', {'max_span': 3, 'p': 1}, (2.5, 0.2)):
      with pytest.raises(ValueError, match='span_mask'):
        cls(tokenizer=tok(), span_mask=bad)
  assert BertCollate(tokenizer=tok(), span_mask=False).span_mask is None
  assert BertCollate(tokenizer=tok(), span_mask={'max_span': 4}).span_mask == (4, 0.2)
  # the C call: a refused setting leaves the switch as it was, on or off
  h, L = tok().handle, _lib.lib()
  col = collate('bert', LAWS[1], 0.5)
  span = batch_of(col)
  for bad in ((17, 0.2), (10, 0.0), (-1, 0.2), (10, float('nan'))):
    assert L.lddl_set_span_mask(h, *bad) == EINVAL and L.lddl_last_error()
  assert all(torch.equal(x, y) for x, y in zip(batch_of(col), span))
  col = collate('bert', None, 0.5)
  token = batch_of(col)
  assert not torch.equal(token[1], span[1])
  for bad in ((17, 0.2), (10, 0.0), (-1, 0.2)):
    assert L.lddl_set_span_mask(h, *bad) == EINVAL
  assert all(torch.equal(x, y) for x, y in zip(batch_of(col), token))
  assert L.lddl_set_span_mask(None, 3, 0.5) == EINVAL and L.lddl_last_error() == b'null ctx'
