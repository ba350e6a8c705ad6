"""Whole-word dynamic masking (lddl_set_whole_word_mask) on every route that
masks dynamically, bit for bit against tests/wwm_model.py: mode 2 of
collate_rows and collate_rows_unpadded (BERT and CodeBERT rows, the wide and
the narrow path of each), of the string route, and mask_tokens.

The rows are hand-made row tables (as tests/test_capi_first_call_gpu.py builds
its own) over the 'tiny64' vocabulary of tests/synth_vocab.py: ids 5..30 are
the letters, 31..56 their '##' forms, 63 is '##ing'; [CLS] 2, [SEP] 3,
[MASK] 4, 64 entries.
"""
import functools

import numpy as np
import pytest
import torch

import mask_model as mm
import synth_vocab as sv
import wwm_model as wm
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

VOCAB, V, CLS, SEP, MASK, IGNORE = 'tiny64', 64, 2, 3, 4, -1
DRAWS = [(31, 9), ((1 << 63) + 12345, 1 << 40)]  # (seed, counter)
PS = [0.0, 0.15, 1.0]


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


# (A / doc, B / code, s, is_random_next).  Columns: [CLS] 0, A 1 .. a, [SEP] a + 1, B from a + 2.
ROWS = [
    # 0: words over columns 62..65 and 126..129: across 63/64 and 127/128
    (plain(61) + word(4, 3) + plain(60, 7) + word(4, 11) + plain(3), word(2, 5) + plain(1), 1, 0),
    # 1: a word of 130 pieces from column 60 to 189: the carry runs through the step of columns 64..127
    (plain(59, 2) + word(130, 9) + plain(2), pieces(2, 4) + plain(1), 1, 1),
    # 2: one word of 509 pieces, 512 tokens
    (word(509, 1), [], 1, 0),
    # 3: the same with a B: 513 tokens
    (word(509, 6), plain(1), 1, 1),
    # 4: A's last word ends at [SEP], B begins with '##' pieces
    (plain(1) + word(3, 8), pieces(2, 12) + word(2, 1), 1, 0),
    # 5: no continuation at all
    (plain(5, 3), plain(4, 9), 1, 1),
    # 6: no continuation, odd length
    (plain(2, 1), plain(2, 5), 1, 0),
    # 7: CodeBERT with docstring, the code begins with '##' pieces
    (word(3, 2) + plain(1), pieces(3, 7) + word(2, 4), 1, 0),
    # 8: CodeBERT without docstring ([CLS] code [SEP]), the code begins with '##' pieces and holds a word of 70
    ([], pieces(2, 3) + plain(1) + word(70, 5) + [63, 63], 0, 0),
    # 9: CodeBERT without docstring, no continuation
    ([], plain(6, 4), 0, 0),
]
WIDE = [0, 1, 2, 4, 5]       # with alignment 8: seq_len 512, even
NARROW = [4, 3, 0, 1, 6]     # with alignment 1: seq_len 513, odd
NO_CONT = [5, 6, 5]
CODE_ROWS = [7, 8, 9, 0, 8, 1]


def row_len(g):
  a, b, s, _ = ROWS[g]
  return len(a) + len(b) + 2 + s


@functools.lru_cache(maxsize=None)
def tok():
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer(sv.vocab_path(VOCAB), 0)
  assert t.vocab_size == V and (t.cls_id, t.sep_id, t.mask_id) == (CLS, SEP, MASK)
  return t


@functools.lru_cache(maxsize=None)
def cont_table():
  t = wm.cont_table(tok().ids_to_tokens)
  assert np.flatnonzero(t).tolist() == list(range(31, 57)) + [63]  # what synth_vocab's tiny64 holds
  return t


@functools.lru_cache(maxsize=None)
def table(static=False):
  """ROWS as a PackResult with spans; static: with one static mask per row (the collates then default to mode 1)"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  n = len(ROWS)
  ids, src0, src1 = [0], [], []  # (an id in front: no span starts at 0)
  for a, b, _, _ in ROWS:
    src0.append(len(ids))
    ids += a
    src1.append(len(ids))
    ids += b
  lens = np.asarray([row_len(g) for g in range(n)], np.int64)

  def t(a, dt):
    a = np.ascontiguousarray(np.asarray(a, dt))
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t([len(r[0]) for r in ROWS], np.uint16), t([len(r[1]) for r in ROWS], np.uint16),
      t([r[2] * 2 + r[3] for r in ROWS], np.uint8), t(np.zeros(n), np.uint8), t(np.zeros(n), np.int64),
      t([[n]], np.int64))
  res.ids, res.src0, res.src1 = t(ids + [0] * 16, np.uint16), t(src0, np.int64), t(src1, np.int64)
  res.cls_id, res.sep_id = CLS, SEP
  if static:
    res.n_masked, res.mlm_off = n, t(np.arange(n + 1), np.int64)
    res.mlm_pos, res.mlm_label, res.mlm_token = t([1] * n, np.uint16), t([30] * n, np.uint16), t([MASK] * n, np.uint16)
  return res


def planes(idx, S):
  """the unmasked batch: ids, special (the special tokens and the padding), token_type_ids, attention_mask"""
  n = len(idx)
  ids, sp, tt, am = (np.zeros((n, S), np.int64) for _ in range(4))
  sp[:] = 1
  for r, g in enumerate(idx):
    a, b, s, _ = ROWS[g]
    row = [CLS] + a + [SEP] * s + b + [SEP]
    ids[r, :len(row)] = row
    am[r, :len(row)] = 1
    sp[r, 1:1 + len(a)] = 0
    sp[r, 1 + len(a) + s:len(row) - 1] = 0
    if s:
      tt[r, len(a) + 2:len(row)] = 1
  return ids, sp, tt, am


def collate(kind, on, p=0.15, seed=31, counter=9, align=8):
  from lddl_amd.loader import BertCollate, CodeCollate
  col = (CodeCollate if kind == 'code' else BertCollate)(tokenizer=tok(), sequence_length_alignment=align,
                                                        base_seed=seed, mlm_probability=p, whole_word_mask=on)
  col.counter = counter
  return col


def expect(idx, S, p, seed, counter):
  ids, sp, tt, am = planes(idx, S)
  return wm.mask(ids, sp, cont_table(), seed, counter, p, MASK, V, IGNORE), (ids, sp, tt, am)


def host(t):
  return t.cpu().numpy()


def check_padded(out, idx, S, p, seed, counter, nsl=True):
  m, (ids, sp, tt, am) = expect(idx, S, p, seed, counter)
  assert tuple(out['input_ids'].shape) == (len(idx), S)
  assert np.array_equal(host(out['labels']), m.labels)
  assert np.array_equal(host(out['input_ids']), m.input_ids)
  assert np.array_equal(host(out['token_type_ids']), tt) and np.array_equal(host(out['attention_mask']), am)
  if nsl:
    assert host(out['next_sentence_labels']).tolist() == [ROWS[g][3] for g in idx]
  if p == 1.0:
    assert np.array_equal(host(out['labels'])[sp == 0], ids[sp == 0])
  return m


@pytest.mark.parametrize('seed,counter', DRAWS)
@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('path', ['wide', 'narrow'])
def test_collate_rows(gpu, path, p, seed, counter):
  idx, align, S = (WIDE, 8, 512) if path == 'wide' else (NARROW, 1, 513)
  out = collate('bert', True, p, seed, counter, align).collate_rows(table(), idx)
  m = check_padded(out, idx, S, p, seed, counter)
  if p == 0.15 and (seed, counter) == DRAWS[0]:
    # this draw selects words of several pieces: whole words, and not the per-token output
    h = wm.heads(*planes(idx, S)[:2], cont_table())
    assert (m.select & (h != np.arange(S)[None, :])).any()
    off = collate('bert', False, p, seed, counter, align).collate_rows(table(), idx)
    assert not np.array_equal(host(off['labels']), m.labels)


@pytest.mark.parametrize('seed,counter', DRAWS)
@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('idx', [[1, 4, 0, 2, 3, 6, 5], [4, 1, 0, 3, 5]], ids=['even_total', 'odd_total'])
def test_collate_rows_unpadded(gpu, idx, p, seed, counter):
  """an even total keeps the four outputs 16-B aligned (the pair path), an odd
  one does not (lane = token); rows start at even and at odd stream offsets"""
  res = table()
  out = collate('bert', True, p, seed, counter).collate_rows_unpadded(res, idx)
  off = collate('bert', False, p, seed, counter).collate_rows_unpadded(res, idx)
  cu = host(out['cu_seqlens']).astype(np.int64)
  T = int(cu[-1])
  assert T % 2 == (0 if len(idx) == 7 else 1)
  assert {int(x) % 2 for x in cu[:-1]} == {0, 1}
  assert np.array_equal(np.diff(cu), [row_len(g) for g in idx])
  S = int(np.diff(cu).max())
  m, (ids, sp, tt, am) = expect(idx, S, p, seed, counter)
  keep = am != 0
  assert np.array_equal(host(out['labels']), m.labels[keep])
  assert np.array_equal(host(out['input_ids']), m.input_ids[keep])
  for k in ('cu_seqlens', 'token_type_ids', 'position_ids', 'next_sentence_labels'):
    assert torch.equal(out[k], off[k]), k
  assert out['max_seqlen'] == off['max_seqlen'] == S
  unmasked = host(out['labels']) == IGNORE
  assert np.array_equal(host(out['input_ids'])[unmasked], ids[keep][unmasked])
  # the padded batch of the same rows, with its padding dropped
  pad = collate('bert', True, p, seed, counter, align=1).collate_rows(res, idx)
  assert np.array_equal(host(pad['input_ids'])[keep], host(out['input_ids']))
  assert np.array_equal(host(pad['labels'])[keep], host(out['labels']))


@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('align', [8, 1])
def test_code_rows(gpu, align, p):
  seed, counter = DRAWS[0]
  res, idx = table(), CODE_ROWS
  S = max(row_len(g) for g in idx)  # 197: odd
  S = S if align == 1 else (S + 7) // 8 * 8
  out = collate('code', True, p, seed, counter, align).collate_rows(res, idx)
  check_padded(out, idx, S, p, seed, counter, nsl=False)
  # all six rows: an odd total, the lane = token path
  flat = collate('code', True, p, seed, counter, align).collate_rows_unpadded(res, idx)
  assert int(flat['cu_seqlens'][-1]) % 2 == 1
  keep = planes(idx, S)[3] != 0
  assert np.array_equal(host(flat['input_ids']), host(out['input_ids'])[keep])
  assert np.array_equal(host(flat['labels']), host(out['labels'])[keep])
  # the first five: an even total, the pair path, rows at even and odd offsets
  flat = collate('code', True, p, seed, counter, align).collate_rows_unpadded(res, idx[:5])
  cu = host(flat['cu_seqlens'])
  assert cu[-1] % 2 == 0 and {int(x) % 2 for x in cu[:-1]} == {0, 1}
  keep[5:] = False
  assert np.array_equal(host(flat['input_ids']), host(out['input_ids'])[keep])
  assert np.array_equal(host(flat['labels']), host(out['labels'])[keep])


@pytest.mark.parametrize('p', PS)
def test_string_route(gpu, p):
  """the same rows rendered into a small Arrow table: BertCollate.__call__ / collate_arrow"""
  import pyarrow as pa
  seed, counter = DRAWS[1]
  idx = [4, 0, 1, 5, 2]
  names = tok().ids_to_tokens
  text = lambda ids: ' '.join(names[i] for i in ids)  # noqa: E731
  t = pa.table({'A': [text(ROWS[g][0]) for g in idx], 'B': [text(ROWS[g][1]) for g in idx],
                'is_random_next': [bool(ROWS[g][3]) for g in idx]})
  out = collate('bert', True, p, seed, counter)(t)
  check_padded(out, idx, 512, p, seed, counter)
  samples = [(text(ROWS[g][0]), text(ROWS[g][1]), bool(ROWS[g][3])) for g in idx]
  out = collate('bert', True, p, seed, counter, align=1)(samples)
  check_padded(out, idx, 512, p, seed, counter)


def mask_case(n, S, seed):
  """ids in [-6, V + 6) with many '##' ids, and a special mask that falls inside words"""
  rng = np.random.default_rng(seed)
  ids = np.where(rng.random((n, S)) < 0.6, rng.integers(31, 57, (n, S)), rng.integers(-6, V + 6, (n, S))).astype(np.int64)
  sp = (rng.random((n, S)) < 0.1).astype(np.int64)
  return ids, sp


def run_mask_tokens(col, ids, sp, counter):
  x = torch.from_numpy(ids.copy()).cuda()
  out, lab = col.mask_tokens(x, torch.from_numpy(sp).cuda(), counter=counter)
  assert out is x
  return host(out), host(lab)


@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('S', [1, 64, 65, 130])
def test_mask_tokens(gpu, S, p):
  seed, counter = DRAWS[S % 2]
  ids, sp = mask_case(9, S, S)
  ids[0, 0], sp[0, 0] = 40, 0  # a '##' id at column 0 heads a word
  assert (ids >= V).any() or S == 1
  got, lab = run_mask_tokens(collate('bert', True, p, seed), ids, sp, counter)
  m = wm.mask(ids, sp, cont_table(), seed, counter, p, MASK, V, IGNORE)
  assert np.array_equal(lab, m.labels) and np.array_equal(got, m.input_ids)
  if p == 1.0:
    assert np.array_equal(lab[sp == 0], ids[sp == 0])


def test_mask_tokens_more_rows_than_one_pass_of_the_grid(gpu):
  seed, counter = DRAWS[0]
  n = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
  ids, sp = mask_case(n, 8, 77)
  got, lab = run_mask_tokens(collate('bert', True, 0.15, seed), ids, sp, counter)
  m = wm.mask(ids, sp, cont_table(), seed, counter, 0.15, MASK, V, IGNORE)
  assert np.array_equal(lab, m.labels) and np.array_equal(got, m.input_ids)
  assert m.select[-5:].any()


def test_rows_without_continuations_and_switching_off_again(gpu):
  seed, counter = DRAWS[0]
  res = table()

  def run(col, idx):
    col.counter = counter
    a = col.collate_rows(res, idx)
    col.counter = counter
    b = col.collate_rows_unpadded(res, idx)
    return [a[k] for k in ('input_ids', 'labels')] + [b[k] for k in ('input_ids', 'labels')]
  on = run(collate('bert', True, 0.15, seed, counter), NO_CONT)
  off = run(collate('bert', False, 0.15, seed, counter), NO_CONT)  # (switches the shared ctx off again)
  assert all(torch.equal(x, y) for x, y in zip(on, off))
  ids, sp, _, _ = planes(NO_CONT, 16)
  assert np.array_equal(host(off[1]), mm.mask(ids, sp, seed, counter, 0.15, MASK, V, IGNORE).labels)
  # with continuations: on differs, and off after on is the per-token output of tests/mask_model.py
  before = run(collate('bert', False, 0.15, seed, counter), WIDE)
  on = run(collate('bert', True, 0.15, seed, counter), WIDE)
  after = run(collate('bert', False, 0.15, seed, counter), WIDE)
  assert all(torch.equal(x, y) for x, y in zip(before, after))
  assert not torch.equal(on[1], after[1])
  ids, sp, _, _ = planes(WIDE, 512)
  m = mm.mask(ids, sp, seed, counter, 0.15, MASK, V, IGNORE)
  assert np.array_equal(host(after[0]), m.input_ids) and np.array_equal(host(after[1]), m.labels)
  x, spm = mask_case(5, 130, 3)
  got, lab = run_mask_tokens(collate('bert', False, 0.15, seed), x, spm, counter)
  m = mm.mask(x, spm, seed, counter, 0.15, MASK, V, IGNORE)
  assert np.array_equal(got, m.input_ids) and np.array_equal(lab, m.labels)


@pytest.mark.parametrize('mode', [0, 1])
def test_modes_0_and_1_ignore_the_switch(gpu, mode):
  res = table(static=True)
  outs = []
  for on in (False, True):
    col = collate('bert', on)
    a = col.collate_rows(res, WIDE, mode=mode)
    b = col.collate_rows_unpadded(res, WIDE, mode=mode)
    outs.append([a[k] for k in sorted(a)] + [b[k] for k in sorted(b) if k != 'max_seqlen'])
  assert all(torch.equal(x, y) for x, y in zip(*outs))
  if mode == 0:
    names = tok().ids_to_tokens
    samples = [(' '.join(names[i] for i in ROWS[g][0]), ' '.join(names[i] for i in ROWS[g][1]), False) for g in (4, 5)]
    a, b = (collate('bert', on).to_encoded_inputs(samples) for on in (False, True))
    assert all(torch.equal(a[k], b[k]) for k in a)
    c0, c1 = (collate('code', on).collate_rows(res, CODE_ROWS, mode=0) for on in (False, True))
    assert all(torch.equal(c0[k], c1[k]) for k in c0)


def test_null_ctx_is_refused(gpu):
  L = _lib.lib()
  assert L.lddl_set_whole_word_mask(None, 1) == -1  # LDDL_EINVAL
  assert L.lddl_last_error() == b'null ctx'
  assert L.lddl_set_whole_word_mask(None, 0) == -1


def test_vocabulary_without_continuations_is_accepted(gpu):
  """'tiny5' holds the five special tokens only: the switch is accepted and changes nothing"""
  from lddl_amd.loader import BertCollate
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer(sv.vocab_path('tiny5'), 0)
  assert _lib.lib().lddl_set_whole_word_mask(t.handle, 1) == 0
  ids = np.random.default_rng(1).integers(-2, 9, (3, 70)).astype(np.int64)
  sp = np.zeros_like(ids)
  outs = []
  for on in (True, False):
    col = BertCollate(tokenizer=t, base_seed=5, whole_word_mask=on)
    outs.append(run_mask_tokens(col, ids, sp, 2))
  assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
  m = mm.mask(ids, sp, 5, 2, 0.15, t.mask_id, 5, -1)
  assert np.array_equal(outs[0][0], m.input_ids) and np.array_equal(outs[0][1], m.labels)
