"""Exact-count dynamic masking (lddl_set_mask_budget) on every dynamic route,
bit for bit against tests/budget_model.py, tokens and whole words.

Hand-made rows over 'tiny64' of tests/synth_vocab.py (ids 5..30 letters, 31..56
their '##' forms).  Rows of 5 .. 2048 tokens: one step, the edges of the 64-
and 128-column steps, the longest row.  BERT: ten rows (a block takes four),
an odd total: the padding-free batch takes lane = token, the fixed batch (even
max_tokens) the pair path with rows at odd offsets.  Rows 3 and 6 hold a
segment that is one word; row 9 is a CodeBERT row without docstring, and the
longest of CODE, padded at alignment 1: an odd width, collate_rows' 8-B stores.
"""
import functools

import numpy as np
import pytest
import torch

import budget_cases as bc
import budget_model as bm
import synth_vocab as sv
import wwm_model as wm

pytestmark = pytest.mark.gpu

V, MASK, IGNORE, SEED, COUNTER = bc.V, bc.MASK, bc.IGNORE, bc.S63, bc.C40
ROWS = bc.ROWS  # (tokens, s, '##' density; 'word': segment 0 is one word): made in tests/budget_cases.py, without a GPU
BERT, CODE = [7, 3, 0, 5, 1, 2, 8, 4, 6, 10], [9, 3, 0, 5, 2, 8]
FIXED = dict(max_tokens=3100, max_seqs=12, max_seqlen=2048)


def host(t):
  return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def tokenizer():
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(sv.vocab_path('tiny64'), 0)


def table(tok, segs, sep, kind='bert'):
  """rows of two segments' ids each (sep: a [SEP] follows segment 0) as a PackResult with spans"""
  from lddl_amd import pipeline
  ids, src, lens = [0], ([], []), ([], [])
  for seg in segs:
    for k in (0, 1):
      src[k].append(len(ids))
      lens[k].append(len(seg[k]))
      ids += seg[k]
  n, ntok = len(segs), np.asarray([len(a) + len(b) + 2 + s for (a, b), s in zip(segs, sep)], np.int64)

  def t(a, dt):
    a = np.ascontiguousarray(np.asarray(a, dt))
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
  res = pipeline.PackResult(n, int(ntok.sum()), 1, None, t(np.concatenate([[0], np.cumsum(ntok)]), np.int64),
                            t(lens[0], np.uint16), t(lens[1], np.uint16), t([s * 2 for s in sep], np.uint8),
                            t(np.zeros(n), np.uint8), t(np.zeros(n), np.int64), t([[n]], np.int64))
  res.ids, res.src0, res.src1 = t(ids + [0] * 16, np.uint16), t(src[0], np.int64), t(src[1], np.int64)
  res.cls_id, res.sep_id, res.kind = tok.cls_id, tok.sep_id, kind
  return res


@functools.lru_cache(maxsize=None)
def world():
  """tokenizer, the rows as a PackResult with spans, their (A, B) ids, the '##' table"""
  tok, segs = tokenizer(), bc.segments()
  res = table(tok, segs, [r[1] for r in ROWS])
  assert res.n_tokens == sum(r[0] for r in ROWS) and np.array_equal(wm.cont_table(tok.ids_to_tokens), bc.cont())
  return tok, res, segs, wm.cont_table(tok.ids_to_tokens)


def collate(code, wwm, P, p, seed=SEED, counter=COUNTER, cls=None, tok=None, **kw):
  from lddl_amd.loader import BertCollate, CodeCollate
  col = (cls or (CodeCollate if code else BertCollate))(
      tokenizer=tok or world()[0], base_seed=seed, mlm_probability=p, whole_word_mask=wwm, max_predictions=P,
      sequence_length_alignment=1 if code else 8, **kw)
  col.counter = counter
  return col


def model(ids, sp, wwm, P, p, seed=SEED, counter=COUNTER):
  m = bm.mask(ids, sp, world()[3] if wwm else None, seed, counter, p, P, MASK, V, IGNORE)
  count, want = m.select.sum(1), [bm.budget(int(c), p, P) for c in (np.asarray(sp) == 0).sum(1)]
  assert (count <= P).all() and ((count <= want).all() if wwm else count.tolist() == want)
  return m


@functools.lru_cache(maxsize=None)
def expect(code, wwm, P, p):
  """the unmasked padded batch (mode 0) of BERT / CODE and the model over it, once for every route"""
  enc = collate(code, wwm, P, p).collate_rows(world()[1], CODE if code else BERT, mode=0)
  return enc, host(enc['attention_mask']) != 0, model(host(enc['input_ids']), host(enc['special_tokens_mask']), wwm, P, p)


def check_route(col, route, res, idx, enc, keep, m, fixed, width, what):
  """one batch through one route against the model m over the unmasked batch enc (keep: its attention mask); col has
  compact_mlm=True: a capacity of slots * P that never raises"""
  want, slots, P = (m.input_ids, m.labels), len(idx), col.max_predictions
  if route == 'mask_tokens':
    got = col.mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], counter=col.counter)
  else:
    if route == 'fixed':
      out, slots = col.collate_rows_fixed(res, idx, **fixed), fixed['max_seqs']
      slack = fixed['max_tokens'] - int(keep.sum())
      want = np.concatenate([want[0][keep], np.zeros(slack, np.int64)]), np.concatenate([want[1][keep], np.full(slack, IGNORE)])
    elif route == 'unpadded':
      out, want = col.collate_rows_unpadded(res, idx), (want[0][keep], want[1][keep])
    else:
      out = col.collate_rows(res, idx)
    got = out['input_ids'], out['labels']
    pos, hit = host(out['masked_lm_positions']), np.flatnonzero(want[1].ravel() != IGNORE)
    assert pos.shape == (slots * P,) == tuple(out['masked_lm_labels'].shape)  # a capacity that never raises
    assert np.array_equal(pos[:len(hit)], hit) and not pos[len(hit):].any()
    assert np.array_equal(host(out['masked_lm_labels'])[:len(hit)], want[1].ravel()[hit])
    off = np.concatenate([[0], np.cumsum(m.select.sum(1)), np.full(slots - len(idx), len(hit))])  # (pad sequences: none)
    assert np.array_equal(host(out['masked_lm_offsets']), off)
    assert out['input_ids'].dim() == 1 or out['input_ids'].shape[1] == width
  assert np.array_equal(host(got[1]), want[1]), what
  assert np.array_equal(host(got[0]), want[0]), what
  return host(got[1])


@pytest.mark.parametrize('P', [1, 20, 80, 4096])
@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
@pytest.mark.parametrize('route', ['mask_tokens', 'rows', 'unpadded', 'fixed', 'code_rows'])
def test_route_equals_model(gpu, route, wwm, P):
  res, code = world()[1], route == 'code_rows'
  for p in (0.0, 0.15, 0.5, 1.0):
    enc, keep, m = expect(code, wwm, P, p)
    check_route(collate(code, wwm, P, p, compact_mlm=True), 'rows' if code else route, res, CODE if code else BERT, enc, keep,
                m, FIXED, 131 if code else 2048, (route, wwm, P, p))


def test_string_route(gpu):
  tok, _, segs, _ = world()
  samples = [tuple(' '.join(tok.ids_to_tokens[i] for i in seg) for seg in segs[g]) + (False,) for g in (3, 0, 5, 1, 6)]
  col = collate(False, True, 20, 0.15)
  enc = col.to_encoded_inputs(samples)
  m, out = model(host(enc['input_ids']), host(enc['special_tokens_mask']), True, 20, 0.15), col(samples)
  assert np.array_equal(host(out['labels']), m.labels) and np.array_equal(host(out['input_ids']), m.input_ids)
  assert all(torch.equal(out[k], enc[k]) for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'))


@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
def test_one_row_of_65536_columns(gpu, wwm):
  """budget 4096 of about 62 000 candidates: the search ends at the third level (an entry of budget_cases.CASES;
  tests/test_budget_model_host.py derives that without a GPU)"""
  case = next(c for c, level, _ in bc.CASES if c.n == 65536 and c.word == wwm and level == 2)
  assert (case.seed, case.counter, case.P, case.p) == (SEED, COUNTER, 4096, 0.15)
  ids, sp = bc.planes(case)
  x, lab = collate(False, wwm, 4096, 0.15).mask_tokens(torch.from_numpy(ids).cuda(), torch.from_numpy(sp).cuda(), counter=COUNTER)
  m = model(ids, sp, wwm, 4096, 0.15)
  assert np.array_equal(host(lab), m.labels) and np.array_equal(host(x), m.input_ids)
