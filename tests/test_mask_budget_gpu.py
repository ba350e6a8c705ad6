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

import budget_model as bm
import synth_vocab as sv
import wwm_model as wm

pytestmark = pytest.mark.gpu

V, MASK, IGNORE, SEED, COUNTER = 64, 4, -1, (1 << 63) + 12345, 1 << 40
# (tokens, s, '##' density; 'word': segment 0 is one word)
ROWS = [(5, 1, 0), (9, 1, .3), (64, 1, .3), (65, 1, 'word'), (128, 1, 0), (129, 1, .3), (512, 1, 'word'), (2048, 1, .3),
        (7, 1, .3), (131, 0, .3), (130, 1, .3)]
BERT, CODE = [7, 3, 0, 5, 1, 2, 8, 4, 6, 10], [9, 3, 0, 5, 2, 8]
FIXED = dict(max_tokens=3100, max_seqs=12, max_seqlen=2048)


def host(t):
  return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def world():
  """tokenizer, the rows as a PackResult with spans, their (A, B) ids, the '##' table"""
  from lddl_amd import pipeline
  from lddl_amd.tokenizer import Tokenizer
  tok = Tokenizer(sv.vocab_path('tiny64'), 0)
  rng = np.random.default_rng(5)
  ids, src, lens, segs = [0], ([], []), ([], []), []
  for n, s, dens in ROWS:
    a = (n - 3) // 2 if s else 0
    seg = []
    for k, m in enumerate((a, n - 2 - s - a)):
      d = 1.0 if dens == 'word' and k == 0 else 0.3 if dens else 0.0
      seg.append(np.where(rng.random(m) < d, rng.integers(31, 57, m), rng.integers(5, 31, m)).tolist())
      src[k].append(len(ids))
      lens[k].append(m)
      ids += seg[k]
    segs.append(seg)
  n, ntok = len(ROWS), np.asarray([r[0] for r in ROWS], np.int64)

  def t(a, dt):
    a = np.ascontiguousarray(np.asarray(a, dt))
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
  res = pipeline.PackResult(n, int(ntok.sum()), 1, None, t(np.concatenate([[0], np.cumsum(ntok)]), np.int64),
                            t(lens[0], np.uint16), t(lens[1], np.uint16), t([r[1] * 2 for r in ROWS], np.uint8),
                            t(np.zeros(n), np.uint8), t(np.zeros(n), np.int64), t([[n]], np.int64))
  res.ids, res.src0, res.src1 = t(ids + [0] * 16, np.uint16), t(src[0], np.int64), t(src[1], np.int64)
  res.cls_id, res.sep_id = tok.cls_id, tok.sep_id
  return tok, res, segs, wm.cont_table(tok.ids_to_tokens)


def collate(code, wwm, P, p, **kw):
  from lddl_amd.loader import BertCollate, CodeCollate
  col = (CodeCollate if code else BertCollate)(tokenizer=world()[0], base_seed=SEED, mlm_probability=p, whole_word_mask=wwm,
                                               max_predictions=P, sequence_length_alignment=1 if code else 8, **kw)
  col.counter = COUNTER
  return col


def model(ids, sp, wwm, P, p):
  m = bm.mask(ids, sp, world()[3] if wwm else None, SEED, COUNTER, p, P, MASK, V, IGNORE)
  count, want = m.select.sum(1), [bm.budget(int(c), p, P) for c in (np.asarray(sp) == 0).sum(1)]
  assert (count <= P).all() and ((count <= want).all() if wwm else count.tolist() == want)
  return m


@functools.lru_cache(maxsize=None)
def expect(code, wwm, P, p):
  """the unmasked padded batch (mode 0) of BERT / CODE and the model over it, once for every route"""
  enc = collate(code, wwm, P, p).collate_rows(world()[1], CODE if code else BERT, mode=0)
  return enc, host(enc['attention_mask']) != 0, model(host(enc['input_ids']), host(enc['special_tokens_mask']), wwm, P, p)


@pytest.mark.parametrize('P', [1, 20, 80, 4096])
@pytest.mark.parametrize('wwm', [False, True], ids=['tokens', 'words'])
@pytest.mark.parametrize('route', ['mask_tokens', 'rows', 'unpadded', 'fixed', 'code_rows'])
def test_route_equals_model(gpu, route, wwm, P):
  res, code = world()[1], route == 'code_rows'
  idx = CODE if code else BERT
  for p in (0.0, 0.15, 0.5, 1.0):
    enc, keep, m = expect(code, wwm, P, p)
    col = collate(code, wwm, P, p, compact_mlm=True)
    want, slots = (m.input_ids, m.labels), len(idx)
    if route == 'mask_tokens':
      got = col.mask_tokens(enc['input_ids'].clone(), enc['special_tokens_mask'], counter=COUNTER)
    else:
      if route == 'fixed':
        out, slots = col.collate_rows_fixed(res, idx, **FIXED), FIXED['max_seqs']
        slack = FIXED['max_tokens'] - int(keep.sum())
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
      assert out['input_ids'].dim() == 1 or out['input_ids'].shape[1] == (131 if code else 2048)
    assert np.array_equal(host(got[1]), want[1]), (route, wwm, P, p)
    assert np.array_equal(host(got[0]), want[0]), (route, wwm, P, p)


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
  """budget 4096 of about 62 000 candidates; with these ids (generator seed 4,
  chosen by running the radix search on the host) the crossing bin of the
  second level holds several heads and the search goes on to the third"""
  rng = np.random.default_rng(4)
  ids = np.where(rng.random((1, 65536)) < 0.3, rng.integers(31, 57, (1, 65536)), rng.integers(5, 31, (1, 65536)))
  sp = (rng.random((1, 65536)) < 0.05).astype(np.int64)
  x, lab = collate(False, wwm, 4096, 0.15).mask_tokens(torch.from_numpy(ids).cuda(), torch.from_numpy(sp).cuda(), counter=COUNTER)
  m = model(ids, sp, wwm, 4096, 0.15)
  assert np.array_equal(host(lab), m.labels) and np.array_equal(host(x), m.input_ids)
