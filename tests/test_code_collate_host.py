"""The CodeBERT loader without a GPU: its six entry points in the header, the
binding and the built library; the numpy model of tests/code_collate_model.py
against rows written out by hand; RowBatches' row lengths from flags bit 1."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import code_collate_model as cm
import mask_model as mm
from conftest import ROOT

ENTRY_POINTS = ['lddl_collate_code_rows_seq_len', 'lddl_collate_code_rows', 'lddl_collate_code_rows_cu_seqlens',
                'lddl_collate_code_rows_unpadded', 'lddl_code_rows_from_strings_len', 'lddl_code_rows_from_strings']
CLS, SEP, MASK = 101, 102, 103


def header():
  src = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  docs = {m.group(2): m.group(1) for m in re.finditer(r'/\*((?:(?!\*/).)*)\*/\s*int\s+(lddl_\w+)\s*\(', src, flags=re.S)}
  bare = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
  decl = {m.group(1): [p.strip() for p in ' '.join(m.group(2).split()).split(',')]
          for m in re.finditer(r'\bint\s+(lddl_\w+)\s*\(([^;{]*?)\)\s*;', bare, flags=re.S)}
  return docs, decl


def kind(c_param):
  if '*' in c_param or '[' in c_param:
    return 'ptr'
  return c_param.rsplit(' ', 1)[0].replace('const ', '').strip()


def ctypes_kind(t):
  if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
    return 'ptr'
  return {ctypes.c_int64: 'int64_t', ctypes.c_int32: 'int32_t', ctypes.c_double: 'double', ctypes.c_uint64: 'uint64_t'}[t]


@pytest.mark.parametrize('name', ENTRY_POINTS)
def test_entry_point_is_declared_bound_and_exported(name):
  from lddl_amd import build, _lib
  docs, decl = header()
  assert name in decl, 'not declared in include/lddl_amd.h'
  # the comment in front of it names the row it reads and says the reference has no loader for it
  text = ' '.join(re.sub(r'\n \*', '\n', docs[name]).split())
  assert 'pretrain_codebert.py:425-433' in text and 'no loader' in text, name
  res, args = _lib.SIGNATURES[name]
  assert res is ctypes.c_int
  assert [ctypes_kind(a) for a in args] == [kind(p) for p in decl[name]]
  build.build_hip()
  assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_arguments_follow_the_bert_calls():
  """no static arrays, no next_sentence_labels, d_flags in the two length
  calls, d_num_tokens in place of d_is_random_next and the static columns"""
  _, decl = header()
  names = lambda f: [p.split()[-1].lstrip('*').split('[')[0] for p in decl[f]]  # noqa: E731
  static = ['d_mlm_off', 'd_mlm_pos', 'd_mlm_label', 'd_mlm_token']
  for code, bert in (('lddl_collate_code_rows', 'lddl_collate_rows'),
                     ('lddl_collate_code_rows_unpadded', 'lddl_collate_rows_unpadded')):
    assert names(code) == [a for a in names(bert) if a not in static + ['d_next_sentence_labels']]
  for code, bert in (('lddl_collate_code_rows_seq_len', 'lddl_collate_rows_seq_len'),
                     ('lddl_collate_code_rows_cu_seqlens', 'lddl_collate_rows_cu_seqlens')):
    b = names(bert)
    assert names(code) == b[:3] + ['d_flags'] + b[3:]
  columns = ['d_pos', 'd_pos_off', 'd_lab', 'd_lab_off']
  rename = {'d_a': 'd_doc', 'd_a_off': 'd_doc_off', 'd_b': 'd_code', 'd_b_off': 'd_code_off'}
  b = [rename.get(a, a) for a in names('lddl_rows_from_strings_len') if a not in columns + ['d_out_mlm_off']]
  assert names('lddl_code_rows_from_strings_len') == b[:5] + ['d_num_tokens'] + b[5:]
  b = [rename.get(a, a) for a in names('lddl_rows_from_strings')
       if a not in columns + ['d_mlm_off', 'd_out_mlm_pos', 'd_out_mlm_label', 'd_out_mlm_token', 'mlm_cap']]
  assert names('lddl_code_rows_from_strings') == [('d_num_tokens' if a == 'd_is_random_next' else a) for a in b]


# ---- the numpy model against rows written out by hand -----------------------------
# (partition, doc ids, code ids, flags, bin, tokens) as PackResult.rows() gives them
PAIR = (0, [7, 8], [20, 21, 22], 2, 0, None)   # s = 1, a > 0
EMPTY_DOC = (0, [], [30, 31], 2, 0, None)      # s = 1, a = 0
SINGLE = (0, [], [40, 41, 42, 43], 0, 0, None)  # s = 0
ROWS = [PAIR, EMPTY_DOC, SINGLE]


def test_layout_of_each_regime():
  ids, tt, sp = cm.layout(PAIR, CLS, SEP)
  assert ids.tolist() == [CLS, 7, 8, SEP, 20, 21, 22, SEP]
  assert tt.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and sp.tolist() == [1, 0, 0, 1, 0, 0, 0, 1]
  ids, tt, sp = cm.layout(EMPTY_DOC, CLS, SEP)
  assert ids.tolist() == [CLS, SEP, 30, 31, SEP]
  assert tt.tolist() == [0, 0, 1, 1, 1] and sp.tolist() == [1, 1, 0, 0, 1]
  ids, tt, sp = cm.layout(SINGLE, CLS, SEP)
  assert ids.tolist() == [CLS, 40, 41, 42, 43, SEP]
  assert tt.tolist() == [0] * 6 and sp.tolist() == [1, 0, 0, 0, 0, 1]
  with pytest.raises(AssertionError):
    cm.layout((0, [7], [20], 0, 0, None), CLS, SEP)  # s = 0 with a > 0


def test_padded_model_mode_0():
  out = cm.padded(ROWS, [2, 0, 1], 4, 0, CLS, SEP)
  assert set(out) == {'input_ids', 'token_type_ids', 'attention_mask', 'special_tokens_mask'}
  assert out['input_ids'].tolist() == [[CLS, 40, 41, 42, 43, SEP, 0, 0], [CLS, 7, 8, SEP, 20, 21, 22, SEP],
                                       [CLS, SEP, 30, 31, SEP, 0, 0, 0]]
  assert out['token_type_ids'].tolist() == [[0] * 8, [0, 0, 0, 0, 1, 1, 1, 1], [0, 0, 1, 1, 1, 0, 0, 0]]
  assert out['attention_mask'].tolist() == [[1] * 6 + [0] * 2, [1] * 8, [1] * 5 + [0] * 3]
  assert out['special_tokens_mask'].tolist() == [[1, 0, 0, 0, 0, 1, 1, 1], [1, 0, 0, 1, 0, 0, 0, 1],
                                                 [1, 1, 0, 0, 1, 1, 1, 1]]
  assert cm.padded(ROWS, [1], 1, 0, CLS, SEP)['input_ids'].shape == (1, 5)
  assert cm.padded(ROWS, [1], 8, 0, CLS, SEP)['input_ids'].shape == (1, 8)


def test_unpadded_model_is_the_padded_one_without_padding():
  kw = dict(seed=5, counter=9, p=0.5, mask_id=MASK, n_random=1000, ignore=-100)
  idx = [2, 0, 1, 0]
  for mode in (0, 2):
    pad = cm.padded(ROWS, idx, 1, mode, CLS, SEP, **kw)
    out = cm.unpadded(ROWS, idx, mode, CLS, SEP, **kw)
    keep = pad['attention_mask'].astype(bool)
    for k in ('input_ids', 'token_type_ids', 'special_tokens_mask' if mode == 0 else 'labels'):
      assert np.array_equal(pad[k][keep], out[k]), (mode, k)
    assert out['cu_seqlens'].tolist() == [0, 6, 14, 19, 27] and out['cu_seqlens'].dtype == np.int32
    assert out['max_seqlen'] == 8
    assert out['position_ids'].tolist() == list(range(6)) + list(range(8)) + list(range(5)) + list(range(8))


def test_mode_2_is_mode_0_then_the_documented_draw():
  kw = dict(seed=77, counter=3, p=1.0, mask_id=MASK, n_random=1000, ignore=-1)
  plain = cm.padded(ROWS, [0, 1, 2], 8, 0, CLS, SEP)
  out = cm.padded(ROWS, [0, 1, 2], 8, 2, CLS, SEP, **kw)
  m = mm.mask(plain['input_ids'], plain['special_tokens_mask'], 77, 3, 1.0, MASK, 1000, -1)
  assert np.array_equal(out['input_ids'], m.input_ids) and np.array_equal(out['labels'], m.labels)
  # at probability 1 every token of a segment is selected and nothing else is
  assert np.array_equal(out['labels'] != -1, plain['special_tokens_mask'] == 0)
  assert np.array_equal(out['labels'][out['labels'] != -1], plain['input_ids'][plain['special_tokens_mask'] == 0])


# ---- RowBatches: a row's length from its flags --------------------------------------
def fake_table(len0, len1, flags):
  t = lambda a, dt: torch.from_numpy(np.asarray(a, dt))  # noqa: E731
  return types.SimpleNamespace(n_pairs=len(len0), nbins=1, len0=t(len0, np.int16), len1=t(len1, np.int16),
                               flags=t(flags, np.uint8), bins=t([0] * len(len0), np.uint8))


def test_row_batches_lengths_from_flags():
  from lddl_amd.loader import RowBatches, plan_token_batches
  len0, len1, flags = [0, 3, 0, 0, 5], [4, 4, 6, 1, 2], [0, 2, 2, 0, 2]
  rb = RowBatches(fake_table(len0, len1, flags), max_tokens=64)
  assert rb.lengths.tolist() == [6, 10, 9, 3, 10]
  assert [b.tolist() for b in rb.plan()] == [b.tolist() for b in plan_token_batches([6, 10, 9, 3, 10], 64)]
  # every BERT row has bit 1 set (with or without is_random_next): len0 + len1 + 3, the value of before
  bert = RowBatches(fake_table(len0, len1, [2, 3, 2, 3, 2]), max_tokens=64)
  assert bert.lengths.tolist() == [a + b + 3 for a, b in zip(len0, len1)]
  # a budget that the old count of + 3 would have split
  rows = fake_table([0] * 4, [2] * 4, [0] * 4)  # four rows of 4 tokens
  assert [len(b) for b in RowBatches(rows, max_tokens=16).plan()] == [4]
  assert [len(b) for b in plan_token_batches([5] * 4, 16)] == [3, 1]
