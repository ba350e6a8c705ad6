"""The CodeBERT batch of CodeCollate (lddl_collate_code_rows and
lddl_collate_code_rows_unpadded) in numpy.  Plain helper module: no tests, no
fixtures.

Built from what PackResult.rows() returns, which honours flags bit 1, and from
tests/mask_model.py; it never looks at a kernel's output.  A row of rows() is
(partition, doc ids, code ids, flags, bin, tokens); with a = len(doc),
b = len(code), s = (flags >> 1) & 1 and n = a + b + 2 + s (include/lddl_amd.h):

  s = 1:  0 [CLS] | [1, a] doc | a + 1 [SEP] | [a + 2, n - 2] code | n - 1 [SEP]
  s = 0:  0 [CLS] | [1, n - 2] code | n - 1 [SEP]                  (a must be 0)

  layout(row, cls_id, sep_id)   (input_ids, token_type_ids, special_tokens_mask) of one row, [n] each
  padded(rows, idx, align, ...)    the dict of CodeCollate.collate_rows
  unpadded(rows, idx, ...)         the dict of CodeCollate.collate_rows_unpadded

mode 0 gives 'special_tokens_mask', mode 2 'labels' after mask_model.mask keyed
by (seed, counter, row of the batch, column of the row).
"""
import numpy as np

import mask_model as mm


def layout(row, cls_id, sep_id):
  doc, code, flags = row[1], row[2], row[3]
  a, s = len(doc), (flags >> 1) & 1
  assert s == 1 or a == 0, 'doc tokens and no [SEP] after them'
  ids = [cls_id] + list(doc) + ([sep_id] if s else []) + list(code) + [sep_id]
  n = len(ids)
  assert n == a + len(code) + 2 + s
  tt = np.zeros(n, np.int64)
  special = np.zeros(n, np.int64)
  special[[0, n - 1]] = 1
  if s:
    tt[a + 2:] = 1
    special[a + 1] = 1
  return np.asarray(ids, np.int64), tt, special


def _label_key(mode):
  assert mode in (0, 2)
  return 'special_tokens_mask' if mode == 0 else 'labels'


def padded(rows, idx, align, mode, cls_id, sep_id, seed=0, counter=0, p=0.15, mask_id=0, n_random=0, ignore=-1):
  rs = [layout(rows[int(g)], cls_id, sep_id) for g in idx]
  m = max(len(r[0]) for r in rs)
  S = (m - 1) // align * align + align
  ids, tt, am = (np.zeros((len(rs), S), np.int64) for _ in range(3))
  special = np.ones((len(rs), S), np.int64)  # the padding counts as special
  for r, (i, t, sp) in enumerate(rs):
    n = len(i)
    ids[r, :n], tt[r, :n], am[r, :n], special[r, :n] = i, t, 1, sp
  out = {'input_ids': ids, 'token_type_ids': tt, 'attention_mask': am}
  if mode == 0:
    out['special_tokens_mask'] = special
  else:
    out['input_ids'], out['labels'] = mm.mask(ids, special, seed, counter, p, mask_id, n_random, ignore)[:2]
  return out


def unpadded(rows, idx, mode, cls_id, sep_id, seed=0, counter=0, p=0.15, mask_id=0, n_random=0, ignore=-1):
  rs = [layout(rows[int(g)], cls_id, sep_id) for g in idx]
  lens = np.asarray([len(r[0]) for r in rs], np.int64)
  ids, tt, special = (np.concatenate([r[k] for r in rs]) for k in range(3))
  pos = np.concatenate([np.arange(n, dtype=np.int64) for n in lens])
  row = np.repeat(np.arange(len(rs), dtype=np.int64), lens)
  out = {'input_ids': ids, 'token_type_ids': tt, 'position_ids': pos,
         'cu_seqlens': np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), 'max_seqlen': int(lens.max())}
  if mode == 0:
    out['special_tokens_mask'] = special
  else:
    out['input_ids'], out['labels'] = mm.mask(ids, special, seed, counter, p, mask_id, n_random, ignore, rows=row,
                                              cols=pos)[:2]
  return out
