"""Span corruption (lddl_collate_corrupt_rows, defined in include/lddl_amd.h) in
numpy, over tests/infill_model.py: the definition as a plain sequential loop
per row.  Plain helper module: no tests, no fixtures.

  row(ids, special, ...)   (the encoder's tokens, the target, selected, ord) of one row
"""
import numpy as np

import infill_model as im


def row(ids, special, table, seed, counter, r, q, cdf, L, base, S, sep):
  """ids, special: the n columns of batch row r; table: wwm_model.cont_table;
  sentinel(k) = base + k for k < S.  ord[j]: the ordinal of the run that
  column j lies in, -1 outside the runs"""
  _, sel = im.row(ids, special, table, seed, counter, r, q, cdf, L, 0)
  enc, tgt, ords, k = [], [], [], -1
  for j, x in enumerate(int(x) for x in ids):
    opens = bool(sel[j]) and (j == 0 or not sel[j - 1])
    k += opens
    ords.append(k if sel[j] else -1)
    if not (sel[j] and k < S):
      enc.append(x)
      continue
    if opens:
      enc.append(base + k)
      tgt.append(base + k)
    tgt.append(x)
  tgt.append(sep)
  return np.asarray(enc, np.int64), np.asarray(tgt, np.int64), sel, np.asarray(ords)
