"""Text infilling (lddl_collate_infill_rows, defined in include/lddl_amd.h) in
numpy, over tests/mask_model.py and tests/wwm_model.py: the definition as a
plain sequential loop per row.  Plain helper module: no tests, no fixtures.

  params(L, lam, ratio)    (q, cdf[16]) from lddl_infill_params (host only)
  row(ids, special, ...)   (the encoder's tokens, selected) of one row
"""
import ctypes

import numpy as np

import mask_model as mm
import wwm_model as wm
from span_model import SPAN_KEY


def params(L, lam, ratio):
  from lddl_amd import _lib
  q, cdf = ctypes.c_double(), (ctypes.c_double * 16)()
  rc = _lib.lib().lddl_infill_params(L, lam, ratio, ctypes.byref(q), cdf)
  if rc:
    raise ValueError('lddl_infill_params(%r, %r, %r) = %d' % (L, lam, ratio, rc))
  return q.value, np.asarray(list(cdf), np.float64)


def row(ids, special, table, seed, counter, r, q, cdf, L, mask_id):
  """ids, special: the n columns of batch row r; table: wwm_model.cont_table"""
  ids, sp = np.asarray(ids, np.int64), np.asarray(special) != 0
  cols = np.arange(len(ids))
  start = wm.starts(ids[None], sp[None], table)[0]
  k = mm.sm(mm.u64(seed) ^ mm.sm(counter))
  ks = mm.sm(k ^ np.uint64(SPAN_KEY))
  with np.errstate(over='ignore'):
    i = ((mm.u64(r) << np.uint64(20)) | mm.u64(cols)) * np.uint64(3)
    u_open, u_len = mm.unit(mm.sm(k + i)), mm.unit(mm.sm(ks + i))
  sel, out = np.zeros(len(ids), bool), []
  w, heads = 0, []  # of the segment so far: its words, and (w(h), len(h)) of its open heads
  for j in cols:
    if sp[j]:
      w, heads = 0, []
    else:
      if start[j]:
        w += 1
        if u_open[j] < q:
          heads.append((w, 1 + sum(1 for t in range(1, L) if u_len[j] >= cdf[t - 1])))
      heads = [(wh, lh) for wh, lh in heads if w - wh < lh]
      sel[j] = bool(heads)
    if not sel[j]:
      out.append(int(ids[j]))
    elif j == 0 or not sel[j - 1]:
      out.append(mask_id)
  return np.asarray(out, np.int64), sel
