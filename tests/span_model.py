"""Span dynamic masking (lddl_set_span_mask, defined in include/lddl_amd.h) in
numpy, over tests/mask_model.py and tests/wwm_model.py: the definition as a
plain sequential loop per row.  Plain helper module: no tests, no fixtures.

  params(L, g, p)                 (q, cdf[16]) from lddl_span_params, the doubles
                                  the kernels get (host only: no GPU, no ctx)
  law(L, g)                       P(len = l), l = 1 .. L, from the closed form
  mask(ids, special, table, ...)  Span: mask_model.Masked's planes, and the
                                  open heads, their drawn lengths and w(j)

ids and special are [n, S] planes as in wwm_model; table is its cont_table (a
bool per vocabulary entry: it begins with '##'), or None for a vocabulary
without continuations.
"""
import collections
import ctypes

import numpy as np

import mask_model as mm
import wwm_model as wm

SPAN_KEY = 0x5350414E4D41534B

Span = collections.namedtuple('Span', 'input_ids labels select masked random open length word')


def params(L, g, p):
  from lddl_amd import _lib
  q, cdf = ctypes.c_double(), (ctypes.c_double * 16)()
  rc = _lib.lib().lddl_span_params(L, g, p, ctypes.byref(q), cdf)
  if rc:
    raise ValueError('lddl_span_params(%r, %r, %r) = %d: %s' % (L, g, p, rc, _lib.lib().lddl_last_error().decode()))
  return q.value, np.asarray(list(cdf), np.float64)


def law(L, g):
  l = np.arange(1, L + 1, dtype=np.float64)
  return g * (1.0 - g) ** (l - 1) / (1.0 - (1.0 - g) ** L)


def mask(ids, special, table, seed, counter, p, L, g, mask_id, n_random, ignore, rows=None):
  """rows default to the plane's own row numbers, the columns are the plane's"""
  ids = np.asarray(ids, np.int64)
  sp = np.asarray(special) != 0
  n, S = ids.shape
  assert sp.shape == ids.shape
  rows = np.arange(n) if rows is None else np.asarray(rows)
  q, cdf = params(L, g, p)
  start = wm.starts(ids, sp, np.zeros(1, bool) if table is None else table)
  h = np.broadcast_to(mm.draws(seed, counter, rows[:, None], np.arange(S)[None, :]), (3, n, S))
  k = mm.sm(mm.u64(seed) ^ mm.sm(counter))
  ks = mm.sm(k ^ np.uint64(SPAN_KEY))
  with np.errstate(over='ignore'):
    i = ((mm.u64(rows)[:, None] << np.uint64(20)) | mm.u64(np.arange(S))[None, :]) * np.uint64(3)
    u_len = mm.unit(mm.sm(ks + i))
  u_open = mm.unit(h[0])
  select, opened = np.zeros((n, S), bool), np.zeros((n, S), bool)
  length, word = np.zeros((n, S), np.int64), np.zeros((n, S), np.int64)
  for r in range(n):
    w, heads = 0, []  # of the segment so far: its words, and (w(h), len(h)) of its open heads
    for j in range(S):
      if sp[r, j]:
        w, heads = 0, []
        continue
      if start[r, j]:
        w += 1
        if u_open[r, j] < q:
          opened[r, j] = True
          length[r, j] = 1 + sum(1 for t in range(1, L) if u_len[r, j] >= cdf[t - 1])
          heads.append((w, int(length[r, j])))
      word[r, j] = w
      heads = [(wh, lh) for wh, lh in heads if w - wh < lh]  # w only grows: a head left behind stays behind
      select[r, j] = bool(heads)
  masked = select & (mm.unit(h[1]) < 0.8)
  random = select & ~masked & (mm.unit(h[2]) < 0.5)
  rnd = (((h[2] & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)
  out = np.where(masked, np.int64(mask_id), np.where(random, rnd, ids))
  return Span(out, np.where(select, ids, np.int64(ignore)), select, masked, random, opened, length, word)
