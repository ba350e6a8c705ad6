"""Exact-count span corruption (lddl_collate_corrupt_exact_rows, defined in
include/lddl_amd.h) in numpy: the counts with np.rint, the two gap choices as an
argsort of the keys, the interleave, then tests/corrupt_model.py's encoder /
target construction over the resulting `selected`.  Plain helper module: no
tests, no fixtures.

  counts(n, density, mean, S_max)   (N, S) of a row of n columns
  lengths(n, ...)                   (e_r, t_r, N, S)
  selected(n, ...)                  bool [n]
  row(ids, ...)                     (the encoder's tokens, the target, selected) of one row
"""
import numpy as np

import mask_model as mm

C_NOISE, C_PLAIN = 0x5345474E4F495345, 0x534547504C41494E


def counts(n, density, mean, S_max):
  c = n - 2
  if c < 2:
    return 0, 0
  N = int(min(max(np.rint(c * np.float64(density)), 1), c - 1))
  return N, int(min(max(np.rint(N / np.float64(mean)), 1), N, c - N, S_max))


def lengths(n, density, mean, S_max):
  N, S = counts(n, density, mean, S_max)
  return n - N + S, N + S + 1, N, S


def cuts(k, C, r, G, K):
  """the K of the gaps 0 .. G - 1 with the smallest keys, ascending"""
  kt = mm.sm(k ^ mm.u64(C))
  g = np.arange(G, dtype=np.uint64)
  with np.errstate(over='ignore'):
    h = mm.sm(kt + ((mm.u64(r) << np.uint64(20)) | g) * np.uint64(3))
  key = (h & ~np.uint64(0xFFFFF)) | g
  return np.sort(np.argsort(key)[:K])


def selected(n, seed, counter, r, density, mean, S_max):
  N, S = counts(n, density, mean, S_max)
  sel = np.zeros(n, bool)
  if S == 0:
    return sel
  c, k = n - 2, mm.sm(mm.u64(seed) ^ mm.sm(counter))
  # cumulative lengths: a cut at gap g ends a span behind item g of its kind
  A = np.concatenate([[0], cuts(k, C_NOISE, r, N - 1, S - 1) + 1, [N]])
  B = np.concatenate([[0], cuts(k, C_PLAIN, r, c - N - 1, S - 1) + 1, [c - N]])
  for s in range(1, S + 1):  # the interior reads b_1 a_1 b_2 a_2 ...; its token i is column i + 1
    sel[1 + B[s] + A[s - 1]:1 + B[s] + A[s]] = True
  return sel


def row(ids, seed, counter, r, density, mean, base, S_max, sep):
  """corrupt_model.row's construction with this module's `selected`; ord < S <= S_max: every run is corrupted"""
  sel = selected(len(ids), seed, counter, r, density, mean, S_max)
  enc, tgt, k = [], [], -1
  for j, x in enumerate(int(x) for x in ids):
    opens = bool(sel[j]) and not sel[j - 1]  # (column 0 is never selected)
    k += opens
    if not sel[j]:
      enc.append(x)
      continue
    if opens:
      enc.append(base + k)
      tgt.append(base + k)
    tgt.append(x)
  tgt.append(sep)
  return np.asarray(enc, np.int64), np.asarray(tgt, np.int64), sel
