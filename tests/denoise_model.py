"""BART's full denoising collate (lddl_collate_denoise_rows, defined in include/lddl_amd.h) in numpy, over
tests/infill_model.py and tests/mask_model.py: a sequential sentence split, the permutation by key ranks, text
infilling over the permuted row, random replacement at the openings.  Plain helper module: no tests, no fixtures."""
import collections
import math

import numpy as np

import infill_model as im
import mask_model as mm

PERMUTE_KEY, REPLACE_KEY = 0x5045524D53454E54, 0x52414E44544F4B4E  # "PERMSENT", "RANDTOKN"

Row = collections.namedtuple('Row', 'enc sel permuted orders replaced')


def sentences(ids, lo, hi, stop):
  out, first = [], lo
  for j in range(lo, hi):
    if (ids[j] == stop and not (j > lo and ids[j - 1] == stop)) or j == hi - 1:
      out.append((first, j + 1))
      first = j + 1
  return out


def _hash(seed, counter, key, r, cols):
  k = mm.sm(mm.sm(mm.u64(seed) ^ mm.sm(counter)) ^ np.uint64(key))
  with np.errstate(over='ignore'):
    return mm.sm(k + ((mm.u64(r) << np.uint64(20)) | mm.u64(cols)) * np.uint64(3))


def ordering(seed, counter, r, g, m, ratio):
  K = min(m, math.ceil(m * ratio))
  order = np.arange(m)
  if K < 2:
    return order
  i = np.arange(m)
  key = (_hash(seed, counter, PERMUTE_KEY, r, g << 11 | i) >> np.uint64(32) << np.uint64(32)) | mm.u64(i)
  by_rank = np.argsort(key)  # by_rank[k]: the sentence of rank k
  order[np.sort(by_rank[:K])] = by_rank[:K]
  return order


def row(ids, special, table, seed, counter, r, q, cdf, L, mask_id, n_random, permute_ratio, random_ratio, stop):
  ids, sp = np.asarray(ids, np.int64), np.asarray(special) != 0
  permuted, orders = ids.copy(), {}
  marks = np.flatnonzero(sp)  # [CLS], the inner [SEP] if there is one, the last [SEP]
  for g, (lo, hi) in enumerate(zip(marks[:-1] + 1, marks[1:])):
    sents = sentences(ids, lo, hi, stop)
    if sents:
      orders[g] = ordering(seed, counter, r, g, len(sents), permute_ratio)
      permuted[lo:hi] = np.concatenate([ids[slice(*sents[o])] for o in orders[g]])
  enc, sel = im.row(permuted, sp, table, seed, counter, r, q, cdf, L, mask_id)
  opening = sel & ~np.concatenate([[False], sel[:-1]])
  place = np.cumsum(~sel | opening) - 1  # of an emitted column in enc
  h = _hash(seed, counter, REPLACE_KEY, r, np.arange(len(ids)))
  replaced = opening & (mm.unit(h) < random_ratio)
  enc[place[replaced]] = (((h & np.uint64(0xFFFFFFFF)) * np.uint64(n_random)) >> np.uint64(32)).astype(np.int64)[replaced]
  return Row(enc, sel, permuted, orders, replaced[opening])
