"""The compact MLM targets of lddl_mlm_targets (include/lddl_amd.h defines
them) in numpy: the dense labels of a batch define the result completely.

With F the ascending flat indices that lie inside a row and whose label is not
ignore_index, and M = len(F):
  positions[k] = F[k], target_labels[k] = labels[F[k]]      for k < M
  positions[k] = 0,    target_labels[k] = ignore_index      for M <= k < capacity
  offsets[r] = the selected tokens of the rows before r; offsets[n_rows] = M
Rows: those of a 2-D labels array, or [cu_seqlens[r], cu_seqlens[r + 1]) of a
1-D one (tokens in no row are not selected)."""
import collections

import numpy as np

Targets = collections.namedtuple('Targets', 'positions target_labels offsets count')


def targets(labels, ignore_index, cu_seqlens=None, capacity=None):
  """capacity None: exactly M entries"""
  labels = np.asarray(labels, np.int64)
  flat = labels.reshape(-1)
  if cu_seqlens is None:
    assert labels.ndim == 2
    n, S = labels.shape
    cu = np.arange(n + 1, dtype=np.int64) * S
  else:
    assert labels.ndim == 1
    cu = np.asarray(cu_seqlens, np.int64)
    assert cu[0] >= 0 and (np.diff(cu) >= 0).all() and cu[-1] <= flat.size
  in_row = np.zeros(flat.size, bool)
  counts = []
  for lo, hi in zip(cu[:-1], cu[1:]):
    in_row[lo:hi] = True
    counts.append(np.count_nonzero(flat[lo:hi] != ignore_index))
  F = np.flatnonzero(in_row & (flat != ignore_index)).astype(np.int64)
  M = F.size
  offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
  assert offsets[-1] == M
  K = M if capacity is None else int(capacity)
  assert M <= K
  positions = np.zeros(K, np.int64)
  target_labels = np.full(K, ignore_index, np.int64)
  positions[:M] = F
  target_labels[:M] = flat[F]
  return Targets(positions, target_labels, offsets, M)
