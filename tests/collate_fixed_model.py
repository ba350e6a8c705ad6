"""The fixed-shape padding-free batch (lddl_collate_rows_fixed,
collate_rows_fixed) in numpy, built from the padding-free batch it extends:
the real rows stay where they are, the slack [total, T) becomes pad sequences
of at most S tokens in the slots behind the rows, the remaining slots are
empty at T.  Shared by tests/test_collate_fixed_model_host.py and
tests/test_collate_fixed_gpu.py."""
import numpy as np

TOKEN_KEYS = ('input_ids', 'token_type_ids', 'position_ids')


def label_key(mode):
  return 'special_tokens_mask' if mode == 0 else 'labels'


def pad_seqs(total, T, S):
  """p: the pad sequences that a slack of T - total tokens is cut into"""
  return -(-(T - total) // S) if total < T else 0


def fixed_cu_seqlens(lengths, T, N, S):
  """int32 [N + 1]: the rows, the pad sequences of the slack, then empty slots
  at T; ValueError where the call refuses"""
  lengths = np.asarray(lengths, np.int64).reshape(-1)
  n, total = len(lengths), int(lengths.sum())
  if n == 0:
    raise ValueError('empty batch')
  if total > T:
    raise ValueError('%d tokens, tok_cap %d' % (total, T))
  if int(lengths.max()) > S:
    raise ValueError('a row of %d tokens, max_seqlen %d' % (int(lengths.max()), S))
  p = pad_seqs(total, T, S)
  if n + p > N:
    raise ValueError('%d rows and %d pad sequences, seq_cap %d' % (n, p, N))
  cu = np.full(N + 1, T, np.int64)
  cu[:n + 1] = np.concatenate([[0], np.cumsum(lengths)])
  cu[n + 1:n + p + 1] = np.minimum(total + S * np.arange(1, p + 1), T)
  return cu.astype(np.int32)


def fixed_batch(unp, T, N, S, ignore_index, mode):
  """unp: the padding-free batch as numpy arrays (the keys of
  collate_rows_unpadded; next_sentence_labels optional).  Returns the fixed
  batch: the same keys at the fixed shapes plus num_tokens, num_rows, num_seqs,
  max_seqlen and status."""
  cu_in = np.asarray(unp['cu_seqlens'], np.int64)
  n, total = len(cu_in) - 1, int(cu_in[-1])
  cu = fixed_cu_seqlens(np.diff(cu_in), T, N, S)
  p = pad_seqs(total, T, S)
  slack = np.arange(T - total, dtype=np.int64)
  fill = {'input_ids': np.zeros(T - total, np.int64), 'token_type_ids': np.zeros(T - total, np.int64),
          'position_ids': slack % S, label_key(mode): np.full(T - total, 1 if mode == 0 else ignore_index, np.int64)}
  out = {}
  for k, v in fill.items():
    real = np.asarray(unp[k], np.int64)
    assert real.shape == (total,), (k, real.shape, total)
    out[k] = np.concatenate([real, v])
  if 'next_sentence_labels' in unp:
    nsl = np.asarray(unp['next_sentence_labels'], np.int64)
    assert nsl.shape == (n,)
    out['next_sentence_labels'] = np.concatenate([nsl, np.full(N - n, ignore_index, np.int64)])
  out['cu_seqlens'] = cu
  out['max_seqlen'] = S
  out['num_tokens'], out['num_rows'], out['num_seqs'] = total, n, n + p
  out['status'] = np.asarray([total, n, n + p, S], np.int32)
  return out
