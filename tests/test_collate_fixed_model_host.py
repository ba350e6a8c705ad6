"""The fixed-shape padding-free batch without a GPU: the invariants of the numpy
definition (tests/collate_fixed_model.py) on hand-made lengths, that
loader.fixed_seq_cap bounds the slots of every batch plan_token_batches makes,
and the registration of the two C calls and the Python methods."""
import inspect

import numpy as np
import pytest

import collate_fixed_model as fm

# (lengths, T, N, S): no slack; slack 1 at an odd and at an even total; slack S, S + 1, several S; n + p == N exactly;
# N much larger than n + p; one row
CASES = [
    ([3, 4, 7, 64, 65, 129], 272, 6, 129),
    ([3, 4, 7], 15, 4, 8),
    ([3, 4, 8], 16, 4, 8),
    ([3, 4, 7], 22, 4, 8),
    ([3, 4, 7], 23, 5, 8),
    ([3, 4, 7], 14 + 8 * 5 + 3, 9, 8),
    ([5, 16, 3], 24 + 16 * 2, 5, 16),
    ([3, 4, 7], 30, 500, 8),
    ([7], 8, 2, 8),
    ([8], 100, 13, 8),
]


@pytest.mark.parametrize('lengths,T,N,S', CASES)
def test_stream_is_exactly_covered_by_sequences(lengths, T, N, S):
  cu = fm.fixed_cu_seqlens(lengths, T, N, S)
  assert cu.dtype == np.int32 and cu.shape == (N + 1,)
  n, total = len(lengths), sum(lengths)
  p = fm.pad_seqs(total, T, S)
  assert cu[0] == 0 and cu[N] == T
  d = np.diff(cu.astype(np.int64))
  assert (d >= 0).all() and d.sum() == T          # consecutive, no gap, no overlap: every token in one sequence
  assert d.max() <= S                             # every sequence fits max_seqlen
  assert d[:n].tolist() == lengths
  assert (d[n:n + p] > 0).all() and (d[n:n + max(p - 1, 0)] == S).all()  # pad sequences are full but the last
  assert (d[n + p:] == 0).all() and (cu[n + p:] == T).all()               # empty slots sit at T
  assert p == (0 if total == T else (T - total + S - 1) // S)


def unpadded_of(lengths, mode, with_nsl=True):
  total = sum(lengths)
  rng = np.random.default_rng(5)
  out = {'input_ids': rng.integers(1, 1000, total), 'token_type_ids': rng.integers(0, 2, total),
         'position_ids': np.concatenate([np.arange(m) for m in lengths]),
         fm.label_key(mode): rng.integers(0, 2, total) if mode == 0 else np.where(rng.random(total) < .2, 77, -1),
         'cu_seqlens': np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)}
  if with_nsl:
    out['next_sentence_labels'] = rng.integers(0, 2, len(lengths))
  return out


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('lengths,T,N,S', CASES)
def test_fixed_batch_of_the_model(lengths, T, N, S, mode):
  unp = unpadded_of(lengths, mode)
  out = fm.fixed_batch(unp, T, N, S, -1, mode)
  n, total = len(lengths), sum(lengths)
  p = fm.pad_seqs(total, T, S)
  lk = fm.label_key(mode)
  assert set(out) == set(unp) | {'max_seqlen', 'num_tokens', 'num_rows', 'num_seqs', 'status'}
  for k in fm.TOKEN_KEYS + (lk,):
    assert out[k].shape == (T,) and out[k].dtype == np.int64
    assert np.array_equal(out[k][:total], unp[k])  # the real tokens first, unchanged
  assert not out['input_ids'][total:].any() and not out['token_type_ids'][total:].any()
  assert (out[lk][total:] == (1 if mode == 0 else -1)).all()
  cu = out['cu_seqlens']
  for r in range(n, n + p):  # positions restart in every pad sequence
    assert np.array_equal(out['position_ids'][cu[r]:cu[r + 1]], np.arange(cu[r + 1] - cu[r]))
  nsl = out['next_sentence_labels']
  assert nsl.shape == (N,) and np.array_equal(nsl[:n], unp['next_sentence_labels']) and (nsl[n:] == -1).all()
  assert (out['num_tokens'], out['num_rows'], out['num_seqs'], out['max_seqlen']) == (total, n, n + p, S)
  assert out['status'].tolist() == [total, n, n + p, S] and out['status'].dtype == np.int32
  assert 'next_sentence_labels' not in fm.fixed_batch(unpadded_of(lengths, mode, False), T, N, S, -1, mode)


def test_model_refusals():
  with pytest.raises(ValueError, match='tok_cap'):
    fm.fixed_cu_seqlens([3, 4, 7], 13, 9, 8)
  with pytest.raises(ValueError, match='max_seqlen'):
    fm.fixed_cu_seqlens([3, 9], 20, 9, 8)
  with pytest.raises(ValueError, match='seq_cap'):
    fm.fixed_cu_seqlens([3, 4, 7], 23, 4, 8)  # slack 9 = two pad sequences: 5 slots
  with pytest.raises(ValueError):
    fm.fixed_cu_seqlens([], 8, 4, 8)


# (max_tokens, max_rows, S); planner seeds 0..2, lengths from default_rng(100 + case)
PLANS = [(64, 4, 16), (64, 64, 16), (257, 7, 33), (1000, 3, 128), (4096, 40, 512), (4096, 9, 512), (513, 2, 512)]


@pytest.mark.parametrize('case', range(len(PLANS)))
def test_fixed_seq_cap_bounds_every_planned_batch(case):
  from lddl_amd.loader import fixed_seq_cap, plan_token_batches
  T, R, S = PLANS[case]
  N = fixed_seq_cap(T, R, S)
  assert N == R + -(-T // S)
  lengths = np.random.default_rng(100 + case).integers(3, S + 1, 700)
  for seed in range(3):
    plan = plan_token_batches(lengths, T, R, seed=seed, epoch=seed)
    assert sorted(np.concatenate(plan).tolist()) == list(range(len(lengths)))
    # every batch, the epoch's last one among them, and the shortest last batch an epoch can end with: one row
    for b in plan + [plan[-1][:1]]:
      cu = fm.fixed_cu_seqlens(lengths[b], T, N, S)  # raises where n + p > N, total > T or a row > S
      n, p = len(b), fm.pad_seqs(int(lengths[b].sum()), T, S)
      assert n + p <= N and cu[N] == T


def test_fixed_seq_cap_arguments():
  from lddl_amd.loader import fixed_seq_cap
  assert fixed_seq_cap(65536, 512, 512) == 512 + 128
  assert fixed_seq_cap(10, 1, 3) == 1 + 4
  assert 'max_rows + ceil(max_tokens / max_seqlen)' in fixed_seq_cap.__doc__
  for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
    with pytest.raises(ValueError):
      fixed_seq_cap(*bad)


def test_calls_and_methods_are_registered():
  from lddl_amd import _lib, loader
  for name in ('lddl_collate_rows_fixed', 'lddl_collate_code_rows_fixed'):
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)
  # the code twin drops the four static arrays and next_sentence_labels
  assert len(_lib.SIGNATURES['lddl_collate_rows_fixed'][1]) == len(_lib.SIGNATURES['lddl_collate_code_rows_fixed'][1]) + 5
  for cls in (loader.BertCollate, loader.CodeCollate, loader.MlmCollate):
    sig = inspect.signature(cls.collate_rows_fixed)
    assert list(sig.parameters) == ['self', 'res', 'rows', 'row0', 'n_rows', 'mode', 'max_tokens', 'max_seqs', 'max_seqlen']
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('max_tokens', 'max_seqs', 'max_seqlen'))
  assert 'fixed_seq_cap' in loader.RowBatches.__doc__
