"""Time the fixed-shape padding-free collate against the two-call route it fuses, on the GPU.

  two_call:  lddl_collate_rows_cu_seqlens + lddl_collate_rows_unpadded   (the baseline: the existing route)
  one_call:  lddl_collate_rows_fixed

over the batches of one plan: BERT rows packed at target_seq_length 512,
RowBatches(res, max_tokens=65536, max_rows=R), mode 2.  Three pairs:

  calls            the C calls into preallocated outputs (the baseline's sized for max_tokens, so neither allocates)
  methods          collate_rows_unpadded / collate_rows_fixed, with their allocations
  methods_compact  the same with compact_mlm=K

Each sample is one batch collated and synchronised, timed between HIP events
on the stream.  The two routes alternate batch by batch after a warm-up over
the same batches, so that drift of a shared host hits both; every repeat walks
the same batches.  spread = q3 - q1 of a route's samples.  Prints one JSON
document; --out writes it to a file as well.

    python tools/time_collate_fixed.py [--mb 12] [--batches 8] [--reps 12] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lddl_amd import _lib, pipeline, synth  # noqa: E402
from lddl_amd.loader import BertCollate, RowBatches, fixed_seq_cap  # noqa: E402

T, R, S, K = 65536, 512, 512, 12288


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def stats(ms):
  q = statistics.quantiles(ms, n=4)
  return {'median_ms': round(statistics.median(ms), 4), 'q1_ms': round(q[0], 4), 'q3_ms': round(q[2], 4),
          'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4), 'spread_ms': round(q[2] - q[0], 4), 'samples': len(ms)}


def pair(two, one, batches, warmup, reps):
  """two(idx), one(idx): the routes; alternating, batch by batch"""
  for _ in range(warmup):
    for idx in batches:
      two(idx)
      one(idx)
  torch.cuda.synchronize()
  tm, om = [], []
  for _ in range(reps):
    for idx in batches:
      tm.append(timed(lambda: two(idx)))
      om.append(timed(lambda: one(idx)))
  r = {'two_call': stats(tm), 'one_call': stats(om)}
  r['one_over_two_median'] = round(r['one_call']['median_ms'] / r['two_call']['median_ms'], 3)
  r['one_within_two_plus_spread'] = bool(r['one_call']['median_ms'] <= r['two_call']['median_ms'] + r['two_call']['spread_ms'])
  return r


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--mb', type=float, default=12.0, help='synthetic corpus size')
  ap.add_argument('--batches', type=int, default=8)
  ap.add_argument('--reps', type=int, default=12)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda', 0)
  c = synth.make_wiki(int(a.mb * 1e6), seed=512)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 4), dev)
  res = pk.run(sh, target_seq_length=512, bin_size=64, duplicate_factor=2, seed=1, spans=True)
  torch.cuda.synchronize()
  batches = list(RowBatches(res, max_tokens=T, max_rows=R, seed=3))[:a.batches]
  assert len(batches) == a.batches, 'corpus too small: %d full batches' % len(batches)
  N = fixed_seq_cap(T, R, S)
  L, h = _lib.lib(), pk.tok.handle
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  st = P(torch.cuda.current_stream().cuda_stream)
  table = (p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1), p(res.flags))
  none4 = (P(0),) * 4
  draw = (2, -1, 0.15, 7, 3)

  flat = torch.empty((2, 4, T), dtype=torch.int64, device=dev)
  cu = torch.empty((2, N + 1), dtype=torch.int32, device=dev)
  nsl = torch.empty((2, N), dtype=torch.int64, device=dev)
  status = torch.empty(4, dtype=torch.int32, device=dev)
  total, longest, n_rows, n_seqs = (ctypes.c_int64() for _ in range(4))

  def two_call(idx):
    n = idx.numel()
    _lib.check(L.lddl_collate_rows_cu_seqlens(h, p(res.len0), p(res.len1), p(idx), 0, n, res.n_pairs, p(cu[0]),
                                              ctypes.byref(total), ctypes.byref(longest), st))
    _lib.check(L.lddl_collate_rows_unpadded(h, *table, p(idx), 0, n, res.n_pairs, *none4, p(cu[0]), total.value, *draw,
                                            p(flat[0, 0]), p(flat[0, 1]), p(flat[0, 2]), p(flat[0, 3]), p(nsl[0]), st))

  def one_call(idx):
    _lib.check(L.lddl_collate_rows_fixed(h, *table, p(idx), 0, idx.numel(), res.n_pairs, *none4, p(cu[1]), T, N, S, *draw,
                                         p(flat[1, 0]), p(flat[1, 1]), p(flat[1, 2]), p(flat[1, 3]), p(nsl[1]), p(status),
                                         ctypes.byref(total), ctypes.byref(n_rows), ctypes.byref(n_seqs), st))

  tokens = []
  for idx in batches:  # the two routes agree on every batch that is timed
    two_call(idx)
    t = total.value
    one_call(idx)
    assert total.value == t and n_rows.value == idx.numel()
    assert torch.equal(flat[0, :, :t], flat[1, :, :t]) and torch.equal(cu[0, :idx.numel() + 1], cu[1, :idx.numel() + 1])
    assert int(cu[1, N]) == T and bool((flat[1, 3, t:] == -1).all())
    tokens.append(t)

  report = {'gpu': torch.cuda.get_device_name(0), 'n_pairs': res.n_pairs, 'corpus_mb': a.mb, 'seq': 512, 'mode': 2,
            'max_tokens': T, 'max_rows': R, 'max_seqlen': S, 'max_seqs': N, 'compact_mlm': K,
            'batches': [{'rows': int(i.numel()), 'tokens': t} for i, t in zip(batches, tokens)], 'pairs': {}}
  report['pairs']['calls'] = pair(two_call, one_call, batches, a.warmup, a.reps)
  for name, kw in (('methods', {}), ('methods_compact', {'compact_mlm': K})):
    col = BertCollate(tokenizer=pk.tok, base_seed=7, **kw)
    report['pairs'][name] = pair(lambda idx: col.collate_rows_unpadded(res, idx, mode=2),
                                 lambda idx: col.collate_rows_fixed(res, idx, mode=2, max_tokens=T, max_seqs=N, max_seqlen=S),
                                 batches, a.warmup, a.reps)
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
