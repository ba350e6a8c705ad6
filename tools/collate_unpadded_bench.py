"""Time the padded and the padding-free collate of the same rows, on the GPU.

  padded:    lddl_collate_rows_seq_len + lddl_collate_rows            (the yardstick)
  unpadded:  lddl_collate_rows_cu_seqlens + lddl_collate_rows_unpadded

mode 2, for one batch of 256 rows and one of 8 192 rows drawn (seeded) from
one seq-512 / bin-64 pack result of a synthetic corpus, and for one
RowBatches(res, max_tokens=...) batch of about the same token count (rows of
all bins, cut by tokens).  Each figure is the pair of C calls between HIP
events on the stream, inputs and outputs already on the device (each call
includes its read-back and synchronise); the two routes alternate so that
drift of a shared host hits both.  stored bytes: padded 32 B per column,
unpadded 32 B per token, + 8 B (+ 4 B of cu_seqlens) per row.  Prints one
JSON document; --out writes it to a file as well.

    python tools/collate_unpadded_bench.py [--mb 10] [--reps 30] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lddl_amd import _lib, pipeline, synth  # noqa: E402
from lddl_amd.loader import RowBatches  # noqa: E402


def events(fn, warmup, reps):
  """ms per call of fn() between events on the current stream"""
  for _ in range(warmup):
    fn()
  ms = []
  for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  return ms


def stats(ms, stored):
  d = {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
       'reps': len(ms), 'stored_bytes': stored}
  d['stored_TBps'] = round(stored / (d['median_ms'] * 1e-3) / 1e12, 3)
  return d


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--mb', type=float, default=10.0, help='synthetic corpus size')
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--sizes', type=int, nargs='+', default=[256, 8192])
  ap.add_argument('--whole-word', action='store_true', help='whole-word masking on (lddl_set_whole_word_mask): both calls')
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  assert a.reps >= 20
  dev = torch.device('cuda', 0)
  c = synth.make_wiki(int(a.mb * 1e6), seed=512)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 4), dev)
  res = pk.run(sh, target_seq_length=512, bin_size=64, duplicate_factor=2, seed=1, spans=True)
  torch.cuda.synchronize()
  L = _lib.lib()
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  h = pk.tok.handle
  st = P(torch.cuda.current_stream().cuda_stream)
  if a.whole_word:
    _lib.check(L.lddl_set_whole_word_mask(h, 1))
  report = {'gpu': torch.cuda.get_device_name(0), 'n_pairs': res.n_pairs, 'corpus_mb': a.mb, 'seq': 512, 'bin': 64,
            'mode': 2, 'whole_word': a.whole_word, 'batches': {}}

  def measure(idx):
    n = idx.numel()
    seq, total, longest = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    cu = torch.empty(n + 1, dtype=torch.int32, device=dev)

    def pad_len():
      _lib.check(L.lddl_collate_rows_seq_len(h, p(res.len0), p(res.len1), p(idx), 0, n, res.n_pairs, 8,
                                             ctypes.byref(seq), st))

    def unp_len():
      _lib.check(L.lddl_collate_rows_cu_seqlens(h, p(res.len0), p(res.len1), p(idx), 0, n, res.n_pairs, p(cu),
                                                ctypes.byref(total), ctypes.byref(longest), st))

    pad_len()
    unp_len()
    S, T = seq.value, total.value
    out = torch.empty((4, n, S), dtype=torch.int64, device=dev)
    flat = torch.empty((4, T), dtype=torch.int64, device=dev)
    nsl = torch.empty(n, dtype=torch.int64, device=dev)

    def padded():
      pad_len()
      _lib.check(L.lddl_collate_rows(h, p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1), p(res.flags),
                                     p(idx), 0, n, res.n_pairs, P(0), P(0), P(0), P(0), S, 2, -1, 0.15, 7, 3,
                                     p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(nsl), st))

    def unpadded():
      unp_len()
      _lib.check(L.lddl_collate_rows_unpadded(h, p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1),
                                              p(res.flags), p(idx), 0, n, res.n_pairs, P(0), P(0), P(0), P(0), p(cu),
                                              T, 2, -1, 0.15, 7, 3, p(flat[0]), p(flat[1]), p(flat[2]), p(flat[3]),
                                              p(nsl), st))

    padded()
    unpadded()
    torch.cuda.synchronize()
    m = out[2].bool()
    assert torch.equal(out[0][m], flat[0]) and torch.equal(out[3][m], flat[3]), 'the two routes differ'
    half = max(a.reps // 2, 10)
    pm, um = [], []
    for _ in range(2):
      pm += events(padded, a.warmup, half)
      um += events(unpadded, a.warmup, half)
    r = {'n_rows': n, 'seq_len': S, 'tokens': T, 'max_seqlen': longest.value,
         'padding_fraction': round(1.0 - T / (n * S), 4),
         'padded': stats(pm, n * S * 32 + n * 8), 'unpadded': stats(um, T * 32 + n * 8 + (n + 1) * 4)}
    r['unpadded_over_padded_median'] = round(r['unpadded']['median_ms'] / r['padded']['median_ms'], 3)
    r['ranges_overlap'] = bool(r['unpadded']['min_ms'] <= r['padded']['max_ms'] and
                               r['padded']['min_ms'] <= r['unpadded']['max_ms'])
    return r

  for n in a.sizes:
    assert res.n_pairs >= n, 'corpus too small: %d rows' % res.n_pairs
    idx = torch.from_numpy(np.random.default_rng(n).permutation(res.n_pairs)[:n]).to(dev)
    r = measure(idx)
    # one token-budget batch of about as many tokens: rows of all bins, cut by tokens
    # (seed n + 1: seed n, epoch 0 seeds the permutation that drew idx above)
    plan = RowBatches(res, max_tokens=r['tokens'], seed=n + 1).plan()
    r['token_budget_batch'] = measure(torch.from_numpy(plan[0]).to(dev))
    report['batches'][str(n)] = r
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
