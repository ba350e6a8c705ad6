"""Time lddl_mlm_targets against the torch formulation of the same lists, on the GPU.

  call:    lddl_mlm_targets into preallocated outputs (capacity = the labels' size)
  method:  collate.mlm_targets(labels[, cu_seqlens]): the same call with its three allocations
  torch:   pos = torch.nonzero(labels.view(-1) != ignore_index).view(-1); tgt = labels.view(-1)[pos]
           (what a user writes today; no per-row offsets, and nonzero synchronises as the call does)

on the labels of dynamic masking (mask_tokens, p 0.15) for a padded batch
[256, 512] and for a padding-free stream of T = 65 536 tokens with its
cu_seqlens.  Each figure is one variant between HIP events on the stream,
labels already on the device; the variants alternate so that drift of a shared
host hits all of them.  Nothing here is a pass bar: both sides are
launch-bound.  Prints one JSON document; --out writes it to a file as well.

    python tools/time_mlm_targets.py [--reps 50] [--warmup 10] [--out FILE]
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

from lddl_amd import _lib  # noqa: E402
from lddl_amd.loader import BertCollate  # noqa: E402

IGNORE, P_MLM, S = -1, 0.15, 512


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


def stats(ms):
  q = statistics.quantiles(ms, n=4)
  return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
          'q1_ms': round(q[0], 4), 'q3_ms': round(q[2], 4), 'reps': len(ms)}


def dynamic_labels(col, lengths, seed):
  """the labels of mask_tokens over rows of the given lengths, [n, S] (ignore_index on the special tokens and the padding)"""
  rng = np.random.default_rng(seed)
  n = len(lengths)
  ids = rng.integers(1000, col.tok.vocab_size, (n, S)).astype(np.int64)
  sp = np.zeros((n, S), np.int64)
  for r, m in enumerate(lengths):
    sp[r, 0] = sp[r, m // 2] = sp[r, m - 1] = 1  # [CLS] and the two [SEP]
    sp[r, m:] = 1
  _, labels = col.mask_tokens(torch.from_numpy(ids).cuda(), torch.from_numpy(sp).cuda())
  return labels


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=50)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  assert a.reps >= 20
  dev = torch.device('cuda', 0)
  col = BertCollate(_lib.VOCAB_BERT, device=0, mlm_probability=P_MLM, ignore_index=IGNORE)
  L, h = _lib.lib(), col.tok.handle
  ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  rng = np.random.default_rng(512)
  report = {'gpu': torch.cuda.get_device_name(0), 'mlm_probability': P_MLM, 'ignore_index': IGNORE, 'cases': {}}

  # the padded batch
  cases = {'padded_256x512': (dynamic_labels(col, rng.integers(64, S + 1, 256), 1), None)}
  # the padding-free stream: rows of 64 .. 512 tokens until they hold exactly 65 536
  lengths, left = [], 65536
  while left:
    m = min(int(rng.integers(64, S + 1)), left)
    if 0 < left - m < 3:
      m -= 3  # (no row shorter than its special tokens)
    lengths.append(m)
    left -= m
  lab = dynamic_labels(col, lengths, 2)
  keep = torch.arange(S, device=dev)[None, :] < torch.tensor(lengths, device=dev)[:, None]
  cu = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32, device=dev)
  cases['unpadded_T65536'] = (lab[keep].contiguous(), cu)

  for name, (labels, cu) in cases.items():
    total = labels.numel()
    n = labels.shape[0] if cu is None else cu.numel() - 1
    seq = labels.shape[1] if cu is None else 0
    pos = torch.empty(total, dtype=torch.int64, device=dev)
    tgt = torch.empty(total, dtype=torch.int64, device=dev)
    off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    count = ctypes.c_int64()

    def call():
      _lib.check(L.lddl_mlm_targets(h, ptr(labels), n, seq, ptr(cu), total, IGNORE, total, ptr(pos), ptr(tgt), ptr(off),
                                    ctypes.byref(count), st))

    def method():
      return col.mlm_targets(labels, cu)

    def formulation():
      flat = labels.view(-1)
      p = torch.nonzero(flat != IGNORE).view(-1)
      return p, flat[p]

    call()
    mp, mt, _ = method()
    tp, tt = formulation()
    M = count.value
    assert M == tp.numel() and torch.equal(pos[:M], tp) and torch.equal(tgt[:M], tt), 'the call and torch differ'
    assert torch.equal(mp, tp) and torch.equal(mt, tt) and int(off[-1]) == M
    half = max(a.reps // 2, 10)
    ms = {'call': [], 'method': [], 'torch': []}
    for _ in range(2):
      ms['call'] += events(call, a.warmup, half)
      ms['method'] += events(method, a.warmup, half)
      ms['torch'] += events(formulation, a.warmup, half)
    r = {'n_rows': n, 'tokens': total, 'masked': M}
    r.update({k: stats(v) for k, v in ms.items()})
    r['call_over_torch_median'] = round(r['call']['median_ms'] / r['torch']['median_ms'], 3)
    r['method_over_torch_median'] = round(r['method']['median_ms'] / r['torch']['median_ms'], 3)
    report['cases'][name] = r
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
