"""Time what mode 2 of lddl_collate_rows costs under each selection, on the GPU.

One fixed batch of 256 rows x 512 columns, every row full, 30 % '##' ids,
p = 0.15.  Variants, switched on the ctx between calls: token, whole-word, and
the two with lddl_set_mask_budget(80) on (exact-count masking: the call then
launches mask_budget_kernel in front of the fill).  A library without
lddl_set_mask_budget (LDDL_LIB: the parent commit's, for an A/B of the switch
off) runs the first two only.  Device events around each call, which includes
its 4-byte error-word read-back; the variants alternate call by call after a
warm-up; median and quartiles in microseconds.  Prints one JSON document;
--out writes it to a file as well.

    python tools/mask_select_bench.py [--calls 300] [--warmup 10] [--out FILE]
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
from lddl_amd.tokenizer import Tokenizer  # noqa: E402

N, S, A, B = 256, 512, 254, 255


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--calls', type=int, default=300)
  ap.add_argument('--warmup', type=int, default=10)
  ap.add_argument('--max-predictions', type=int, default=80)
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda', 0)
  tok = Tokenizer(_lib.VOCAB_BERT, 0)
  L, h = _lib.lib(), tok.handle
  names = tok.ids_to_tokens
  cont = np.asarray([i for i, t in enumerate(names) if t.startswith('##')])
  plain = np.asarray([i for i, t in enumerate(names) if not t.startswith('##') and i > 999])
  rng = np.random.default_rng(7)
  n_ids = N * (A + B)
  ids = np.where(rng.random(n_ids) < 0.3, rng.choice(cont, n_ids), rng.choice(plain, n_ids)).astype(np.uint16)

  def t(x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(dev)
  d_ids = t(np.concatenate([ids, np.zeros(16, np.uint16)]))
  src0 = t(np.arange(N, dtype=np.int64) * (A + B))
  src1 = t(np.arange(N, dtype=np.int64) * (A + B) + A)
  len0, len1 = t(np.full(N, A, np.uint16)), t(np.full(N, B, np.uint16))
  flags = t(np.full(N, 2, np.uint8))
  out = torch.empty((4, N, S), dtype=torch.int64, device=dev)
  nsl = torch.empty(N, dtype=torch.int64, device=dev)
  P = ctypes.c_void_p
  p = lambda x: P(x.data_ptr())  # noqa: E731
  st = P(torch.cuda.current_stream().cuda_stream)
  budget = hasattr(L, 'lddl_set_mask_budget')
  variants = [('token', 0, 0), ('whole_word', 1, 0)]
  if budget:
    variants += [('token_budget', 0, a.max_predictions), ('whole_word_budget', 1, a.max_predictions)]

  def call(word, cap):
    _lib.check(L.lddl_set_whole_word_mask(h, word))
    if budget:
      _lib.check(L.lddl_set_mask_budget(h, cap))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(L.lddl_collate_rows(h, p(d_ids), p(src0), p(src1), p(len0), p(len1), p(flags), P(0), 0, N, N, P(0), P(0),
                                   P(0), P(0), S, 2, -1, 0.15, 7, 3, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(nsl),
                                   st))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3

  us = {name: [] for name, _, _ in variants}
  digest = {}
  for it in range(a.warmup + a.calls):
    for name, word, cap in variants:
      v = call(word, cap)
      if it >= a.warmup:
        us[name].append(v)
      elif it == 0:  # what the variant computes, for comparing two libraries: the labels' count and checksum
        lab = out[3]
        digest[name] = [int((lab != -1).sum()), int((lab * torch.arange(lab.numel(), device=dev).view_as(lab)).sum())]
  report = {'gpu': torch.cuda.get_device_name(0), 'lib': _lib.LIB_PATH, 'rows': N, 'seq_len': S, 'calls': a.calls,
            'max_predictions': a.max_predictions, 'digest': digest, 'us': {}}
  for name, v in us.items():
    q = statistics.quantiles(v, n=4)
    report['us'][name] = {'median': round(statistics.median(v), 2), 'q1': round(q[0], 2), 'q3': round(q[2], 2)}
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
