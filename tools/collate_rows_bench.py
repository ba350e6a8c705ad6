"""Time the two ways from a pack result to a training batch, on the GPU.

  new:  lddl_collate_rows mode 2 over a row-index list (spans of the dense ids)
  old:  lddl_collate_bert mode 2 over the same rows' rendered A / B strings

for one batch of 256 rows and one of 8 192 rows drawn (seeded) from one
seq-512 / bin-64 pack result of a synthetic corpus.  Per batch size:

* the C calls alone, between HIP events on the stream, inputs already on the
  device (each call includes its 4-byte error-word read-back; the fill calls
  launch one kernel each: collate_rows_kernel / collate_fill_kernel);
* the length passes alone (lddl_collate_rows_seq_len / lddl_collate_seq_len);
* end to end on the host clock with a device synchronise:
  BertCollate.collate_rows(res, idx) against string render on the device +
  copy to the host + pinned staging + H2D + lddl_collate_seq_len +
  lddl_collate_bert (BertCollate's own path; no parquet encode / decode, which
  the file route pays on top).

Output bandwidth = n_rows * seq_len * 40 B / time (five int64 outputs counted
per column, the project's usual figure) and its share of the 8 TB/s HBM peak;
stored_TBps counts what is really stored: the four [n_rows, seq_len] tensors
(32 B per column) and n_rows * 8 B of next_sentence_labels.  Prints one
JSON document; --out writes it to a file as well.

    python tools/collate_rows_bench.py [--mb 10] [--reps 30] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lddl_amd import _lib, pipeline, synth, writer  # noqa: E402
from lddl_amd.loader import BertCollate  # noqa: E402

PEAK = 8.0e12


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


def wall(fn, warmup, reps):
  for _ in range(warmup):
    fn()
  ms = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t) * 1e3)
  return ms


def stats(ms, nbytes=None, stored=None):
  q = statistics.quantiles(ms, n=4)
  d = {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
       'q1_ms': round(q[0], 4), 'q3_ms': round(q[2], 4), 'reps': len(ms)}
  if nbytes:
    bw = nbytes / (d['median_ms'] * 1e-3)
    d['out_TBps'] = round(bw / 1e12, 3)
    d['share_of_8TBps'] = round(bw / PEAK, 3)
    d['stored_TBps'] = round(stored / (d['median_ms'] * 1e-3) / 1e12, 3)
  return d


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--mb', type=float, default=10.0, help='synthetic corpus size')
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--sizes', type=int, nargs='+', default=[256, 8192])
  ap.add_argument('--whole-word', action='store_true', help='whole-word masking on (lddl_set_whole_word_mask): both routes')
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
  col = BertCollate(tokenizer=pk.tok, sequence_length_alignment=8, base_seed=7, whole_word_mask=a.whole_word)
  L = _lib.lib()
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  h = pk.tok.handle
  report = {'gpu': torch.cuda.get_device_name(0), 'n_pairs': res.n_pairs, 'corpus_mb': a.mb, 'seq': 512, 'bin': 64,
            'whole_word': a.whole_word, 'batches': {}}
  for n in a.sizes:
    assert res.n_pairs >= n, 'corpus too small: %d rows' % res.n_pairs
    idx = torch.from_numpy(np.random.default_rng(n).permutation(res.n_pairs)[:n]).to(dev)
    st = P(torch.cuda.current_stream().cuda_stream)
    seq = ctypes.c_int64()
    _lib.check(L.lddl_collate_rows_seq_len(h, p(res.len0), p(res.len1), p(idx), 0, n, res.n_pairs, 8,
                                           ctypes.byref(seq), st))
    S = seq.value
    out = torch.empty((4, n, S), dtype=torch.int64, device=dev)
    nsl = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = n * S * 40
    stored = n * S * 32 + n * 8

    def new_len():
      _lib.check(L.lddl_collate_rows_seq_len(h, p(res.len0), p(res.len1), p(idx), 0, n, res.n_pairs, 8,
                                             ctypes.byref(seq), st))

    def new_fill():
      _lib.check(L.lddl_collate_rows(h, p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1), p(res.flags),
                                     p(idx), 0, n, res.n_pairs, P(0), P(0), P(0), P(0), S, 2, -1, 0.15, 7, 3,
                                     p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(nsl), st))

    # the same rows as device string columns (what the parquet files would hold)
    s0, s1 = res.src0[idx].contiguous(), res.src1[idx].contiguous()
    l0, l1 = res.len0[idx].contiguous(), res.len1[idx].contiguous()
    rn = (res.flags[idx] & 1).contiguous()

    def render_dev():
      return (writer.render(pk, res.ids, s0, 0, n, writer.SPAN, len0=l0, host=False),
              writer.render(pk, res.ids, s1, 0, n, writer.SPAN, len0=l1, host=False))

    (a_off, a_dat), (b_off, b_dat) = render_dev()
    a_dat, b_dat = a_dat.clone(), b_dat.clone()
    seq2 = ctypes.c_int64()

    def old_len():
      _lib.check(L.lddl_collate_seq_len(h, p(a_dat), p(a_off), p(b_dat), p(b_off), n, 8, ctypes.byref(seq2), st))

    old_len()
    assert seq2.value == S, (seq2.value, S)
    out2 = torch.empty((4, n, S), dtype=torch.int64, device=dev)
    nsl2 = torch.empty(n, dtype=torch.int64, device=dev)

    def old_fill():
      _lib.check(L.lddl_collate_bert(h, p(a_dat), p(a_off), p(b_dat), p(b_off), p(rn), P(0), P(0), P(0), P(0), n, S,
                                     2, -1, 0.15, 7, 3, p(out2[0]), p(out2[1]), p(out2[2]), p(out2[3]), p(nsl2), st))

    new_fill()
    old_fill()
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(nsl, nsl2), 'the two routes differ'

    def new_e2e():
      col.collate_rows(res, idx)

    def old_e2e():
      (ao, ad), (bo, bd) = render_dev()
      cols = [(writer._host(ad), writer._host(ao)), (writer._host(bd), writer._host(bo))]
      col._run(cols, rn.cpu().numpy(), False)

    r = {'seq_len': S, 'out_bytes': nbytes, 'stored_bytes': stored}
    # alternate the two routes so that drift of the shared host hits both
    half = max(a.reps // 2, 10)
    nf, of = [], []
    for _ in range(2):
      nf += events(new_fill, a.warmup, half)
      of += events(old_fill, a.warmup, half)
    r['new_fill_call'] = stats(nf, nbytes, stored)
    r['old_fill_call'] = stats(of, nbytes, stored)
    r['new_len_call'] = stats(events(new_len, a.warmup, a.reps))
    r['old_len_call'] = stats(events(old_len, a.warmup, a.reps))
    r['new_end_to_end'] = stats(wall(new_e2e, 3, a.reps), nbytes, stored)
    r['old_render_stage_collate'] = stats(wall(old_e2e, 3, a.reps), nbytes, stored)
    report['batches'][str(n)] = r
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
