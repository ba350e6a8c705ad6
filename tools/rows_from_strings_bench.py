"""Time the load of a shard's string columns into a GPU row table against the
per-batch string collate it replaces, on the GPU.

  (a) load:    lddl_rows_from_strings_len + lddl_rows_from_strings over the
               rows' A / B strings (once per shard)
  (b) strings: lddl_collate_seq_len + lddl_collate_bert mode 2 over the same
               strings (once per batch per epoch: what collate_arrow calls)
  (c) rows:    lddl_collate_rows_seq_len + lddl_collate_rows mode 2 over the
               loaded table (once per batch per epoch after the load)

for 256 rows and for 8 192 rows drawn (seeded) from one seq-512 / bin-64 pack
result of a synthetic corpus, whose strings are rendered on the device as
tools/collate_rows_bench.py does.  Each pair of C calls runs between HIP
events on the stream, inputs already on the device; the three routes take
turns within every repetition so that drift of the shared host hits all of
them.  The same run asserts that (b) and (c) give equal tensors.

break_even: the number of collated batches of 256 rows after which loading
once and collating from the table is cheaper than collating from the strings
every time, N > load / (strings - rows); from the device calls alone, and on
the host clock with the staging included (load_rows against collate_arrow
and collate_rows over an Arrow table of the same rows).

Prints one JSON document; --out writes it to a file as well.

    python tools/rows_from_strings_bench.py [--mb 10] [--reps 30] [--out FILE]
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


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def wall(fn):
  torch.cuda.synchronize()
  t = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e3


def stats(ms):
  return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
          'reps': len(ms)}


def turns(fns, warmup, reps, clock):
  """{name: [ms]}: every repetition runs each route once, in turn"""
  for _ in range(warmup):
    for fn in fns.values():
      fn()
  out = {k: [] for k in fns}
  for _ in range(reps):
    for k, fn in fns.items():
      out[k].append(clock(fn))
  return out


def break_even(load, strings, rows):
  gain = strings - rows
  return round(load / gain, 2) if gain > 0 else None


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--mb', type=float, default=10.0, help='synthetic corpus size')
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--sizes', type=int, nargs='+', default=[256, 8192])
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  import pyarrow as pa
  dev = torch.device('cuda', 0)
  c = synth.make_wiki(int(a.mb * 1e6), seed=512)
  pk = pipeline.Packer(_lib.VOCAB_BERT, 0)
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 4), dev)
  res = pk.run(sh, target_seq_length=512, bin_size=64, duplicate_factor=2, seed=1, spans=True)
  torch.cuda.synchronize()
  col = BertCollate(tokenizer=pk.tok, sequence_length_alignment=8, base_seed=7)
  L = _lib.lib()
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  h = pk.tok.handle
  report = {'gpu': torch.cuda.get_device_name(0), 'n_pairs': res.n_pairs, 'corpus_mb': a.mb, 'seq': 512, 'bin': 64,
            'mode': 2, 'batches': {}}
  for n in a.sizes:
    assert res.n_pairs >= n, 'corpus too small: %d rows' % res.n_pairs
    idx = torch.from_numpy(np.random.default_rng(n).permutation(res.n_pairs)[:n]).to(dev)
    st = P(torch.cuda.current_stream().cuda_stream)
    # the rows as device string columns (what the parquet files hold)
    s0, s1 = res.src0[idx].contiguous(), res.src1[idx].contiguous()
    l0, l1 = res.len0[idx].contiguous(), res.len1[idx].contiguous()
    rn = (res.flags[idx] & 1).contiguous()
    a_off, a_dat = writer.render(pk, res.ids, s0, 0, n, writer.SPAN, len0=l0, host=False)
    a_off, a_dat = a_off.clone(), a_dat.clone()
    b_off, b_dat = writer.render(pk, res.ids, s1, 0, n, writer.SPAN, len0=l1, host=False)
    b_off, b_dat = b_off.clone(), b_dat.clone()
    strings = [p(a_dat), p(a_off), p(b_dat), p(b_off)]

    # (a) the load
    t_len0, t_len1 = (torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2))
    t_src0, t_src1 = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    t_tok = torch.empty(n + 1, dtype=torch.int64, device=dev)
    t_flags = torch.empty(n, dtype=torch.uint8, device=dev)
    tot = (ctypes.c_int64 * 3)()

    def load_len():
      _lib.check(L.lddl_rows_from_strings_len(h, *strings, P(0), P(0), P(0), P(0), n, p(t_len0), p(t_len1), p(t_src0),
                                              p(t_src1), p(t_tok), P(0), tot, st))

    load_len()
    n_ids = int(tot[0])
    t_ids = torch.zeros(n_ids + 16, dtype=torch.int16, device=dev)

    def load():
      load_len()
      _lib.check(L.lddl_rows_from_strings(h, *strings, P(0), P(0), P(0), P(0), p(rn), n, p(t_len0), p(t_len1), p(t_src0),
                                          p(t_src1), P(0), p(t_ids), n_ids, p(t_flags), P(0), P(0), P(0), 0, st))

    load()
    assert torch.equal(t_len0, l0) and torch.equal(t_len1, l1) and int(tot[2]) == int(t_tok[-1])

    # (b) the string collate, (c) the collate from the loaded table
    seq_b, seq_c = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(L.lddl_collate_seq_len(h, *strings, n, 8, ctypes.byref(seq_b), st))
    S = seq_b.value
    out_b = torch.empty((4, n, S), dtype=torch.int64, device=dev)
    out_c = torch.empty((4, n, S), dtype=torch.int64, device=dev)
    nsl_b, nsl_c = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))

    def from_strings():
      _lib.check(L.lddl_collate_seq_len(h, *strings, n, 8, ctypes.byref(seq_b), st))
      _lib.check(L.lddl_collate_bert(h, *strings, p(rn), P(0), P(0), P(0), P(0), n, S, 2, -1, 0.15, 7, 3, p(out_b[0]),
                                     p(out_b[1]), p(out_b[2]), p(out_b[3]), p(nsl_b), st))

    def from_rows():
      _lib.check(L.lddl_collate_rows_seq_len(h, p(t_len0), p(t_len1), P(0), 0, n, n, 8, ctypes.byref(seq_c), st))
      _lib.check(L.lddl_collate_rows(h, p(t_ids), p(t_src0), p(t_src1), p(t_len0), p(t_len1), p(t_flags), P(0), 0, n, n,
                                     P(0), P(0), P(0), P(0), S, 2, -1, 0.15, 7, 3, p(out_c[0]), p(out_c[1]),
                                     p(out_c[2]), p(out_c[3]), p(nsl_c), st))

    from_strings()
    from_rows()
    torch.cuda.synchronize()
    assert seq_b.value == seq_c.value == S
    assert torch.equal(out_b, out_c) and torch.equal(nsl_b, nsl_c), 'the string route and the table route differ'

    ms = turns({'load': load, 'strings': from_strings, 'rows': from_rows}, a.warmup, a.reps, timed)
    r = {'seq_len': S, 'ids': n_ids, 'string_bytes': int(a_dat.numel() + b_dat.numel()),
         'a_load_len_plus_fill': stats(ms['load']), 'b_collate_seq_len_plus_bert': stats(ms['strings']),
         'c_collate_rows_seq_len_plus_rows': stats(ms['rows']), 'equal_b_c': True}
    r['a_le_b'] = bool(r['a_load_len_plus_fill']['median_ms'] <= r['b_collate_seq_len_plus_bert']['median_ms'] or
                       r['a_load_len_plus_fill']['min_ms'] <= r['b_collate_seq_len_plus_bert']['max_ms'])

    # the same on the host clock, staging included: an Arrow table of the rows
    A = writer._host(a_dat).tobytes()
    B = writer._host(b_dat).tobytes()
    ao, bo = writer._host(a_off), writer._host(b_off)
    table = pa.table({'A': [A[ao[i]:ao[i + 1]].decode() for i in range(n)],
                      'B': [B[bo[i]:bo[i + 1]].decode() for i in range(n)],
                      'is_random_next': rn.cpu().numpy().astype(bool)})
    tab = col.load_rows(table)
    hs = turns({'load': lambda: col.load_rows(table), 'strings': lambda: col.collate_arrow(table),
                'rows': lambda: col.collate_rows(tab)}, 3, a.reps, wall)
    r['host_clock'] = {'load_rows': stats(hs['load']), 'collate_arrow': stats(hs['strings']),
                       'collate_rows': stats(hs['rows'])}
    report['batches'][str(n)] = r
  b256 = report['batches'].get('256')
  if b256:
    med = lambda d: d['median_ms']  # noqa: E731
    report['break_even_batches_of_256'] = {
        'device_calls': break_even(med(b256['a_load_len_plus_fill']), med(b256['b_collate_seq_len_plus_bert']),
                                   med(b256['c_collate_rows_seq_len_plus_rows'])),
        'host_clock': break_even(med(b256['host_clock']['load_rows']), med(b256['host_clock']['collate_arrow']),
                                 med(b256['host_clock']['collate_rows']))}
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
