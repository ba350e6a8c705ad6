"""Time the BART sentence aggregation on the GPU: lddl_bart_count,
lddl_bart_plan_len + lddl_bart_plan, and lddl_bart_render of every chunk, on
synth's Wikipedia-style corpus tiled on the device as bench.py tiles it.

Each C call (its synchronises included) runs between HIP events on the
stream, inputs already on the device; --reps repetitions, median and min-max.
The count is set against two yardsticks on the same box and corpus: the
tokenizer's `tok5::scan_kernel` (lddl_tokenize with lddl_set_timing, the
kernel's own events), which does strictly more per byte, and the 8 TB/s HBM
roofline (the count reads every corpus byte once and the offsets).

Also recorded: the CPU rate of the same rule (str.split() counts + the walk,
tests/bart_model.py's arithmetic) on the box's CPU share, and the host
sentence splitter's rate on whole lines, measured on one core over 4 MB (the
stage that dominates the CLI's wall time, its host_split_s; the figure for
the whole corpus on the CPU share is an extrapolation from that rate and is
named so; no end-to-end speed-up is claimed from the GPU stage).

Prints one JSON document; --out writes it to a file as well, and beside it
resource_usage.txt: the compiler's report (VGPRs, LDS, scratch, waves per
SIMD per kernel) of lddl_amd/csrc/bart.hip, compiled again with the build's
flags, so the two files come from the same tree.

    python tools/bart_bench.py [--gb 4] [--unique-mb 64] [--reps 30] [--out profiles/bart/bench.json]
"""
import argparse
import concurrent.futures
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

from lddl_amd import _lib, bart, synth  # noqa: E402
from lddl_amd.hostinfo import cpu_share  # noqa: E402
from lddl_amd.pipeline import ShardSet, partition_by_bytes  # noqa: E402
from lddl_amd.tokenizer import Tokenizer  # noqa: E402

HBM_GBS = 8000.0


def timed(fn):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def stats(ms):
  return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
          'reps': len(ms)}


def tiled(base, reps, device, n_part):
  """the base corpus `reps` times back to back on the device (every tile its own documents)"""
  nb, ns, nd = base.nbytes, base.n_sent, base.n_doc
  data = torch.empty(nb * reps + 16, dtype=torch.uint8, device=device)
  src = torch.from_numpy(base.data[:nb]).to(device)
  for r in range(reps):
    data[r * nb:(r + 1) * nb].copy_(src)
  data[nb * reps:].zero_()
  so = torch.from_numpy(base.sent_off - base.sent_off[0]).to(device)
  dso = torch.from_numpy(base.doc_sent_off).to(device)
  pdo = partition_by_bytes(base, n_part)
  pd = torch.from_numpy(pdo).to(device)
  npb = len(pdo) - 1
  sent_off = torch.empty(ns * reps + 1, dtype=torch.int64, device=device)
  doc_sent_off = torch.empty(nd * reps + 1, dtype=torch.int64, device=device)
  part_doc_off = torch.empty(npb * reps + 1, dtype=torch.int64, device=device)
  for r in range(reps):
    sent_off[r * ns:(r + 1) * ns + 1] = so + r * nb
    doc_sent_off[r * nd:(r + 1) * nd + 1] = dso + r * ns
    part_doc_off[r * npb:(r + 1) * npb + 1] = pd + r * nd
  return ShardSet(data, sent_off, doc_sent_off, part_doc_off, None, nb * reps)


def _cpu_piece(a):
  """count + walk of documents [d0, d1) of the base corpus on one core: (bytes, seconds)"""
  data, so, dso, T = a
  t0 = time.perf_counter()
  raw = data.tobytes()
  base = int(so[0])
  nw = [len(raw[int(x) - base:int(y) - base].decode('utf-8').split()) for x, y in zip(so[:-1], so[1:])]
  chunks = 0
  for d in range(len(dso) - 1):
    cnt = 0
    for s in range(int(dso[d] - dso[0]), int(dso[d + 1] - dso[0])):
      cnt += nw[s]
      if cnt >= T:
        chunks += 1
        cnt = 0
    chunks += cnt > 0
  return len(raw), time.perf_counter() - t0, chunks


def cpu_rate(base, T, procs, mb):
  """GB/s of the rule on `procs` processes over the first `mb` MB of the base corpus"""
  nd = int(np.searchsorted(base.sent_off[base.doc_sent_off], mb * 1e6))
  nd = max(procs, min(nd, base.n_doc))
  cuts = np.linspace(0, nd, procs + 1).astype(np.int64)
  work = []
  for a, b in zip(cuts[:-1], cuts[1:]):
    s0, s1 = int(base.doc_sent_off[a]), int(base.doc_sent_off[b])
    so = base.sent_off[s0:s1 + 1]
    work.append((base.data[int(so[0]):int(so[-1])], so, base.doc_sent_off[a:b + 1], T))
  with concurrent.futures.ProcessPoolExecutor(procs) as ex:
    list(ex.map(_cpu_piece, work[:procs]))  # warm the workers
    t0 = time.perf_counter()
    got = list(ex.map(_cpu_piece, work))
    wall = time.perf_counter() - t0
  nbytes = sum(g[0] for g in got)
  return {'procs': procs, 'bytes': nbytes, 'wall_s': round(wall, 4), 'gb_per_s': round(nbytes / wall / 1e9, 4),
          'chunks': int(sum(g[2] for g in got))}


def host_split_rate(base, mb):
  """seconds per GB of the rule-based splitter on whole lines (one core): documents of the base corpus joined
  back into lines and split as the CLI's workers split them"""
  from lddl_amd import preprocess
  lines, nb = [], 0
  for d in range(base.n_doc):
    line = 'doc%d ' % d + ' '.join(base.sentence(s) for s in range(base.doc_sent_off[d], base.doc_sent_off[d + 1]))
    lines.append(line)
    nb += len(line)
    if nb >= mb * 1e6:
      break
  t0 = time.perf_counter()
  preprocess.split_records(lines, False, preprocess._rule_split, True)
  dt = time.perf_counter() - t0
  return {'bytes': nb, 'seconds': round(dt, 4), 'host_split_s_per_gb_one_core': round(dt / nb * 1e9, 2)}


def resource_usage(path):
  """-Rpass-analysis=kernel-resource-usage of bart.hip with lddl_amd/build.py's flags -> path"""
  import re
  import subprocess
  import tempfile
  from lddl_amd import build
  src = os.path.join(build.CSRC, 'bart.hip')
  with tempfile.TemporaryDirectory() as d:
    cmd = [os.environ.get('LDDL_HIPCC', 'hipcc'), '--offload-arch=%s' % build.ARCH, '-O3', '-std=c++17', '-fPIC',
           '-Wno-unused-result', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.path.join(d, 'bart.o'), src]
    r = subprocess.run(cmd, check=True, cwd=build.CSRC, capture_output=True, text=True)
  lines = ['# hipcc --offload-arch=%s -O3 -Rpass-analysis=kernel-resource-usage, lddl_amd/csrc/bart.hip' % build.ARCH]
  for ln in r.stderr.splitlines():
    m = re.search(r'remark: (?:[^ ]+ )?(.*?) \[-Rpass-analysis=kernel-resource-usage\]$', ln)
    if not m:
      continue
    t = m.group(1).strip()
    if t.startswith(('Function Name:', 'Name:')):
      lines.append('Function Name: ' + t.split(':', 1)[1].strip())
    elif t.split(':')[0].split(' [')[0] in ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS Size'):
      lines.append('   ' + t)
  assert sum(l.startswith('Function Name') for l in lines) >= 5, r.stderr[-2000:]
  with open(path, 'w') as f:
    f.write('\n'.join(lines) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gb', type=float, default=4.0, help='corpus GiB on the device')
  ap.add_argument('--unique-mb', type=int, default=64)
  ap.add_argument('--reps', type=int, default=30)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--target-seq-length', type=int, default=128)
  ap.add_argument('--cpu-mb', type=float, default=32.0)
  ap.add_argument('--out')
  a = ap.parse_args()
  assert torch.cuda.is_available(), 'needs a GPU'
  dev = torch.device('cuda', 0)
  base = synth.make_wiki(a.unique_mb << 20, seed=20261015)
  # the host baselines first: their worker processes fork before the GPU is touched
  cpu = cpu_rate(base, a.target_seq_length - 3, cpu_share(), a.cpu_mb)
  split = host_split_rate(base, 4.0)
  reps = max(1, int(round(a.gb * (1 << 30) / base.nbytes)))
  sh = tiled(base, reps, dev, 64)
  tok = Tokenizer(device=0)
  L, h = _lib.lib(), tok.handle
  P = ctypes.c_void_p
  p = lambda t: P(t.data_ptr())  # noqa: E731
  st = P(torch.cuda.current_stream().cuda_stream)
  n_sent, n_doc, tsl = sh.n_sent, sh.n_doc, a.target_seq_length
  res = bart.aggregate(sh, None, tsl, tok)
  nc = res.n_chunks
  nwords = torch.empty(n_sent, dtype=torch.int32, device=dev)
  dco = torch.empty(n_doc + 1, dtype=torch.int64, device=dev)
  tot = (ctypes.c_int64 * 2)()
  sent0 = torch.empty(nc, dtype=torch.int64, device=dev)
  nsent, ntok = (torch.empty(nc, dtype=torch.int32, device=dev) for _ in range(2))
  coff = torch.empty(nc + 1, dtype=torch.int64, device=dev)
  out_off = torch.empty(nc + 1, dtype=torch.int64, device=dev)
  out = torch.empty(res.nbytes, dtype=torch.uint8, device=dev)
  nb = ctypes.c_int64(0)

  def count():
    _lib.check(L.lddl_bart_count(h, p(sh.data), sh.nbytes, p(sh.sent_off), n_sent, p(nwords), st))

  def plan():
    _lib.check(L.lddl_bart_plan_len(h, p(nwords), p(sh.sent_off), p(sh.doc_sent_off), n_doc, n_sent, tsl, p(dco), tot,
                                    st))
    _lib.check(L.lddl_bart_plan(h, p(nwords), p(sh.sent_off), p(sh.doc_sent_off), p(dco), n_doc, n_sent, tsl, nc,
                                p(sent0), p(nsent), p(ntok), p(coff), st))

  def render():
    _lib.check(L.lddl_bart_render(h, p(sh.data), sh.nbytes, p(sh.sent_off), n_sent, p(sent0), p(nsent), p(coff), nc, 0,
                                  nc, p(out_off), p(out), res.nbytes, ctypes.byref(nb), st))

  fns = {'count': count, 'plan': plan, 'render': render}
  for _ in range(a.warmup):
    for fn in fns.values():
      fn()
  assert torch.equal(nwords, res.nwords) and torch.equal(coff, res.chunk_off) and nb.value == res.nbytes
  ms = {k: [] for k in fns}
  for _ in range(a.reps):
    for k, fn in fns.items():
      ms[k].append(timed(fn))
  # the yardstick: the tokenizer's scan over the same corpus on the same box
  tok.set_timing(True)
  ids = torch.empty(sh.nbytes + 16, dtype=torch.int16, device=dev)
  o_ntok = torch.empty(n_sent, dtype=torch.int32, device=dev)
  o_off = torch.empty(n_sent + 1, dtype=torch.int64, device=dev)
  scan = []
  for i in range(2 + max(5, a.reps // 3)):
    tok.tokenize_device(sh.data, sh.sent_off, 512, ids, o_ntok, o_off, nbytes=sh.nbytes)
    if i >= 2:
      scan.append(tok.stats()['scan_ms'])
  tok.set_timing(False)
  gb = sh.nbytes / 1e9
  c, s = stats(ms['count']), stats(scan)
  read_bytes = sh.nbytes + 8 * (n_sent + 1) + 4 * n_sent
  report = {
      'gpu': torch.cuda.get_device_name(0), 'corpus': 'synth.make_wiki %d MB x %d' % (a.unique_mb, reps),
      'corpus_bytes': sh.nbytes, 'sentences': n_sent, 'documents': n_doc, 'target_seq_length': tsl, 'chunks': nc,
      'column_bytes': res.nbytes,
      'count': dict(c, gb_per_s=round(gb / c['median_ms'] * 1e3, 1), ms_per_gb=round(c['median_ms'] / gb, 4),
                    hbm_roofline_ms=round(read_bytes / HBM_GBS / 1e6, 4),
                    fraction_of_roofline=round(read_bytes / HBM_GBS / 1e6 / c['median_ms'], 4)),
      'plan_len_plus_fill': stats(ms['plan']),
      'render_all_chunks': dict(stats(ms['render']),
                                gb_per_s_written=round(res.nbytes / 1e9 / statistics.median(ms['render']) * 1e3, 1)),
      'yardstick_tok5_scan_kernel': dict(s, ms_per_gb=round(s['median_ms'] / gb, 4)),
      'cpu_model': cpu, 'host_split_rules_whole_lines': split,
  }
  report['count_le_scan'] = bool(c['median_ms'] <= s['median_ms'] or c['min_ms'] <= s['max_ms'])
  # not measured: the one-core rate above times the corpus, divided by the CPU share
  report['host_split_s_extrapolated_to_this_corpus_on_cpu_share'] = round(
      split['host_split_s_per_gb_one_core'] * gb / cpu['procs'], 2)
  text = json.dumps(report, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
      f.write(text + '\n')
    resource_usage(os.path.join(os.path.dirname(os.path.abspath(a.out)), 'resource_usage.txt'))


if __name__ == '__main__':
  main()
