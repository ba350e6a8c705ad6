"""Measurements of the GPU sentence split (profiles/split_gpu/bench.json).

    python tools/split_bench.py pair [--mb 64] [--out profiles/split_gpu/bench.json]
    python tools/split_bench.py cli  [--mb 256] [--runs 3] [--out ...]

pair  lddl_split_len + lddl_split on a resident buffer, HIP events around the
      pair (its synchronises included), 30 repetitions after 5 warm-ups, on
      Wikipedia-style records (~5 KB) and Books-style records (~512 KB, the
      same text concatenated); yardstick: splitnative.split_raw on the same
      Wikipedia records on one core, its rate times 16.
cli   the bart and bert (seq 512, bin 64) sub-commands on raw synthetic input,
      --split-device host and gpu alternating, wall time and the timing dict.
Results are merged into the output file under the keys 'pair' / 'cli'."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wiki_records(nbytes, seed=1):
  """about nbytes of 'wiki-<i> <text>' records: 4 MB generated, then repeated with new ids"""
  from lddl_amd import synth
  docs = synth.make_wiki(min(nbytes, 4 << 20), seed=seed).documents()
  base = [' '.join(d) for d in docs]
  out, n, i = [], 0, 0
  while n < nbytes:
    r = ('wiki-%d %s' % (i, base[i % len(base)])).encode('utf-8')
    out.append(r)
    n += len(r)
    i += 1
  return out


def books_records(wiki, target=512 << 10):
  out, cur, n = [], [], 0
  for r in wiki:
    cur.append(r)
    n += len(r) + 1
    if n >= target:
      out.append(b' '.join(cur))
      cur, n = [], 0
  if cur:
    out.append(b' '.join(cur))
  return out


def time_pair(tok, raws, mode, reps=30, warm=5):
  import torch
  from lddl_amd import _lib, splitgpu
  from lddl_amd.tokenizer import _ptr
  L = _lib.lib()
  splitgpu.set_props(tok)
  buf, rec_off = splitgpu.join_records(raws)
  n_rec, nbytes = len(raws), int(buf.size)
  d_buf = torch.from_numpy(buf.copy()).cuda()
  d_rec = torch.from_numpy(rec_off).cuda()
  dso = torch.empty(n_rec + 1, dtype=torch.int64, device='cuda')
  id_end = torch.empty(n_rec, dtype=torch.int64, device='cuda')
  tot, bad = (ctypes.c_int64 * 2)(), ctypes.c_int64()
  data = so = None
  ms = []
  for it in range(warm + reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _lib.check(L.lddl_split_len(tok.handle, _ptr(d_buf), nbytes, _ptr(d_rec), n_rec, mode, _ptr(dso), _ptr(id_end), tot,
                                ctypes.byref(bad), None))
    if data is None:
      data = torch.empty(tot[1] + 16, dtype=torch.uint8, device='cuda')
      so = torch.empty(tot[0] + 1, dtype=torch.int64, device='cuda')
    _lib.check(L.lddl_split(tok.handle, _ptr(d_buf), nbytes, _ptr(d_rec), n_rec, mode, _ptr(dso), tot[0], tot[1],
                            _ptr(data), _ptr(so), None))
    e1.record()
    e1.synchronize()
    if it >= warm:
      ms.append(e0.elapsed_time(e1))
  med = statistics.median(ms)
  return {'records': n_rec, 'bytes': nbytes, 'sentences': int(tot[0]), 'out_bytes': int(tot[1]), 'ms_median': med,
          'ms_min': min(ms), 'ms_max': max(ms), 'gb_per_s_median': nbytes / med / 1e6, 'ns_per_byte': med * 1e6 / nbytes}


def run_pair(mb):
  from lddl_amd import splitnative
  from lddl_amd.tokenizer import Tokenizer
  wiki = wiki_records(mb << 20)
  books = books_records(wiki)
  t0 = time.perf_counter()
  got = splitnative.split_raw(wiki)
  host_s = time.perf_counter() - t0
  assert got is not None
  nb = sum(map(len, wiki))
  tok = Tokenizer()
  res = {'wiki': time_pair(tok, wiki, 0), 'books': time_pair(tok, books, 0),
         'host_one_core': {'bytes': nb, 's': host_s, 'mb_per_s': nb / host_s / 1e6},
         'yardstick_ms': host_s / 16 * 1e3}
  res['wiki_within_yardstick'] = res['wiki']['ms_median'] <= res['yardstick_ms']
  res['books_over_wiki_per_byte'] = res['books']['ns_per_byte'] / res['wiki']['ns_per_byte']
  tok.close()
  return res


def run_cli(mb, runs):
  wiki = wiki_records(mb << 20, seed=2)
  res = {}
  with tempfile.TemporaryDirectory() as d:
    src = os.path.join(d, 'wiki', 'en')
    os.makedirs(src)
    for k in range(8):
      with open(os.path.join(src, 'w%d.txt' % k), 'wb') as f:
        for r in wiki[k::8]:
          f.write(r + b'\n')
    cmds = {'bart': ['bart', '--target-seq-length', '128'],
            'bert': ['--target-seq-length', '512', '--bin-size', '64']}
    for name, extra in cmds.items():
      res[name] = {'host': [], 'gpu': []}
      for i in range(runs):
        for dev in ('host', 'gpu'):
          sink = os.path.join(d, 'out_%s_%s_%d' % (name, dev, i))
          t0 = time.perf_counter()
          r = subprocess.run([sys.executable, '-m', 'lddl_amd.preprocess'] + extra +
                             ['--wikipedia', os.path.join(d, 'wiki'), '--sink', sink, '--sentence-splitter', 'rules',
                              '--split-device', dev], cwd=ROOT, capture_output=True, text=True)
          wall = time.perf_counter() - t0
          assert r.returncode == 0, r.stderr[-2000:]
          line = [l for l in r.stdout.splitlines() if l.startswith('rank 0:')][0]
          res[name][dev].append({'wall_s': wall, 'timings': line})
          print('%s %s run %d: %.2f s' % (name, dev, i, wall), file=sys.stderr, flush=True)
          subprocess.run(['rm', '-rf', sink])
      for dev in ('host', 'gpu'):
        w = [x['wall_s'] for x in res[name][dev]]
        res[name][dev + '_wall_median'], res[name][dev + '_wall_range'] = statistics.median(w), [min(w), max(w)]
  return res


if __name__ == '__main__':
  ap = argparse.ArgumentParser()
  ap.add_argument('what', choices=['pair', 'cli'])
  ap.add_argument('--mb', type=int, default=None)
  ap.add_argument('--runs', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_gpu', 'bench.json'))
  a = ap.parse_args()
  res = run_pair(a.mb or 64) if a.what == 'pair' else run_cli(a.mb or 256, a.runs)
  os.makedirs(os.path.dirname(a.out), exist_ok=True)
  allres = {}
  if os.path.exists(a.out):
    with open(a.out) as f:
      allres = json.load(f)
  allres[a.what] = res
  with open(a.out, 'w') as f:
    json.dump(allres, f, indent=1, sort_keys=True)
  print(json.dumps(res if a.what == 'pair' else {k: {x: v[x] for x in v if 'median' in x or 'range' in x}
                                                  for k, v in res.items()}))
