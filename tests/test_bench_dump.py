"""bench.py --dump-outputs: the last timed step's outputs as .npy files
(float32 / float64, fixed seeded samples, whole-array checksums), and a plain
run's line against --full's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_result(n_sent=5000, n=3000, seed=0):
  import torch
  from lddl_amd.pipeline import PackResult
  r = np.random.RandomState(seed)
  ntok = torch.from_numpy(r.randint(0, 40, n_sent).astype(np.int32))
  n_tok = int(ntok.sum())
  ids = torch.from_numpy(r.randint(0, 65536, n_tok + 16).astype(np.uint16).view(np.int16))
  l0 = r.randint(1, 60000, n).astype(np.uint16)
  l1 = r.randint(0, 200, n).astype(np.uint16)
  off = np.concatenate([[0], np.cumsum(l0.astype(np.int64) + l1 + 3)])
  res = PackResult(n, int(off[-1]), 4, None, torch.from_numpy(off), torch.from_numpy(l0.view(np.int16)),
                   torch.from_numpy(l1.view(np.int16)), torch.from_numpy(r.randint(0, 4, n).astype(np.uint8)),
                   torch.from_numpy(r.randint(0, 4, n).astype(np.uint8)),
                   torch.from_numpy(np.sort(r.randint(0, 7, n)).astype(np.int64)),
                   torch.from_numpy(r.randint(0, 100, (7, 4)).astype(np.int64)))
  res.ids, res.ntok = ids, ntok
  res.src0 = torch.from_numpy(r.randint(0, n_tok, n).astype(np.int64) + (1 << 33))  # (past float32 and int32)
  res.src1 = torch.from_numpy(r.randint(0, n_tok, n).astype(np.int64))
  return res, ntok, n_sent, n_tok


def test_dump_outputs_small_arrays_whole(tmp_path):
  import bench
  res, ntok, n_sent, n_tok = _fake_result()
  info = bench.dump_outputs(str(tmp_path / 'd'), res, ntok, n_sent, n_tok)
  got = {f[:-4]: np.load(tmp_path / 'd' / f) for f in os.listdir(tmp_path / 'd')}
  assert info['arrays'] == len(got) and info['bytes'] == sum(a.nbytes for a in got.values())
  assert all(a.dtype in (np.float32, np.float64) for a in got.values())
  # below the sample sizes every array is written whole, with its values
  assert np.array_equal(got['ntok'], ntok.numpy())
  assert np.array_equal(got['ids'], res.ids[:n_tok].numpy().view(np.uint16))
  assert np.array_equal(got['len0'], res.len0.numpy().view(np.uint16))
  assert np.array_equal(got['src0'], res.src0.numpy()) and got['src0'].dtype == np.float64
  assert np.array_equal(got['tok_off'], res.tok_off.numpy()[:-1])
  assert np.array_equal(got['bin_count'], res.bin_count.numpy())
  assert got['totals'].tolist() == [n_sent, n_tok, res.n_pairs, res.n_tokens, 0, 4]
  names = [bytes(row.astype(np.uint8)).rstrip(b'\0').decode() for row in got['checksum_names']]
  sums = dict(zip(names, got['checksums']))
  assert sums['src0'] == int(res.src0.numpy().sum()) % (1 << 32)
  assert sums['tok_off'] == int(res.tok_off.numpy().sum()) % (1 << 32)
  assert sums['ids'] == int(res.ids[:n_tok].numpy().astype(np.int64).sum()) % (1 << 32)
  assert 'tokens' not in got and 'mlm_off' not in got


def test_dump_outputs_samples_are_fixed_and_see_changes(tmp_path, monkeypatch):
  import bench
  monkeypatch.setattr(bench, 'DUMP_ROWS', 256)
  monkeypatch.setattr(bench, 'DUMP_TOKENS', 512)
  monkeypatch.setattr(bench, 'DUMP_SENTS', 128)
  a = _fake_result()
  b = _fake_result()
  b[0].flags[1234] ^= 1  # one entry of one column differs
  bench.dump_outputs(str(tmp_path / 'a'), *a)
  bench.dump_outputs(str(tmp_path / 'a2'), *a)
  bench.dump_outputs(str(tmp_path / 'b'), *b)
  files = sorted(os.listdir(tmp_path / 'a'))
  assert files == sorted(os.listdir(tmp_path / 'b'))
  for f in files:
    assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'a2' / f)), f
  rows = np.load(tmp_path / 'a' / 'sampled_rows.npy').astype(np.int64)
  assert len(rows) == 256 and (np.diff(rows) >= 0).all() and rows[-1] < a[0].n_pairs
  assert np.array_equal(np.load(tmp_path / 'a' / 'part.npy'), a[0].part.numpy()[rows])
  assert len(np.load(tmp_path / 'a' / 'ids.npy')) == 512 and len(np.load(tmp_path / 'a' / 'ntok.npy')) == 128
  # the checksum covers the entries the sample leaves out
  assert not np.array_equal(np.load(tmp_path / 'a' / 'checksums.npy'), np.load(tmp_path / 'b' / 'checksums.npy'))


def test_dump_outputs_refuses_more_than_its_budget(tmp_path, monkeypatch):
  import bench
  monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 1000)
  with pytest.raises(RuntimeError):
    bench.dump_outputs(str(tmp_path / 'd'), *_fake_result())
  assert not os.path.exists(tmp_path / 'd' / 'ids.npy')


def test_default_sample_sizes_fit_64_mb():
  import bench
  # the largest case: masking with materialised rows, every sample full
  f64 = 8 * (bench.DUMP_ROWS * 5 + 20412 * 8 + 64)          # sampled_rows, tok_off, part, mlm_off + slack; bin_count
  f32 = 4 * (bench.DUMP_ROWS * 4 + bench.DUMP_SENTS + 2 * bench.DUMP_TOKENS + 3 * bench.DUMP_MASKED)
  assert f64 + f32 <= 64 << 20 == bench.DUMP_MAX_BYTES


@pytest.mark.gpu
def test_plain_run_and_dump_on_gpu(gpu, tmp_path):
  """a small plain run: the line's headline fields, --steps timed steps, the
  dump; the same arguments again give the same arrays"""
  def run(d):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                        '--corpus-gb', '0.03', '--unique-mb', '8', '--dump-outputs', str(d)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])
  line = run(tmp_path / 'a')
  assert line['steps'] == 2 and line['warmup'] == 1 and line['full'] is False
  assert line['unit'] == 'tokens/s' and line['higher_is_better'] is True and line['dtype'] == 'u8'
  assert line['ms_per_step'] > 0
  assert abs(line['value'] - line['config']['wordpiece_tokens_per_gpu'] / (line['ms_per_step'] * 1e-3)) <= 1e-6 * line['value']
  for k in ('cpu_baseline', 'legs', 'frontend', 'frontend_c2', 'parquet_writer'):
    assert k not in line
  run(tmp_path / 'b')
  files = sorted(os.listdir(tmp_path / 'a'))
  assert {'ids.npy', 'ntok.npy', 'src0.npy', 'src1.npy', 'bin_count.npy', 'checksums.npy'} <= set(files)
  assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 << 20
  for f in files:
    a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
    assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
  tot = np.load(tmp_path / 'a' / 'totals.npy')
  assert tot[1] == line['config']['wordpiece_tokens_per_gpu'] and tot[2] == line['config']['pairs_per_gpu']
