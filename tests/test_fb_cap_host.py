"""The capacity of the split tokenizer's fallback list (fb_list_cap,
lddl_amd/csrc/tokenize.h) against a model of the scan's windows
(tests/window_model.py).

The scan lists every window it does not model in fb_list, and any window may
be one, so a segment's list has to hold all of its windows.  A window also
closes after 31 sentences, and empty and one-byte sentences are legal: the
windows per tile are bounded by the sentence count, not by bytes.  The
capacity was 2 * seg + 64 ranges, which a sentence of one long non-vocabulary
word followed by 30 empty ones, repeated, passes about eightfold (ADVICE.md,
round 6): the recorded bug, asserted below.

The header's function is compiled for the host by g++ with AddressSanitizer +
UndefinedBehaviorSanitizer (tests/host_fb_cap.cpp) and asked for the capacity
of every (segment tiles, sentences) pair; the model counts the windows per
segment of sentence-offset arrays that are dense in sentences.  CPU only; the
same corpora run on the GPU in tests/test_tokenize_dense_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import window_model as wm

SEGS = [1, 16, 61, 97, 1 << 40]  # (the last: one segment of all tiles)
ALIGN_SEG = 61                   # every start alignment 0..15 at this one


def _off(lens):
  return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def advice_example(reps=2200, word=60):
  """a sentence of one word too long for a record, then 30 empty ones"""
  return _off(([word] + [0] * 30) * reps)  # 129 KiB


def runs_on_boundaries(run=5000):
  """128-byte sentences (8 per tile) with runs of empty sentences starting
  exactly on a tile (5), a super-tile (32, 112) and a segment boundary (61,
  97; 32 and 112 for segments of 16)"""
  lens = []
  for t in range(128):
    if t in (5, 32, 61, 97, 112):
      lens += [0] * run
    lens += [128] * 8
  return _off(lens)


def families():
  rng = np.random.default_rng(20261019)
  rnd = []
  while sum(rnd) < 192 * 1024:
    rnd.append(int(rng.choice([0, 1, 5, 60, 700, 2047, 2048, 2049, 5000])))
  longs = []
  for k in range(40):
    longs += [0] * 45 + [(2049, 3000, 5000)[k % 3]]
  return {
      'advice': advice_example(),
      'advice_short_word': advice_example(22_000, 3),  # (dense enough for a segment of one tile)
      'all_empty': _off([0] * 100_000),
      'one_byte': _off([1] * (128 * 1024)),
      'alt_2047_empty': _off([2047, 0] * 64),
      'long_between_empties': _off(longs),
      'random_lengths': _off(rnd),
      'runs_on_boundaries': runs_on_boundaries(),
  }


FAMILIES = families()


@pytest.fixture(scope='module')
def host_fb_cap(tmp_path_factory):
  if shutil.which('g++') is None:
    pytest.skip('g++ not available')
  out = str(tmp_path_factory.mktemp('hcap') / 'host_fb_cap')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                  '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'), '-o', out, os.path.join(ROOT, 'tests', 'host_fb_cap.cpp')],
                 check=True)

  def caps(pairs):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=24')
    env.pop('LD_PRELOAD', None)
    r = subprocess.run([out] + [str(int(x)) for p in pairs for x in p], env=env, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'ERROR: AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(pairs)
    return got
  return caps


def test_families_are_what_they_claim():
  for name, off in FAMILIES.items():
    nbytes = int(off[-1])
    assert nbytes == 0 or 64 * 1024 <= nbytes <= 256 * 1024, (name, nbytes)
  off = FAMILIES['runs_on_boundaries']
  for t in (5, 32, 61, 97, 112):  # a run of 5000 empty sentences starts exactly on tile t
    s = int(np.searchsorted(off[:-1], t * 1024))
    assert off[s] == t * 1024 and np.all(off[s:s + 5001] == t * 1024)
  assert len(FAMILIES['all_empty']) - 1 == 100_000 and FAMILIES['all_empty'][-1] == 0


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_windows_fit_the_list(host_fb_cap, name):
  """no segment has more windows than fb_list_cap(segment tiles, n_sent)"""
  off = FAMILIES[name]
  n_sent, nt = len(off) - 1, wm.tile_count(int(off[-1] - off[0]))
  cases = [(seg, 0) for seg in SEGS] + [(ALIGN_SEG, al) for al in range(1, 16)]
  caps = host_fb_cap([(min(seg, nt), n_sent) for seg, _ in cases])
  for (seg, al), cap in zip(cases, caps):
    per_seg = wm.windows(off, seg, al)
    assert sum(ns for ws in per_seg for _, ns in ws) == n_sent  # the windows partition the sentences
    assert all(1 <= ns <= wm.NS_MAX for ws in per_seg for _, ns in ws)
    assert cap >= min(seg, nt)  # one range per tile: the serial path
    worst = max(len(ws) for ws in per_seg)
    assert worst <= cap, (name, seg, al, worst, cap)


def test_advice_example_passes_the_old_capacity():
  """the recorded bug: the windows of one segment pass 2 * seg + 64 (about 17
  windows a tile: in segments of 16 tiles and more; in a segment of one tile,
  where the constant term covers 66, with a 3-byte word in its place)"""
  off = FAMILIES['advice']
  nt = wm.tile_count(int(off[-1]))
  for seg in SEGS:
    worst = max(len(ws) for ws in wm.windows(off, seg))
    short = max(len(ws) for ws in wm.windows(FAMILIES['advice_short_word'], seg))
    assert short > wm.old_cap(min(seg, wm.tile_count(int(FAMILIES['advice_short_word'][-1])))), seg
    if seg >= 16:
      assert worst > wm.old_cap(min(seg, nt)), seg
  # a window per long word, about 17 a tile: several times the old capacity
  ws = wm.windows(off, 1 << 40)[0]
  assert len(ws) >= 2200 and len(ws) >= 16 * (nt - 1) and len(ws) > 6 * wm.old_cap(nt)


def test_capacity_at_the_bench_shape(host_fb_cap):
  """sized by n_sent alone the list would be 2.3 GB at the bench shape (2^23
  tiles a segment, 142 M sentences); it may cost at most twice the 268 MB of
  2 * seg + 64 ranges there"""
  seg, n_sent = 1 << 23, 142_000_000
  cap, = host_fb_cap([(seg, n_sent)])
  assert wm.old_cap(seg) <= cap <= 2 * wm.old_cap(seg)
  assert cap * 16 <= 2 * 268_436_480
