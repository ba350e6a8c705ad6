"""build_vocab_tables (lddl_amd/csrc/tok_tables.h) compiled for the host by g++
with AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_vocab_tables.cpp,
a program of its own) over the synthetic vocabularies of tests/synth_vocab.py:
no sanitizer report; every key is found again by a host restatement of the
WordPiece kernel's bucket probe, with all its Bloom and extension bits set;
the rendering tables give every entry back; each vocabulary reaches the table
path it was written for (probe distance, displaced whole words, keys past 24
bytes); malformed files are refused with LDDL_EFORMAT.  CPU only."""
import json
import os
import shutil
import subprocess

import pytest

import synth_vocab as sv
from conftest import GOLDEN, ROOT


@pytest.fixture(scope='module')
def host_tables(tmp_path_factory):
  if shutil.which('g++') is None:
    pytest.skip('g++ not available')
  out = str(tmp_path_factory.mktemp('hvt') / 'host_vocab_tables')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                  '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'), '-o', out,
                  os.path.join(ROOT, 'tests', 'host_vocab_tables.cpp')], check=True)

  def run(path, *args):
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23',
               UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=24')
    env.pop('LD_PRELOAD', None)
    r = subprocess.run([out, str(path)] + list(args), env=env, capture_output=True, timeout=300)
    err = r.stderr.decode('utf-8', 'replace')
    assert r.returncode == 0, err[-3000:]
    assert 'runtime error' not in err and 'ERROR: AddressSanitizer' not in err, err[-3000:]
    facts, entries = {}, {}
    for line in r.stdout.decode('utf-8', 'replace').splitlines():
      k, _, v = line.partition('=')
      if k == 'entry':
        i, _, hx = v.partition(':')
        entries[int(i)] = bytes.fromhex(hx)
      else:
        facts[k] = v
    return facts, entries
  return run


def key_lengths(name):
  """byte lengths of the distinct non-empty keys without / with '##', as HF reads the lines"""
  out = ([], [])
  for l in set(sv.vocab_bytes(name).decode().split('\n')):
    cont = l.startswith('##')
    if len(l) > 2 * cont:
      out[cont].append(len(l.encode()) - 2 * cont)
  return out


@pytest.mark.parametrize('name', sv.NAMES)
def test_tables_of_synthetic_vocab(host_tables, name):
  f, _ = host_tables(sv.vocab_path(name))
  assert f['rc'] == '0', f
  assert int(f['n']) == sv.vocab_size(name)
  for k in ('not_found', 'bloom_missing', 'ext_missing', 'render_bad'):
    assert f[k] == '0', (k, f)
  assert (f['maxb0'], f['maxb1']) == (f['key_maxb0'], f['key_maxb1'])
  if name not in ('blanks', 'crlf'):  # (their lines are trimmed first)
    kl = key_lengths(name)
    assert (int(f['maxb0']), int(f['maxb1'])) == (max(kl[0]), max(kl[1], default=0))
    assert int(f['long_keys']) == sum(1 for x in kl[0] + kl[1] if x > 24)
    assert int(f['keys']) == len(kl[0]) + len(kl[1])


def test_each_vocab_reaches_its_table_path(host_tables):
  f, _ = host_tables(sv.vocab_path('collide'))
  # groups of 6 keys with one home bucket: two slots there, two in the next, two in a third
  assert int(f['max_probe']) >= 2
  assert int(f['whole_off_slot0']) >= len(sv.collide_displaced_words()) >= 8
  assert int(f['long_keys']) == 12
  a, _ = host_tables(sv.vocab_path('long_a'))
  b, _ = host_tables(sv.vocab_path('long_b'))
  assert (a['maxb0'], a['maxb1']) == ('200', '202') and (b['maxb0'], b['maxb1']) == ('202', '200')
  assert int(a['long_keys']) >= 50 and int(b['long_keys']) >= 50
  u, _ = host_tables(sv.vocab_path('utf8'))
  assert int(u['long_keys']) >= 8 and int(u['maxb0']) == 33
  s, _ = host_tables(sv.vocab_path('specials'))
  n = sv.vocab_size('specials')
  pad, unk, cls, sep, mask = map(int, s['special'].split(','))
  assert (pad, unk, mask) == (n - 2, 0, n - 1) and 0 < cls < sep < n - 2
  s, _ = host_tables(sv.vocab_path('specials_padlast'))
  assert list(map(int, s['special'].split(',')))[::4] == [n - 1, n - 2]


@pytest.mark.parametrize('name', sv.LINE_VOCABS)
def test_vocab_lines_as_hf(host_tables, name):
  """trailing blanks, CRLF, duplicates, an empty line, no final newline: the
  entries the product keeps are HF's tokens at HF's ids (a duplicate's
  earlier ids are no tokens of HF's map)"""
  both = json.load(open(os.path.join(GOLDEN, 'vocab_lines_hf.json')))
  hf = both[name]
  f, entries = host_tables(sv.vocab_path(name), '--dump')
  assert list(map(int, f['special'].split(','))) == both[name + ':special_ids'] == [hf[s] for s in sv.SPECIALS]
  assert f['rc'] == '0' and len(entries) == int(f['n']) == sv.vocab_size(name)
  for t, i in hf.items():
    assert entries[i] == t.encode(), (t, i, entries[i])
  texts = [e.decode() for e in entries.values()]
  assert set(texts) == set(hf)
  if name == 'blanks':
    assert ' qr' in hf and 'mn\x1c' in hf and 'ab' in hf and 'wx' in hf and 'ij' in hf  # only the end is trimmed
    # every White_Space code point is trimmed, the look-alikes are not: a slip in the list fails here
    assert all(sv._ws_key(k) in hf for k, c in enumerate(sv.WHITE_SPACE) if c != 0x0A)
    assert all(l in hf for l in sv.NWS_LINES) and hf['yz'] == len(entries) - len(sv.WS_LINES) - len(sv.NWS_LINES) - 1
  if name == 'dupspecial':
    n = len(entries)
    assert [hf['[SEP]'], hf['[UNK]']] == [n - 1, n - 1 - (len(sv._base()) - len(sv._base()) // 2) - 1]
    assert hf['[MASK]'] == hf['[UNK]'] - 1 > 4


def write(tmp_path, name, data):
  p = tmp_path / name
  p.write_bytes(data)
  return p


BASE = b'[PAD]\n[UNK]\n[CLS]\n[SEP]\n[MASK]\n'


BAD = dict([
    ('empty', b''),
    ('lines65537', BASE + b''.join(b'w%d\n' % i for i in range(65532))),
    ('no_mask', BASE.replace(b'[MASK]\n', b'') + b'a\n'),
    ('no_unk', BASE.replace(b'[UNK]', b'[unk]')),
    ('key256', BASE + b'a' * 256 + b'\n'),
    ('cont254', BASE + b'##' + b'a' * 254 + b'\n'),
    ('cont255', BASE + b'##' + b'a' * 255 + b'\n'),
])


@pytest.mark.parametrize('case', list(BAD))
def test_malformed_vocab_is_eformat(host_tables, tmp_path, case):
  data = BAD[case]
  f, _ = host_tables(write(tmp_path, case + '.txt', data))
  assert f['rc'] != '0' and f['eformat'] == '1', f
  assert f['err']


GOOD = dict((c, (d, n)) for c, d, n in [
    ('lines65536', BASE + b''.join(b'w%d\n' % i for i in range(65531)), 65536),
    ('key255', BASE + b'a' * 255 + b'\n' + b'b\n', 7),
    ('cont253', BASE + b'##' + b'a' * 253 + b'\nb\n', 7),  # 255 bytes with its '##': the longest entry rendering holds
    ('key255_blank', BASE + b'a' * 255 + b' \t\r\nb', 7),  # within 255 once trimmed
])


@pytest.mark.parametrize('case', list(GOOD))
def test_longest_accepted_entries(host_tables, tmp_path, case):
  data, n = GOOD[case]
  f, entries = host_tables(write(tmp_path, case + '.txt', data), '--dump')
  assert f['rc'] == '0' and int(f['n']) == n, f
  for k in ('not_found', 'bloom_missing', 'ext_missing', 'render_bad'):
    assert f[k] == '0', (k, f)
  if n == 7:
    assert len(entries[5]) == 255 and entries[6] == b'b'


def test_widths_vocab_renders_every_length(host_tables):
  """the render tests' vocabulary (tests/test_render_gpu.py): the rendering tables give back an entry of
  every length 0..255, the empty line included"""
  f, entries = host_tables(sv.vocab_path('widths'), '--dump')
  assert f['rc'] == '0' and f['render_bad'] == '0' and int(f['n']) == sv.vocab_size('widths') == len(entries)
  lines = sv.vocab_bytes('widths').split(b'\n')[:-1]
  assert [entries[i] for i in range(len(lines))] == lines
  assert [len(entries[sv.widths_id(k)]) for k in range(256)] == list(range(256))
  assert (f['maxb0'], f['maxb1']) == ('255', '253')
