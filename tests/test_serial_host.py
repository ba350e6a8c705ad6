"""The product's serial tokenizer path (lddl_amd/csrc/tokenize_serial.h: the
split tokenizer's exact fallback, tokenize_fallback_kernel) compiled for the
host by g++ with AddressSanitizer + UndefinedBehaviorSanitizer over the same
tables the device gets (lddl_amd/csrc/tok_tables.h), run over the golden
inputs of both vocabularies and of the synthetic ones at max_tok 512 and 7: no sanitizer report and the
golden ids (HF tokenizers, the call at lddl/dask/bert/pretrain.py:79-80).
CPU only; the HIP build of the same header is checked on the GPU by
tests/test_tokenize_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle.oracle import TABLE, compact

VOCABS = {'bert': os.path.join(ROOT, 'lddl_amd', 'data', 'bert_vocab.txt'),
          'codebert': os.path.join(ROOT, 'lddl_amd', 'data', 'codebert_52000_vocab.txt')}


@pytest.fixture(scope='module')
def host_serial(tmp_path_factory):
  if shutil.which('g++') is None:
    pytest.skip('g++ not available')
  out = str(tmp_path_factory.mktemp('hsan') / 'host_serial')
  subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
                  '-I' + os.path.join(ROOT, 'lddl_amd', 'csrc'), '-o', out, os.path.join(ROOT, 'tests', 'host_serial.cpp')],
                 check=True)
  return out


def run_serial(host_serial, tmp_path, vocab, data, sent_off, max_tok):
  n = len(sent_off) - 1
  fb, fo = tmp_path / 'bytes.bin', tmp_path / 'off.bin'
  np.asarray(data).astype(np.uint8).tofile(fb)
  np.asarray(sent_off).astype(np.int64).tofile(fo)
  fi, fn = tmp_path / 'ids.bin', tmp_path / 'ntok.bin'
  env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23',
             UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1:exitcode=24')
  env.pop('LD_PRELOAD', None)
  r = subprocess.run([host_serial, vocab, TABLE, str(fb), str(fo), str(n), str(max_tok), str(fi), str(fn)],
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-3000:]
  assert 'runtime error' not in r.stderr and 'ERROR: AddressSanitizer' not in r.stderr, r.stderr[-3000:]
  return np.fromfile(fi, dtype=np.int32), np.fromfile(fn, dtype=np.int32)


@pytest.mark.parametrize('name,max_tok', [('bert', 512), ('codebert', 512), ('bert', 7)])
def test_serial_path_under_asan(host_serial, golden, tmp_path, name, max_tok):
  g = golden('tok_%s.npz' % name)
  ids, ntok = run_serial(host_serial, tmp_path, VOCABS[name], g['data'], g['sent_off'], max_tok)
  assert np.array_equal(ntok, np.minimum(g['ntok'], max_tok))
  exp = [x[:max_tok] for x in np.split(g['ids'], np.cumsum(g['ntok'])[:-1])]
  got = compact(ids, ntok, g['sent_off'])
  bad = [i for i, (a, b) in enumerate(zip(exp, got)) if not np.array_equal(a, b)]
  assert not bad, bad[:10]


# the synthetic vocabularies (tests/synth_vocab.py): colliding keys, keys past
# 24 bytes (the pool compare of tokenize_serial.h:probe), multi-byte keys,
# words of many pieces, specials at odd ids and id 0xFFFF
@pytest.mark.parametrize('max_tok', [512, 7])
@pytest.mark.parametrize('name', ['collide', 'long_a', 'long_b', 'ext', 'utf8', 'sparse_a', 'sparse_b', 'specials',
                                  'specials_padlast', 'blanks', 'crlf', 'v65536'])
def test_serial_path_synthetic_vocab_under_asan(host_serial, golden, tmp_path, name, max_tok):
  import synth_vocab as sv
  data, off, exp, gtok = sv.load_golden(golden, name)
  ids, ntok = run_serial(host_serial, tmp_path, sv.vocab_path(name), data, off, max_tok)
  assert np.array_equal(ntok, np.minimum(gtok, max_tok))
  got = compact(ids, ntok, off)
  bad = [i for i in range(len(exp)) if not np.array_equal(exp[i][:max_tok], got[i])]
  assert not bad, [(i, sv.sentence_text(data, off, i)[:80], exp[i][:8].tolist(), got[i][:8].tolist()) for i in bad[:5]]
