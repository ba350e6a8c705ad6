"""Every Unicode scalar value through both GPU tokenizer paths (the exact
serial path, LDDL_TOKENIZE_ALGO=0, and the split tokenizer, 5): ntok and every
emitted id equal to the oracle's, and the block digests equal to the ones HF
tokenizers gave (tests/golden/tok_codepoints.npz) -- families and digests in
tests/codepoint_sweep.py.  The split scan reads per-code-point tables
(tok_tables.h: bmp, xmap) and works inside fixed capacities (expansion
markers, dirty-word bytes, units per round, key bytes) that only windows full
of exceptions fill; run40 / run40sp are those windows.

One Tokenizer per vocabulary serves every case (scratch reuse across families,
algorithms and max_tok), with per-kernel timing on only where a case reads
lddl_tokenize_stats: the rest runs the default path.  With LDDL_CODEPOINTS_REPORT=<file> the split
tokenizer's fallback share per family is appended to that file."""
import os

import numpy as np
import pytest

import codepoint_sweep as cs
import window_model as wm
from test_codepoints_host import assert_blocks, gold, oracle_run  # noqa: F401 (gold: fixture)
from test_oracle_golden import VOCABS
from test_tokenize_gpu import run_hip

pytestmark = pytest.mark.gpu

CASES = [(v, f) for v in ('bert', 'codebert') for f in cs.GOLDEN_FAMILIES[v]]
_TOK = {}


def tokenizer(vocab, algo, monkeypatch, timing=False):
  """the vocabulary's one Tokenizer, switched to the algorithm; timing: the
  call's counters are kept for stats() (event records around every launch and
  wp_kernel's record count, which the default path does without)"""
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', algo)
  if vocab not in _TOK:
    _TOK[vocab] = Tokenizer(VOCABS[vocab])
  _TOK[vocab].set_timing(timing)
  assert _TOK[vocab].set_algo(int(algo)) == int(algo)
  return _TOK[vocab]


def assert_equals_oracle(tok, vocab, family, sel, max_tok):
  """one call over the family: ntok and every emitted id equal to the oracle's
  at the same max_tok; returns the GPU's (flat ids, ntok)"""
  data, sent_off = cs.corpus(family, sel)
  oflat, ontok = oracle_run(vocab, family, sel, max_tok)
  sparse, ntok = run_hip(tok, data, sent_off, max_tok)
  bad = np.flatnonzero(ntok != ontok)
  if len(bad) == 0:
    flat = cs.flat_ids(sparse, ntok, sent_off)
    wrong = np.flatnonzero(flat != oflat)
    # (the sentences of the differing ids, each once)
    bad = np.unique(np.searchsorted(np.cumsum(ontok), wrong, side='right'))
  if len(bad):
    ooff = np.cumsum(ontok) - ontok
    lines = []
    for s in bad[:10].tolist():
      got = sparse[sent_off[s]:sent_off[s] + min(int(ntok[s]), 24)].tolist()
      lines.append('  sentence %d, %s, %r: ntok %d, oracle %d; ids %s, oracle %s' %
                   (s, ' '.join('U+%04X' % c for c in cs.sentence_cps(family, sel, s)),
                    cs.sentence_text(data, sent_off, s)[:60], ntok[s], ontok[s], got,
                    oflat[ooff[s]:ooff[s] + min(int(ontok[s]), 24)].tolist()))
    pytest.fail('%s %s max_tok %d: %d sentences differ from the oracle, the first:\n%s' %
                (vocab, family, max_tok, len(bad), '\n'.join(lines)))
  return flat, ntok


def report(line):
  path = os.environ.get('LDDL_CODEPOINTS_REPORT')
  print(line)
  if path:
    with open(path, 'a') as f:
      f.write(line + '\n')


def assert_not_all_serial(tok, vocab, family, sel):
  """the split tokenizer's last call listed fewer windows for the serial path
  than it had: the family did not pass because everything went down the
  serial path.  stats()['fallback_tiles'] counts listed windows -- up to 31
  sentences or 2 KiB each, tests/window_model.py gives the call's -- not the
  1 KiB tiles that lddl_tokenize sizes its buffers by, so it is held against
  the windows: a corpus of short sentences has several windows per tile
  (markpairs: 197 windows in 44 tiles, 65 of them listed)."""
  data, sent_off = cs.corpus(family, sel)
  listed = tok.stats()['fallback_tiles']
  windows = sum(len(w) for w in wm.windows(sent_off, 1 << 40))
  tiles = wm.tile_count(len(data))
  report('%-8s %-9s tiles %6d windows %6d listed %6d share of windows %.4f' %
         (vocab, family, tiles, windows, listed, listed / windows))
  assert listed < windows, (listed, windows, tiles)


@pytest.mark.parametrize('algo', ['0', '5'])
@pytest.mark.parametrize('vocab,family', CASES)
def test_every_code_point(gpu, gold, monkeypatch, vocab, family, algo):
  sel = cs.golden_selection(gold)
  tok = tokenizer(vocab, algo, monkeypatch, timing=algo == '5')
  flat, ntok = assert_equals_oracle(tok, vocab, family, sel, 512)
  # the same output against HF's digests: holds whatever oracle was built here
  assert_blocks(vocab, family, sel, gold, flat, ntok, 'algorithm ' + algo)
  if algo == '5':
    assert_not_all_serial(tok, vocab, family, sel)


@pytest.mark.parametrize('max_tok', [3, 1])
@pytest.mark.parametrize('family', ['spaced', 'run40sp'])
@pytest.mark.parametrize('vocab', ['bert', 'codebert'])
def test_every_code_point_truncated(gpu, gold, monkeypatch, vocab, family, max_tok):
  sel = cs.golden_selection(gold)
  assert_equals_oracle(tokenizer(vocab, '5', monkeypatch), vocab, family, sel, max_tok)


SEG97, SEG7, CHUNKS3 = {'LDDL_SPLIT_SEG': '97'}, {'LDDL_SPLIT_SEG': '7'}, {'LDDL_SPLIT_CHUNKS': '3'}


@pytest.mark.parametrize('vocab,family,env', [
    pytest.param('bert', 'run40', SEG97, id='run40-seg97'), pytest.param('bert', 'run40', CHUNKS3, id='run40-chunks3'),
    pytest.param('bert', 'markpairs', SEG97, id='markpairs-seg97'),
    pytest.param('bert', 'markpairs', CHUNKS3, id='markpairs-chunks3'),
    pytest.param('bert', 'markpairs', SEG7, id='markpairs-seg7'),
    pytest.param('codebert', 'markwords', SEG97, id='codebert-markwords-seg97'),
    pytest.param('codebert', 'markwords', CHUNKS3, id='codebert-markwords-chunks3')])
def test_dense_exceptions_at_segment_seams(gpu, gold, monkeypatch, vocab, family, env):
  """dense exception windows against segment seams (97 tiles a segment: run40
  has 4280 tiles, markwords 852; markpairs has 44, one segment at 97, so it
  runs at 7 tiles a segment as well) and against record-capacity fallback (3
  record chunks); markwords under codebert, whose vocabulary holds the marks"""
  sel = cs.golden_selection(gold)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  flat, ntok = assert_equals_oracle(tokenizer(vocab, '5', monkeypatch), vocab, family, sel, 512)
  assert_blocks(vocab, family, sel, gold, flat, ntok, 'algorithm 5, %s' % env)
