"""Every Unicode scalar value through the oracle, against the digests that HF
tokenizers gave for the same corpora (tests/golden/tok_codepoints.npz,
tools/gen_golden_codepoints.py; families in tests/codepoint_sweep.py).  CPU
only.  No block is excluded."""
import numpy as np
import pytest

import codepoint_sweep as cs
from oracle.oracle import OracleTokenizer
from test_oracle_golden import VOCABS

CASES = [(v, f) for v in ('bert', 'codebert') for f in cs.GOLDEN_FAMILIES[v]]
EXCLUDED_BLOCKS = {}  # (vocab, family) -> block indices left out of the comparison: none


@pytest.fixture(scope='module')
def gold(golden):
  return golden(cs.GOLDEN_FILE)


_ORACLE = {}


def oracle_run(vocab, family, sel, max_tok=512):
  """(flat ids int32, ntok) of the oracle over a family, computed once per process"""
  key = (vocab, family, max_tok)
  if key not in _ORACLE:
    data, sent_off = cs.corpus(family, sel)
    ids, ntok = OracleTokenizer(VOCABS[vocab]).run(data, sent_off, max_tok, nthreads=8)
    flat = cs.flat_ids(ids, ntok, sent_off)
    flat.setflags(write=False)
    ntok.setflags(write=False)
    _ORACLE[key] = (flat, ntok)
  return _ORACLE[key]


def assert_blocks(vocab, family, sel, gold, flat, ntok, what):
  """the digests and token totals of (flat, ntok) equal the golden's in every block"""
  dig, tot = cs.digest_blocks(flat, ntok)
  gdig, gtot = gold[cs.golden_key(vocab, family, 'dig')], gold[cs.golden_key(vocab, family, 'tot')]
  skip = EXCLUDED_BLOCKS.get((vocab, family), ())
  bad = [b for b in cs.first_bad_blocks(dig, tot, gdig, gtot) if b not in skip]
  if bad:
    b = bad[0]
    pytest.fail('%s %s %s: %d of %d blocks differ from HF tokenizers %s; first block %d (sentences %d..%d, %s): '
                '%d tokens, golden %d' %
                (what, vocab, family, len(bad), len(gdig), str(gold['tokenizers']), b, b * cs.BLOCK,
                 min(len(ntok), (b + 1) * cs.BLOCK) - 1, cs.block_range(family, sel, b, len(ntok)),
                 int(tot[b]) if b < len(tot) else -1, int(gtot[b]) if b < len(gtot) else -1))


def test_no_block_is_excluded():
  assert not any(EXCLUDED_BLOCKS.values())


def test_every_scalar_value_once(gold):
  assert len(np.unique(cs.CPS)) == 1_112_064 and not ((cs.CPS >= 0xD800) & (cs.CPS < 0xE000)).any()
  sel = cs.golden_selection(gold)
  assert cs.n_sentences('markpairs', sel) == 6050 and cs.n_sentences('len100', sel) == 20380
  assert cs.n_sentences('run40') == 27802
  assert len(sel['kept']) >= 83 and cs.n_sentences('markwords', sel) == len(cs.sentences('markwords', sel))


@pytest.mark.parametrize('vocab,family', CASES)
def test_oracle_matches_hf_digests(gold, vocab, family):
  sel = cs.golden_selection(gold)
  data, sent_off = cs.corpus(family, sel)
  assert len(sent_off) - 1 == cs.n_sentences(family, sel)
  assert cs.corpus_digest(data, sent_off) == gold[cs.golden_key(vocab, family, 'corpus')], \
      'the rebuilt %s corpus is not the one the golden digests were taken over' % family
  flat, ntok = oracle_run(vocab, family, sel)
  assert_blocks(vocab, family, sel, gold, flat, ntok, 'oracle')


@pytest.mark.parametrize('family', ['spaced', 'run40sp'])
@pytest.mark.parametrize('vocab', ['bert', 'codebert'])
def test_oracle_truncation_is_a_prefix(gold, vocab, family):
  """max_tok = 3: the counts are min(ntok512, 3) and the ids the first 3 of
  the untruncated run (which the golden digests pin)"""
  sel = cs.golden_selection(gold)
  flat, ntok = oracle_run(vocab, family, sel)
  cut, nc = oracle_run(vocab, family, sel, 3)
  assert np.array_equal(nc, np.minimum(ntok, 3))
  off = np.cumsum(ntok) - ntok
  idx = np.repeat(off, nc) + (np.arange(int(nc.sum())) - np.repeat(np.cumsum(nc) - nc, nc))
  bad = np.flatnonzero(flat[idx] != cut)
  if len(bad):
    s = int(np.searchsorted(np.cumsum(nc), bad[0], side='right'))
    pytest.fail('%s %s: sentence %d (%s) truncated to 3 is not a prefix' %
                (vocab, family, s, ' '.join('U+%04X' % c for c in cs.sentence_cps(family, sel, s))))
