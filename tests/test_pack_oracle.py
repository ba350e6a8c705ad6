"""The Python packer restatement (oracle/pack_oracle.py) against golden rows
produced by the reference's own create_pairs_from_document
(tools/gen_golden_pack.py).  CPU only."""
import gzip
import json
import os

import pytest

from conftest import GOLDEN
from oracle import pack_oracle as po


def load(name):
  with gzip.open(os.path.join(GOLDEN, name), 'rt') as f:
    return json.load(f)


BERT = load('pack_bert.json.gz')
CODE = load('pack_codebert.json.gz')


def bert_rows(case):
  c = case['cfg']
  docs = [[s for s in d if s] for d in case['docs']]
  docs = [d for d in docs if d]
  pairs = po.partition_pairs(docs, case['seed'],
                             lambda D, di, r: po.bert_pairs(D, di, c['max_seq'], c['ssp'], r), c['dup'])
  return docs, pairs


@pytest.mark.parametrize('k', [i for i, c in enumerate(BERT['cases']) if not c['cfg']['masking']])
def test_bert_pairs_match_reference(k):
  case = BERT['cases'][k]
  if case['error']:
    with pytest.raises(AssertionError):
      bert_rows(case)
    return
  docs, pairs = bert_rows(case)
  rows = case['rows']
  assert len(pairs) == len(rows)
  for pr, row in zip(pairs, rows):
    a, b, rn = po.pair_tokens(docs, pr)
    assert (a, b, rn, len(a) + len(b) + 3) == (row['A'], row['B'], row['is_random_next'], row['num_tokens'])
  assert [po.bin_of(r['num_tokens'], case['bin_size'], case['nbins']) for r in rows] == case['bins']


@pytest.mark.parametrize('k', range(len(CODE['cases'])))
def test_codebert_pairs_match_reference(k):
  case = CODE['cases'][k]
  c = case['cfg']
  docs, nd = [], []
  for d, n in zip(case['docs'], case['ndoc']):
    ds = [s for s in d[:n] if s]
    cs = [s for s in d[n:] if s]
    if cs:
      docs.append(ds + cs)
      nd.append(len(ds))

  def run():
    return po.partition_pairs(docs, case['seed'],
                              lambda D, di, r: po.codebert_pairs(D, nd, di, c['max_seq'], c['ssp'], r), c['dup'])
  if case['error']:
    with pytest.raises(IndexError):
      run()
    return
  pairs = run()
  assert len(pairs) == len(case['rows'])
  for (doc_s, code_s, dw, cw), row in zip(pairs, case['rows']):
    dt = [t for (d, s) in doc_s for t in docs[d][s]][dw[0]:dw[1]]
    ct = [t for (d, s) in code_s for t in docs[d][s]][cw[0]:cw[1]]
    special = 3 if nd[code_s[0][0]] else 2
    assert (dt, ct, len(dt) + len(ct) + special) == (row['doc'], row['code'], row['num_tokens'])


REGIMES = load('pack_codebert_regimes.json.gz')


def regime_corpus(case, corpus):
  """the corpus of tests/codebert_regimes.py the fixture was made from (the
  fixture keeps its segment lengths, not its ids)"""
  docs, ndoc, pdo = corpus
  assert [[len(s) for s in d] for d in docs] == case['corpus'] and list(ndoc) == case['ndoc']
  assert list(pdo) == case['part_doc_off']
  return docs, ndoc, pdo


@pytest.mark.parametrize('k', range(len(REGIMES['cases'])))
def test_codebert_regimes_match_reference(k):
  """The regime corpora (unflushed docstring, flush in the second window,
  lost tail, the 16-token drop rule, ...): po.codebert_pairs against the
  reference's rows, per partition in the shuffled order."""
  import codebert_regimes as cr
  case = REGIMES['cases'][k]
  seq, ssp = case['seq'], case['ssp']
  assert (seq, ssp) == cr.CONFIGS[k] and case['dup'] == cr.DUP
  assert case['seed'] == cr.PACK_SEEDS.get((seq, ssp), cr.PACK_SEED)
  docs, ndoc, pdo = regime_corpus(case, cr.corpus(seq))
  for p, exp in enumerate(case['parts']):
    D, nd = cr.partition_docs(docs, ndoc, pdo, p)
    pairs = po.partition_pairs(D, case['seed'] + p, lambda X, di, r: po.codebert_pairs(X, nd, di, seq, ssp, r),
                               case['dup'])
    got = []
    for (doc_s, code_s, dw, cw) in pairs:
      dt = [t for (d, s) in doc_s for t in D[d][s]][dw[0]:dw[1]]
      ct = [t for (d, s) in code_s for t in D[d][s]][cw[0]:cw[1]]
      got.append([dt, ct, len(dt) + len(ct) + (3 if nd[code_s[0][0]] else 2)])
    assert got == exp, p
  # the same rows as the GPU tests take them: binned
  assert cr.golden_rows(case) == cr.oracle_rows(seq, ssp)[1:]


@pytest.mark.parametrize('k', range(len(REGIMES['errors'])))
def test_codebert_regime_errors_match_reference(k):
  """the reference raises exactly that exception, in partition 1 alone; so does the oracle"""
  import codebert_regimes as cr
  case = REGIMES['errors'][k]
  seq, ssp, exc = case['seq'], case['ssp'], case['error']
  assert (seq, ssp, exc) == cr.ERROR_CONFIGS[k] and case['errors'] == [None, exc, None]
  docs, ndoc, pdo = regime_corpus(case, cr.error_corpus(seq, exc))
  for p in range(3):
    D, nd = cr.partition_docs(docs, ndoc, pdo, p)

    def run():
      po.partition_pairs(D, case['seed'] + p, lambda X, di, r: po.codebert_pairs(X, nd, di, seq, ssp, r), case['dup'])
    if p == 1:
      with pytest.raises(IndexError if exc == 'IndexError' else AssertionError):
        run()
    else:
      run()


BERT_MASK = (0.15, 30522, 101, 102, 103)  # ratio, |vocab|, [CLS], [SEP], [MASK]


@pytest.mark.parametrize('k', [i for i, c in enumerate(BERT['cases']) if c['cfg']['masking']])
def test_bert_masked_pairs_match_reference(k):
  """Static masking (pretrain.py:182-238) on the reference's own rows."""
  case = BERT['cases'][k]
  c = case['cfg']
  docs = [[s for s in d if s] for d in case['docs']]
  docs = [d for d in docs if d]
  if case['error']:
    with pytest.raises(AssertionError):
      po.partition_pairs(docs, case['seed'],
                         lambda D, di, r: po.bert_pairs(D, di, c['max_seq'], c['ssp'], r, BERT_MASK), c['dup'])
    return
  pairs = po.partition_pairs(docs, case['seed'],
                             lambda D, di, r: po.bert_pairs(D, di, c['max_seq'], c['ssp'], r, BERT_MASK), c['dup'])
  rows = case['rows']
  assert len(pairs) == len(rows)
  n_masked = 0
  for pr, row in zip(pairs, rows):
    a, b, rn = po.pair_tokens(docs, pr)
    ma, mb, pos, lab = pr[5]
    assert (ma, mb, rn, len(a) + len(b) + 3) == (row['A'], row['B'], row['is_random_next'], row['num_tokens'])
    assert pos == row['masked_lm_positions'] and lab == row['masked_lm_labels']
    n_masked += len(pos)
  assert n_masked > 0 or not rows
