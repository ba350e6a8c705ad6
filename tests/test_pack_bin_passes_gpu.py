"""The packers' binning (bin counts taken where the order is initialised, one
stable scatter pass, one offsets pass), the order words that carry
num_tokens through the shuffle, and the shuffle's first-hit search, on small
synthetic corpora against the oracle: every bin regime (1, 2, 4, 8, 16 and
64 bins by lane, 128 bins by the pass per bin, bin_size == seq, no binning),
row counts per partition around the 64-row step, skewed and empty bins,
empty partitions between full ones, masking (mloc / part_nmask), dropped
sentences and documents, and the unpacked order (seq 2048).  Each check
compares the rows in output order, bin_count, tok_off and, with masking, the
masked positions and labels."""
import functools
import random

import numpy as np
import pytest

from oracle import pack_oracle as po
from oracle.oracle import OracleTokenizer

pytestmark = pytest.mark.gpu

MASK = (0.15, 30522, 101, 102, 103)  # ratio, |vocab|, [CLS], [SEP], [MASK] of bert-base-uncased
WORDS = ('the', 'cat', 'sat', 'on', 'a', 'mat', 'and', 'dog', 'ran', 'home', 'with', 'his', 'friend', 'over', 'hill')
EMPTY = (' ', '\t \t', '\x01\x02', '   \x7f ')  # sentences that tokenize to nothing
ROWS = (0, 1, 63, 64, 65, 127, 128, 129, 300)  # rows per partition of the 'counts' corpus
# 'counts': one-sentence documents per partition that give ROWS at seq 128,
# dup 1, seed 7 after the partition's COUNTS_LONG longer documents (found
# with the oracle; test_row_counts_around_the_step asserts them on the CPU first)
COUNTS_LONG = (0, 0, 4, 2, 4, 4, 4, 4, 4)
COUNTS_SHORT = (0, 0, 52, 58, 52, 118, 119, 117, 290)
COUNTS_ARGS = dict(seq=128, dup=1, seed=7, bin_size=32)


def sent(rnd, lo, hi):
  return ' '.join(rnd.choice(WORDS) for _ in range(rnd.randint(lo, hi)))


def doc(rnd, nsent, lo=3, hi=20):
  return [sent(rnd, lo, hi) for _ in range(nsent)]


def counts_docs(short=COUNTS_SHORT, nlong=COUNTS_LONG):
  """partition i gives ROWS[i] rows: 0 from documents that vanish, 1 from a
  lone one-sentence document, the others from a few documents of many
  sentences (rows in every bin) plus one-sentence documents (a row each)"""
  docs, part = [], [0]
  for i, n in enumerate(ROWS):
    rnd = random.Random(100 + i)
    if n == 0:
      docs += [[rnd.choice(EMPTY)], [rnd.choice(EMPTY), rnd.choice(EMPTY)]]
    elif n == 1:
      docs += [doc(rnd, 1, 3, 9)]
    else:
      docs += [doc(rnd, 12, 3, 30) for _ in range(nlong[i])] + [doc(rnd, 1, 2, 40) for _ in range(short[i])]
    part.append(len(docs))
  return docs, part


def regime_docs():
  """three partitions of documents from 1 to 90 sentences of 1 to 60 words:
  rows from a few tokens up to the target at seq 128 and at seq 512, a few
  hundred rows per partition at dup 5; an empty partition between them"""
  rnd = random.Random(21)
  docs, part = [], [0]
  for n in (14, 0, 22, 9):
    docs += [doc(rnd, rnd.choice((1, 2, 3, 5, 8, 20, 40, 90)), 1, 60) for _ in range(n)]
    if n == 0:
      docs += [[rnd.choice(EMPTY)]]
    part.append(len(docs))
  return docs, part


def skew_docs():
  """partition 0: 512-token sentences (every row fills the target: one bin);
  partition 1: one-sentence documents of 4 or 50 words, rows of 11, 57 or
  103 tokens (at bin size 32: bins 0, 1 and 3, bin 2 empty); partition 2:
  one-sentence documents of 1 to 8 words (every row in bin 0)"""
  rnd = random.Random(22)
  docs = [doc(rnd, 3, 512, 512) for _ in range(30)]
  part = [0, len(docs)]
  docs += [doc(rnd, 1, *rnd.choice(((4, 4), (50, 50)))) for _ in range(70)]
  part.append(len(docs))
  docs += [doc(rnd, 1, 1, 8) for _ in range(70)]
  part.append(len(docs))
  return docs, part


def dropped_docs():
  """zero-token sentences at a document's start, middle and end, documents
  whose every sentence is dropped, and a partition that keeps nothing"""
  rnd = random.Random(23)
  e = lambda: rnd.choice(EMPTY)
  docs, part = [], [0]
  docs += [[e()] + doc(rnd, 5), doc(rnd, 4) + [e(), e()] + doc(rnd, 6), [e(), e(), e()], doc(rnd, 7) + [e()],
           [e()] + doc(rnd, 66) + [e()] + doc(rnd, 9) + [e()], [e()], doc(rnd, 3)]
  part.append(len(docs))
  docs += [[e(), e()], [e()], [e(), e(), e()]]
  part.append(len(docs))
  docs += [[e()], doc(rnd, 30, 3, 40), [e()] + doc(rnd, 2) + [e()] + doc(rnd, 2), [e(), e()]]
  part.append(len(docs))
  return docs, part


def long_docs():
  """rows of up to 2048 tokens: documents of 40 to 120 sentences of 20 to 60 words"""
  rnd = random.Random(24)
  return [doc(rnd, rnd.randint(40, 120), 20, 60) for _ in range(8)], [0, 5, 8]


CORPORA = dict(counts=counts_docs, regimes=regime_docs, skew=skew_docs, dropped=dropped_docs, long=long_docs)


@functools.lru_cache(maxsize=None)
def corpus(name):
  """corpus, partition offsets and the oracle's token ids, built once per name"""
  from lddl_amd import synth, pipeline
  docs, pdo = CORPORA[name]()
  c = synth.corpus_from_documents(docs)
  oids, ontok = OracleTokenizer(pipeline.VOCAB_BERT).run(c.data, c.sent_off, 512, nthreads=8)
  return c, np.asarray(pdo, dtype=np.int64), oids, ontok


@functools.lru_cache(maxsize=None)
def expected(name, seq, dup, seed, bin_size, masking=False):
  """the oracle's rows per partition, computed once per configuration"""
  c, pdo, oids, ontok = corpus(name)
  return po.run_bert_shards(c, oids, ontok, pdo, seq, 0.1, dup, seed, bin_size, masking=MASK if masking else None)


def check(name, seq, dup, seed, bin_size, masking=False, spans=False):
  from lddl_amd import pipeline
  c, pdo, oids, ontok = corpus(name)
  exp = expected(name, seq, dup, seed, bin_size, masking)
  res = pipeline.run_bert(c, target_seq_length=seq, bin_size=bin_size, seed=seed, duplicate_factor=dup,
                          part_doc_off=pdo, check_host=True, masking=masking, masked_lm_ratio=MASK[0], spans=spans)
  assert res.spans == spans
  assert np.array_equal(res.ntok_host, ontok)
  pipeline.assert_same_pairs(res, exp)  # rows (and masked positions / labels) in the binned shuffled order
  nb = seq // bin_size if bin_size else 1
  assert res.nbins == nb
  bc = res.bin_count.cpu().numpy()
  for p, part in enumerate(exp):
    assert np.array_equal(bc[p], np.bincount([po.bin_of(r[3], bin_size or seq, nb) for r in part], minlength=nb)), p
  # tok_off: the rows back to back, continuous across the partitions (tok_local + the partitions' bases)
  want = np.concatenate([[0], np.cumsum([r[3] for part in exp for r in part], dtype=np.int64)])
  assert np.array_equal(res.tok_off[:res.n_pairs + 1].cpu().numpy(), want)
  if masking:  # mlm_off: mloc + the partitions' masked-entry bases
    mwant = np.concatenate([[0], np.cumsum([len(r[4]) for part in exp for r in part], dtype=np.int64)])
    assert np.array_equal(res.mlm_off[:res.n_pairs + 1].cpu().numpy(), mwant)
  return res, exp


def bincounts(part, bin_size, nb):
  return np.bincount([po.bin_of(r[3], bin_size, nb) for r in part], minlength=nb)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,bin_size,nb', [(128, 64, 2), (128, 32, 4), (512, 64, 8), (512, 32, 16), (512, 8, 64),
                                             (512, 4, 128), (128, 128, 1), (512, 512, 1), (128, None, 1),
                                             (512, None, 1)])
def test_bin_regimes(gpu, seq, bin_size, nb, spans):
  exp = expected('regimes', seq, 5, 41, bin_size)
  assert not exp[1] and all(len(exp[p]) > 128 for p in (0, 2, 3))  # an empty partition between full ones
  if 1 < nb <= 16:  # every bin holds rows somewhere
    assert all(sum(bincounts(part, bin_size, nb)[b] for part in exp) > 0 for b in range(nb))
  check('regimes', seq, 5, 41, bin_size, spans=spans)


def test_a_step_with_every_bin():
  """CPU: at seq 512 / bin 64 some 64-row step of a partition's shuffled
  (pre-binning) order holds all 8 bins"""
  c, pdo, oids, ontok = corpus('regimes')
  docs = po.filtered_docs(oids, ontok, c.sent_off, c.doc_sent_off, int(pdo[0]), int(pdo[1]))
  pairs = po.partition_pairs(docs, 41 + 0, lambda D, di, r: po.bert_pairs(D, di, 512, 0.1, r, None), 5)
  nt = [sum(len(x) for x in po.pair_tokens(docs, pr)[:2]) + 3 for pr in pairs]
  assert any(len({po.bin_of(n, 64, 8) for n in nt[k:k + 64]}) == 8 for k in range(0, len(nt), 64))


@pytest.mark.parametrize('spans', [False, True])
def test_row_counts_around_the_step(gpu, spans):
  a = COUNTS_ARGS
  exp = expected('counts', a['seq'], a['dup'], a['seed'], a['bin_size'])
  assert [len(part) for part in exp] == list(ROWS)
  check('counts', a['seq'], a['dup'], a['seed'], a['bin_size'], spans=spans)


@pytest.mark.parametrize('bin_size', [32, 64])
def test_skewed_bins(gpu, bin_size):
  nb = 128 // bin_size
  exp = expected('skew', 128, 5, 43, bin_size)
  c0, c1, c2 = (bincounts(part, bin_size, nb) for part in exp)
  assert c0[nb - 1] == len(exp[0]) > 64 and c2[0] == len(exp[2]) > 64  # one bin: the last, the first
  if bin_size == 32:
    assert c1[0] > 0 and c1[1] > 0 and c1[2] == 0 and c1[3] > 0  # an empty bin in the middle
  check('skew', 128, 5, 43, bin_size)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,bin_size', [(128, 32), (512, 64)])
def test_masked(gpu, seq, bin_size, spans):
  check('regimes', seq, 2, 45, bin_size, masking=True, spans=spans)


def test_masked_row_counts(gpu):
  a = COUNTS_ARGS
  check('counts', a['seq'], a['dup'], a['seed'], a['bin_size'], masking=True, spans=True)


@pytest.mark.parametrize('masking', [False, True])
@pytest.mark.parametrize('spans', [False, True])
def test_dropped_sentences(gpu, spans, masking):
  c, pdo, _, ontok = corpus('dropped')
  assert (ontok == 0).sum() >= 20 and ontok[0] == 0
  exp = expected('dropped', 128, 5, 47, 32, masking)
  assert exp[0] and not exp[1] and exp[2]  # the middle partition keeps no document
  check('dropped', 128, 5, 47, 32, masking=masking, spans=spans)


@pytest.mark.parametrize('bin_size,nb', [(256, 8), (16, 128), (None, 1)])
def test_unpacked_order(gpu, bin_size, nb):
  """seq 2048: num_tokens does not fit the order word's high bits, the
  passes read it from the records"""
  exp = expected('long', 2048, 5, 49, bin_size)
  assert max(r[3] for part in exp for r in part) > 1024 and all(len(part) > 64 for part in exp)
  check('long', 2048, 5, 49, bin_size)
