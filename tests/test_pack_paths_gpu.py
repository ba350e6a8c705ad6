"""Branches of the wave packer's pair loop that the corpus-level suites reach
rarely or not at all, each on a small synthetic corpus against the oracle:
register-resident and global-fill documents, the document table past its
static LDS copy, >= 65536 kept sentences, dropped sentences / documents
(slot != sentence index; spans and materialised rows), partitions of one and
two documents, truncation across MT19937 twists, the seed edge values, and
the masked instantiation on every one of those corpora (the truncation draws
and the masking draws share one MT19937 stream there)."""
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


def sent(rnd, lo, hi):
  return ' '.join(rnd.choice(WORDS) for _ in range(rnd.randint(lo, hi)))


def doc(rnd, nsent, lo=3, hi=20):
  return [sent(rnd, lo, hi) for _ in range(nsent)]


def mixed_docs():
  """documents of <= 64 and > 64 kept sentences (register-resident / global
  fill), both as the visited document and as the random-next one"""
  rnd = random.Random(1)
  sizes = [3, 64, 65, 130, 1, 64, 3, 65, 2, 130, 63, 5]
  return [doc(rnd, n) for n in sizes], [0, 5, len(sizes)]


def doctable_docs():
  """> 512 kept documents in one partition: the document table stays in global memory"""
  rnd = random.Random(2)
  return [doc(rnd, rnd.randint(2, 3), 2, 6) for _ in range(600)], [0, 600]


def many_sentence_docs():
  """>= 65536 kept sentences of one or two words in one partition"""
  rnd = random.Random(3)
  docs = [doc(rnd, 331, 1, 2) for _ in range(200)]
  assert sum(len(d) for d in docs) >= 65536
  return docs, [0, len(docs)]


def dropped_docs():
  """empty sentences at the start, middle and end of documents, documents
  that vanish, and a partition whose first and last documents vanish"""
  rnd = random.Random(4)
  e = lambda: rnd.choice(EMPTY)
  docs = []
  part = [0]
  # partition 0: empties inside kept documents, a vanishing document between them
  docs += [[e()] + doc(rnd, 4), doc(rnd, 3) + [e()] + doc(rnd, 5), [e(), e()], doc(rnd, 6) + [e(), e()],
           [e()] + doc(rnd, 70) + [e()] + doc(rnd, 10) + [e()], doc(rnd, 2)]
  part.append(len(docs))
  # partition 1: the first and the last document vanish
  docs += [[e()], doc(rnd, 5), [e()] + doc(rnd, 2) + [e()] + doc(rnd, 2), [e(), e(), e()], doc(rnd, 66), [e()]]
  part.append(len(docs))
  # partition 2: nothing dropped (identity slots) next to the others
  docs += [doc(rnd, 4), doc(rnd, 9), doc(rnd, 3)]
  part.append(len(docs))
  return docs, part


def few_docs():
  """partitions of one and of two kept documents: the random-next draw's ten
  retries and is_random_next = False"""
  rnd = random.Random(5)
  docs = [doc(rnd, 12, 5, 60), doc(rnd, 9, 5, 60), doc(rnd, 7, 5, 60), doc(rnd, 1, 5, 60), doc(rnd, 1, 5, 9)]
  return docs, [0, 1, 3, 4, 5]


def long_sentence_docs():
  """512-token sentences at seq 128: every pair truncates several hundred
  steps, two MT words each, across many twists of the 624-word state"""
  rnd = random.Random(6)
  return [doc(rnd, 3, 512, 512) for _ in range(24)], [0, 10, 24]


CORPORA = dict(mixed=mixed_docs, doctable=doctable_docs, many=many_sentence_docs, dropped=dropped_docs,
               few=few_docs, long=long_sentence_docs)


@functools.lru_cache(maxsize=None)
def corpus(name):
  """corpus, partition offsets and the oracle's token ids, built once per name"""
  from lddl_amd import synth, pipeline
  docs, pdo = CORPORA[name]()
  c = synth.corpus_from_documents(docs)
  oids, ontok = OracleTokenizer(pipeline.VOCAB_BERT).run(c.data, c.sent_off, 512, nthreads=8)
  return c, np.asarray(pdo, dtype=np.int64), oids, ontok


def check(name, seq, dup, seed, bin_size=32, masking=False, spans=False, ratio=MASK[0]):
  from lddl_amd import pipeline
  c, pdo, oids, ontok = corpus(name)
  res = pipeline.run_bert(c, target_seq_length=seq, bin_size=bin_size, seed=seed, duplicate_factor=dup,
                          part_doc_off=pdo, check_host=True, masking=masking, masked_lm_ratio=ratio, spans=spans)
  assert res.spans == spans
  assert np.array_equal(res.ntok_host, ontok)
  exp = po.run_bert_shards(c, oids, ontok, pdo, seq, 0.1, dup, seed, bin_size,
                           masking=(ratio,) + MASK[1:] if masking else None)
  pipeline.assert_same_pairs(res, exp)  # A, B, is_random_next, num_tokens, in the binned shuffled order
  nb = res.nbins
  bc = res.bin_count.cpu().numpy()
  for p, part in enumerate(exp):
    assert np.array_equal(bc[p], np.bincount([po.bin_of(r[3], bin_size, nb) for r in part], minlength=nb)), p
  return res, exp


@pytest.mark.parametrize('seq', [128, 512])
def test_register_and_global_fill_documents(gpu, seq):
  _, exp = check('mixed', seq, 5, 77, bin_size=seq // 4)
  assert any(r[2] for part in exp for r in part) and any(not r[2] for part in exp for r in part)


def test_document_table_past_static_lds(gpu):
  c, pdo, oids, ontok = corpus('doctable')
  assert len(po.filtered_docs(oids, ontok, c.sent_off, c.doc_sent_off, 0, int(pdo[1]))) > 512
  check('doctable', 128, 5, 31)


def test_65536_kept_sentences(gpu):
  _, _, _, ontok = corpus('many')
  assert int((ontok > 0).sum()) >= 65536
  check('many', 128, 1, 9)


@pytest.mark.parametrize('spans', [False, True])
def test_dropped_sentences_and_documents(gpu, spans):
  """spans: the rows rebuilt from lddl_row_spans' src0 / src1 over the dense
  ids; otherwise the materialised rows' tokens"""
  c, pdo, _, ontok = corpus('dropped')
  assert (ontok == 0).sum() >= 15 and ontok[0] == 0 and ontok[-1] > 0
  res, _ = check('dropped', 128, 5, 5, spans=spans)
  if spans:  # the same tokens as the materialised rows
    from lddl_amd import pipeline
    m = pipeline.run_bert(c, target_seq_length=128, bin_size=32, seed=5, duplicate_factor=5, part_doc_off=pdo)
    assert np.array_equal(res.host_tokens(), m.host_tokens())
    assert np.array_equal(res.tok_off[:res.n_pairs + 1].cpu().numpy(), m.tok_off[:m.n_pairs + 1].cpu().numpy())


def test_dropped_sentences_seq512(gpu):
  check('dropped', 512, 5, 6, bin_size=64)


def test_one_and_two_document_partitions(gpu):
  _, exp = check('few', 128, 5, 11)
  assert exp[0] and not any(r[2] for r in exp[0])  # one document: never a random next
  assert any(r[2] for r in exp[1])  # two documents: the other one, most of the time


def test_truncation_across_twists(gpu):
  _, exp = check('long', 128, 5, 3)
  assert all(r[3] == 128 for part in exp for r in part)


@pytest.mark.parametrize('seed', [0, 2**32 - 2])
def test_seed_edges(gpu, seed):
  """seed + p on a second (and third) partition: 2**32 - 2 + p crosses the one-word key's end"""
  check('dropped', 128, 5, seed)
  check('mixed', 128, 5, seed)


def test_masked_on_dropped_corpus(gpu):
  check('dropped', 128, 5, 4242, masking=True)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('name,seq,dup,ratio', [('mixed', 128, 5, 0.15), ('doctable', 128, 5, 0.15),
                                                ('few', 128, 5, 0.15), ('long', 128, 5, 0.15),
                                                ('mixed', 512, 5, 0.15), ('long', 512, 5, 0.15),
                                                ('few', 128, 5, 1.0), ('long', 128, 5, 1.0)])
def test_masked_on_branch_corpora(gpu, name, seq, dup, ratio, spans):
  """the masked kernel on the corpora above: a slip in the draw accounting of
  the truncation ('long': hundreds of steps per pair) or of the random-next
  retries ('few') moves every later masking draw of the partition"""
  _, exp = check(name, seq, dup, 4242, bin_size=seq // 4, masking=True, spans=spans, ratio=ratio)
  assert all(r[4] for part in exp for r in part)  # words only: every row has a masked position
  if ratio == 1.0:
    assert all(len(r[4]) == r[3] - 3 for part in exp for r in part)


@pytest.mark.parametrize('spans', [False, True])
def test_masked_65536_kept_sentences(gpu, spans):
  """'many' masked: 66 200 sentences in one partition, so one wave packs them
  all (0.5 s on an MI355X, the oracle included)"""
  check('many', 128, 1, 4242, masking=True, spans=spans)
