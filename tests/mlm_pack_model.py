"""The MLM-only packer (lddl_pack_mlm, pack_mlm_wave_kernel in
lddl_amd/csrc/pack_wave.hip) as an exact host model in plain Python over
``random``, and the hand-made corpora its tests pack.  Host only: nothing here
touches a GPU.

The reference has no such mode, so there is no golden to take from it; the
model is the row definition of DESIGN.md ("MLM-only rows"), built from the
reference's pieces in its draw order: random.seed(seed + p) per partition, the
short_seq_prob draw of create_pairs_from_document (pretrain.py:259-265), one
random() coin per excess token (:161-179), random.shuffle of the partition's
rows (:401) and the stable binning of binning.py:63-93.

A corpus is (docs, part_doc_off): documents as lists of sentences (id lists,
empty ones included) and the partitions as document ranges, the form
tests/codebert_regimes.py uses and test_pack_gpu.shards_from_docs uploads.
"""
import collections
import functools
import random

Row = collections.namedtuple('Row', 'toks doc bin')  # doc: index into the corpus' documents


class CountingRandom:
  """random.Random(seed) behind a count of the model's calls: random() and
  randint().  (A wrapper, not a subclass: a subclass that overrides random()
  makes CPython draw randint and shuffle from random() instead of
  getrandbits(), another stream than ``random.seed(seed)`` gives.)"""

  def __init__(self, seed):
    self.r = random.Random(seed)
    self.n_random = self.n_randint = 0

  def random(self):
    self.n_random += 1
    return self.r.random()

  def randint(self, a, b):
    self.n_randint += 1
    return self.r.randint(a, b)

  def shuffle(self, x):
    self.r.shuffle(x)


def bin_of(num_tokens, bin_size, nbins):
  return min((num_tokens - 1) // bin_size, nbins - 1)


def kept_documents(docs, pdo, p):
  """partition p's documents with their empty sentences dropped, those left
  without a sentence dropped -> [(document index, sentences)]"""
  out = []
  for d in range(pdo[p], pdo[p + 1]):
    sents = [list(s) for s in docs[d] if len(s) > 0]
    if sents:
      out.append((d, sents))
  return out


def generate(kept, seq, ssp, dup, rnd):
  """the rows of one partition in generation order -> [(toks, doc)]"""
  rows = []
  for _ in range(dup):
    for d, doc in kept:
      max_num = seq - 2
      target = max_num
      if rnd.random() < ssp:
        target = rnd.randint(2, max_num)
      chunk, cur = [], 0
      for i, sent in enumerate(doc):
        chunk.append(sent)
        cur += len(sent)
        if i == len(doc) - 1 or cur >= target:
          toks = [t for s in chunk for t in s]
          while len(toks) > max_num:  # one random() per excess token
            if rnd.random() < 0.5:
              del toks[0]
            else:
              toks.pop()
          rows.append((toks, d))
          chunk, cur = [], 0
  return rows


def pack_partition(docs, pdo, p, seq, ssp, dup, seed, bin_size=None, stats=None):
  """partition p's rows in final order (shuffled, then grouped by bin) -> [Row]"""
  rnd = CountingRandom(seed + p)
  rows = generate(kept_documents(docs, pdo, p), seq, ssp, dup, rnd)
  if stats is not None:
    stats.append((rnd.n_random, rnd.n_randint))
  rnd.shuffle(rows)
  nbins = seq // bin_size if bin_size else 1
  rows = [Row(t, d, bin_of(len(t) + 2, bin_size, nbins) if bin_size else 0) for t, d in rows]
  return sorted(rows, key=lambda r: r.bin)  # (stable)


def pack(corpus, seq, ssp, dup, seed, bin_size=None, stats=None):
  """-> per partition its [Row] in final order"""
  docs, pdo = corpus
  return [pack_partition(docs, pdo, p, seq, ssp, dup, seed, bin_size, stats) for p in range(len(pdo) - 1)]


def bin_counts(parts, seq, bin_size):
  nbins = seq // bin_size if bin_size else 1
  return [[sum(1 for r in part if r.bin == b) for b in range(nbins)] for part in parts]


# ------------------------------------------------------------- corpora --
class _Ids:
  """token ids 1000, 1001, ... (mod 29000: below the BERT vocabulary's 30522
  and above its special tokens), so that a row names its place in the corpus"""

  def __init__(self):
    self.n = 0

  def __call__(self, n):
    out = [1000 + (self.n + k) % 29000 for k in range(n)]
    self.n += n
    return out


def build(parts):
  """[[sentence lengths per document] per partition] -> (docs, part_doc_off)"""
  ids = _Ids()
  docs, pdo = [], [0]
  for part in parts:
    for d in part:
      docs.append([ids(n) for n in d])
    pdo.append(len(docs))
  return docs, pdo


def _docs(rnd, n, smin, smax, lens):
  return [[rnd.choice(lens) for _ in range(rnd.randint(smin, smax))] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def corpus_small(n_part=5):
  """(a), (e): sentences of 1-6 tokens, 3-12 per document: several chunks per
  document at target_seq_length 16"""
  rnd = random.Random(7)
  return build([_docs(rnd, 6 + p, 3, 12, [1, 2, 3, 4, 5, 6]) for p in range(n_part)])


@functools.lru_cache(maxsize=None)
def corpus_long_docs():
  """(b): at target_seq_length 512, documents of far more than 64 kept
  sentences of 1-3 tokens (a chunk of ~250 sentences: find_over runs several
  rounds), a document of exactly 64 and of 65, and one-sentence documents"""
  rnd = random.Random(8)
  p0 = [[rnd.choice([1, 2, 3]) for _ in range(700)], [5], [1] * 64, [1] * 65, [600], [2] * 130 + [509, 1]]
  p1 = [[3], [rnd.choice([1, 2]) for _ in range(400)], [510], [511], [1]]
  return build([p0, p1])


@functools.lru_cache(maxsize=None)
def corpus_trunc():
  """(c): at target_seq_length 16 (max_num 14), sentences with 1 .. 300 excess
  tokens: rounds of 64 coins, and > 312 coins in a partition, so that rounds
  are cut at the end of the MT19937 state and a coin straddles the twist (a
  document's own draw shifts the parity)"""
  p0 = [[14 + 65], [14 + 64], [14 + 1], [3, 14 + 200], [14 + 129, 2], [14], [15], [14 + 300], [7, 7, 14 + 63]]
  p1 = [[14 + 310], [14 + 64], [14 + 65], [2, 2], [14 + 311], [14 + 70]]
  p2 = [[14 + 100]] * 9
  return build([p0, p1, p2])


@functools.lru_cache(maxsize=None)
def corpus_filter():
  """(d): empty sentences and empty documents at the start, middle and end of
  a partition, an all-empty partition between two others, a partition without
  documents, and a partition of more than 512 documents"""
  rnd = random.Random(9)
  p0 = [[], [0, 0], [0, 3, 0, 4, 0], [5], [], [0], [2, 0, 0, 6], [0, 0, 7], [4, 4, 4, 4, 4], [0], []]
  p1 = [[], [0, 0, 0], [0]]
  p2 = [[1, 2, 3], [0, 9, 9, 0]]
  p3 = []
  p4 = [[rnd.choice([0, 1, 2, 5]) for _ in range(rnd.randint(0, 3))] for _ in range(600)]
  return build([p0, p1, p2, p3, p4])


@functools.lru_cache(maxsize=None)
def corpus_bins(seq):
  """(f): row lengths across every bin of seq // 4 bins: documents of 1-9
  sentences whose lengths reach seq (packed with short_seq_prob 0.5)"""
  rnd = random.Random(10 + seq)
  lens = [1, 2, 3, 5, 8, 13, seq // 8, seq // 4, seq // 2, seq]
  return build([_docs(rnd, 40, 1, 9, lens) for _ in range(3)])


@functools.lru_cache(maxsize=None)
def corpus_rows():
  """about 200 rows at target_seq_length 32 / duplicate_factor 2 for the
  layers above the kernel: three partitions of ordinary documents"""
  rnd = random.Random(11)
  return build([_docs(rnd, 17, 2, 14, [1, 2, 3, 4, 6, 9, 12, 20]) for _ in range(3)])
