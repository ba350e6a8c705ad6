"""The sentence-order packer (lddl_pack_sop, pack_sop_wave_kernel in
lddl_amd/csrc/pack_wave.hip) as an exact host model in plain Python over
``random``, and the hand-made corpora its tests pack.  Host only: nothing here
touches a GPU.

The reference has no such mode (half of its B segments come from a random
document), so there is no golden to take from it; the model is the row
definition of DESIGN.md ("Sentence-order rows"), built from the reference's
pieces in its draw order: random.seed(seed + p) per partition, the
short_seq_prob draw of create_pairs_from_document (pretrain.py:259-265), the A
split randint(1, n - 1) (:285-286), one random() < 0.5 for the exchange,
_truncate_seq_pair on the exchanged pair (:161-176), random.shuffle of the
partition's rows (:401) and the stable binning of binning.py:63-93.

A corpus is (docs, part_doc_off) as in tests/mlm_pack_model.py, whose
CountingRandom, build and bin_of this model uses.
"""
import collections
import functools
import random

from mlm_pack_model import CountingRandom, bin_of, build, _docs  # noqa: F401

Row = collections.namedtuple('Row', 'A B swap doc bin')  # doc: index into the corpus' documents
# what generate() notes per row for the host tests: the chunk's sentences, the split, the lengths before truncation
Trace = collections.namedtuple('Trace', 'doc chunk a_end swap la lb target')


def kept_documents(docs, pdo, p):
  """partition p's documents with their empty sentences dropped, those left
  with fewer than 2 sentences dropped -> [(document index, sentences)]"""
  out = []
  for d in range(pdo[p], pdo[p + 1]):
    sents = [list(s) for s in docs[d] if len(s) > 0]
    if len(sents) >= 2:
      out.append((d, sents))
  return out


def truncate_seq_pair(a, b, max_num, rnd):
  """pretrain.py:161-176"""
  while len(a) + len(b) > max_num:
    t = a if len(a) > len(b) else b
    assert len(t) >= 2  # the row definition's "no error path": no side is trimmed to nothing
    if rnd.random() < 0.5:
      del t[0]
    else:
      t.pop()


def generate(kept, seq, ssp, dup, rnd, trace=None):
  """the rows of one partition in generation order -> [(A, B, swap, doc)]"""
  rows = []
  max_num = seq - 3
  assert max_num >= 2
  for _ in range(dup):
    for d, doc in kept:
      target = max_num
      if rnd.random() < ssp:
        target = rnd.randint(2, max_num)
      chunk, cur = [], 0
      for i, sent in enumerate(doc):
        chunk.append(sent)
        cur += len(sent)
        if i == len(doc) - 1 or (cur >= target and len(chunk) >= 2):
          if len(chunk) >= 2:  # (a chunk of one sentence, the document's trailing one: no row, no draw)
            a_end = rnd.randint(1, len(chunk) - 1)
            swap = rnd.random() < 0.5
            a = [t for s in chunk[:a_end] for t in s]
            b = [t for s in chunk[a_end:] for t in s]
            if swap:
              a, b = b, a
            if trace is not None:
              trace.append(Trace(d, [list(s) for s in chunk], a_end, swap, len(a), len(b), target))
            truncate_seq_pair(a, b, max_num, rnd)
            assert len(a) >= 1 and len(b) >= 1
            rows.append((a, b, swap, d))
          chunk, cur = [], 0
  return rows


def pack_partition(docs, pdo, p, seq, ssp, dup, seed, bin_size=None, stats=None, trace=None):
  """partition p's rows in final order (shuffled, then grouped by bin) -> [Row]"""
  rnd = CountingRandom(seed + p)
  rows = generate(kept_documents(docs, pdo, p), seq, ssp, dup, rnd, trace)
  if stats is not None:
    stats.append((rnd.n_random, rnd.n_randint))
  rnd.shuffle(rows)
  nbins = seq // bin_size if bin_size else 1
  rows = [Row(a, b, s, d, bin_of(len(a) + len(b) + 3, bin_size, nbins) if bin_size else 0) for a, b, s, d in rows]
  return sorted(rows, key=lambda r: r.bin)  # (stable)


def pack(corpus, seq, ssp, dup, seed, bin_size=None, stats=None, trace=None):
  """-> per partition its [Row] in final order"""
  docs, pdo = corpus
  return [pack_partition(docs, pdo, p, seq, ssp, dup, seed, bin_size, stats, trace) for p in range(len(pdo) - 1)]


def bin_counts(parts, seq, bin_size):
  nbins = seq // bin_size if bin_size else 1
  return [[sum(1 for r in part if r.bin == b) for b in range(nbins)] for part in parts]


# ------------------------------------------------------------- corpora --
@functools.lru_cache(maxsize=None)
def corpus_small(n_part=5):
  """sentences of 1-6 tokens, 2-12 per document, and a few documents of
  exactly two sentences: several chunks per document at target_seq_length 16,
  chunks of exactly 2 sentences (randint(1, 1)) among them"""
  rnd = random.Random(7)
  return build([_docs(rnd, 6 + p, 2, 12, [1, 2, 3, 4, 5, 6]) + [[3, 4], [9, 9]] for p in range(n_part)])


@functools.lru_cache(maxsize=None)
def corpus_long_docs():
  """at target_seq_length 512, documents of far more than 64 kept sentences
  of 1-3 tokens (a chunk of ~250 sentences: the chunk scan goes on past its
  first 64 with find_over, a_end is drawn from a wide range), documents of
  exactly 64, 65 and 128 kept sentences, and one-sentence documents"""
  rnd = random.Random(8)
  p0 = [[rnd.choice([1, 2, 3]) for _ in range(700)], [5], [1] * 64, [1] * 65, [600], [0, 1] * 128,
        [2] * 130 + [509, 1], [8] * 63 + [3, 0, 1]]
  p1 = [[3], [rnd.choice([1, 2]) for _ in range(400)], [510], [511, 4], [1], [7] * 64, [7] * 65]
  return build([p0, p1])


# target_seq_length 16: max_num 13
def _pairs_trunc(order):
  """two-sentence documents (x, y) with an excess of x + y - 13 coins"""
  p = [(13, 1), (40, 36), (38, 39), (39, 39), (1, 141), (160, 170), (200, 200), (330, 5), (3, 330), (7, 7),
       (20, 2), (2, 20), (14, 14)]
  return [[a, b] if order else [b, a] for a, b in p]


@functools.lru_cache(maxsize=None)
def corpus_trunc():
  """pair truncation at target_seq_length 16 (max_num 13): an excess of 1,
  63, 64, 65, 129 and more than 312 coins in one partition (rounds are cut at
  the end of the MT19937 state, a coin straddles the twist); A longer than,
  equal to and shorter than B; and a first sentence alone >= target, flushed
  only with its successor ("at least 2 sentences")"""
  p0 = _pairs_trunc(True) + [[20, 1, 1, 1], [13, 13, 13], [15, 2, 16, 1, 30]]
  p1 = _pairs_trunc(False) + [[1, 1, 1, 20, 5]]
  p2 = [[50, 50]] * 5 + [[60, 41], [41, 60]] * 3
  return build([p0, p1, p2])


@functools.lru_cache(maxsize=None)
def corpus_filter():
  """empty sentences and empty documents at the start, middle and end of a
  partition, documents of exactly one kept sentence between others, a
  partition whose documents all drop between two that do not, a partition
  without documents, and a partition of more than 512 documents"""
  rnd = random.Random(9)
  p0 = [[], [0, 0], [0, 3, 0, 4, 0], [5], [], [0], [2, 0, 0, 6], [0, 0, 7], [4, 4, 4, 4, 4], [0, 8, 0], [3, 3, 0],
        [0], []]
  p1 = [[], [0, 0, 0], [0], [5], [0, 6, 0]]
  p2 = [[1, 2, 3], [7], [0, 9, 9, 0]]
  p3 = []
  p4 = [[rnd.choice([0, 1, 2, 5]) for _ in range(rnd.randint(0, 4))] for _ in range(600)]
  return build([p0, p1, p2, p3, p4])


@functools.lru_cache(maxsize=None)
def corpus_bins(seq):
  """row lengths across every bin of seq // 4 bins: documents of 2-9
  sentences whose lengths reach seq (packed with short_seq_prob 0.5)"""
  rnd = random.Random(10 + seq)
  lens = [1, 2, 3, 5, 8, 13, seq // 8, seq // 4, seq // 2, seq]
  return build([_docs(rnd, 40, 2, 9, lens) for _ in range(3)])


@functools.lru_cache(maxsize=None)
def corpus_rows():
  """about 200 rows at target_seq_length 32 / duplicate_factor 2 for the
  layers above the kernel: three partitions of ordinary documents"""
  rnd = random.Random(11)
  return build([_docs(rnd, 24, 2, 14, [1, 2, 3, 4, 6, 9, 12, 20]) for _ in range(3)])


@functools.lru_cache(maxsize=None)
def corpus_share():
  """more than 2000 rows at target_seq_length 16 for the swap share"""
  rnd = random.Random(12)
  return build([_docs(rnd, 150, 2, 12, [1, 2, 3, 4, 5, 6]) for _ in range(4)])
