"""The host model of the sentence-order packer (tests/sop_pack_model.py)
against a hand-computed case and its own invariants, and the host-only surface
of the feature: the --sop flag, its place in the resume key, and the refusals
of sop=True with masking, CodeBERT or nsp=False before a device is touched.
Nothing here needs a GPU."""
import math
import random

import pytest

import sop_pack_model as sm


# ---- the hand-computed case ---------------------------------------------------
# target_seq_length 9 (max_num 6), short_seq_prob 0, duplicate_factor 1, one partition.
#   doc 0  sentences of 7, 1, 2, 2, 3 tokens: the first alone holds >= 6 but a chunk needs 2 sentences, so
#          [7, 1] is flushed (8 tokens, 2 coins); then 2 + 2 + 3 = 7 >= 6 at the document's end (1 coin)
#   doc 1  one kept sentence (and an empty one): dropped, no draw
#   doc 2  sentences of 2, 4, 1: 2 + 4 = 6 flushes [2, 4] (no coin); the trailing [1] alone: no row, no draw
HAND = ([[[1000, 1001, 1002, 1003, 1004, 1005, 1006], [1007], [1008, 1009], [1010, 1011], [1012, 1013, 1014]],
         [[], [1015]],
         [[1016, 1017], [1018, 1019, 1020, 1021], [1022]]], [0, 3])


def _replay_hand(seed):
  """the row definition written out once more, draw by draw, on the stdlib generator"""
  r = random.Random(seed)
  toks = lambda lo, hi: list(range(lo, hi))  # noqa: E731
  # doc 0
  r.random()  # the short_seq draw (probability 0: no effect)
  out = []
  for chunk in ([toks(1000, 1007), toks(1007, 1008)], [toks(1008, 1010), toks(1010, 1012), toks(1012, 1015)]):
    a_end = r.randint(1, len(chunk) - 1)
    swap = r.random() < 0.5
    a = [t for s in chunk[:a_end] for t in s]
    b = [t for s in chunk[a_end:] for t in s]
    if swap:
      a, b = b, a
    while len(a) + len(b) > 6:
      t = a if len(a) > len(b) else b
      if r.random() < 0.5:
        del t[0]
      else:
        t.pop()
    out.append((a, b, swap, 0))
  # doc 2
  r.random()
  chunk = [toks(1016, 1018), toks(1018, 1022)]
  assert r.randint(1, 1) == 1  # drawn all the same
  swap = r.random() < 0.5
  a, b = chunk[0], chunk[1]
  if swap:
    a, b = b, a
  out.append((a, b, swap, 2))
  rows = list(out)
  r.shuffle(rows)
  return out, rows


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_hand_case(seed):
  kept = sm.kept_documents(*HAND, 0)
  assert [d for d, _ in kept] == [0, 2]
  rnd = sm.CountingRandom(seed)
  trace = []
  gen = sm.generate(kept, 9, 0.0, 1, rnd, trace)
  want_gen, want_rows = _replay_hand(seed)
  assert gen == want_gen
  # 2 document draws + 3 swaps + (2 + 1 + 0) coins; 3 a_end draws, the last one randint(1, 1)
  assert (rnd.n_random, rnd.n_randint) == (2 + 3 + 3, 3)
  assert [len(t.chunk) for t in trace] == [2, 3, 2]
  got = sm.pack(HAND, 9, 0.0, 1, seed)
  assert [[(r.A, r.B, r.swap, r.doc) for r in part] for part in got] == [want_rows]
  # every row keeps both sides and fits
  assert all(len(a) >= 1 and len(b) >= 1 and len(a) + len(b) <= 6 for a, b, _, _ in gen)
  # binned in 3 bins of 3: stable grouping of the shuffled order
  binned = sm.pack(HAND, 9, 0.0, 1, seed, bin_size=3)[0]
  flat = got[0]
  for b in range(3):
    assert [(r.A, r.B) for r in binned if r.bin == b] == [(r.A, r.B) for r in flat
                                                         if min((len(r.A) + len(r.B) + 2) // 3, 2) == b]
  assert [r.bin for r in binned] == sorted(r.bin for r in binned)


# ---- invariants over random corpora ---------------------------------------------
def _random_corpus(seed, longest):
  rnd = random.Random(seed)
  parts = [[[rnd.randint(0, longest) for _ in range(rnd.randint(0, 9))] for _ in range(rnd.randint(0, 12))]
           for _ in range(4)]
  return sm.build(parts)


def _is_sublist_at(hay, needle):
  n = len(needle)
  return any(hay[k:k + n] == needle for k in range(len(hay) - n + 1))


@pytest.mark.parametrize('seq,ssp,dup', [(16, 0.0, 1), (16, 0.5, 2), (16, 1.0, 3), (64, 0.1, 2), (5, 0.3, 2)])
def test_rows_and_draw_counts(seq, ssp, dup):
  """Undoing the swap, each side is a window of its own part of the chunk, and the chunk is a run of the document.
  The two sides together are ONE contiguous run only when the coins took tokens from the chunk's outer ends (or
  none): _truncate_seq_pair also trims the first part's back and the second part's front, so the stronger
  statement does not hold for every row, and is asserted where it applies."""
  max_num = seq - 3
  for cs in range(5):
    docs, pdo = _random_corpus(100 + cs, 40)
    for p in range(len(pdo) - 1):
      kept = sm.kept_documents(docs, pdo, p)
      rnd = sm.CountingRandom(77 + p)
      trace = []
      rows = sm.generate(kept, seq, ssp, dup, rnd, trace)
      assert len(rows) == len(trace)
      n_excess = 0
      for (a, b, swap, d), t in zip(rows, trace):
        assert d == t.doc and swap == t.swap and pdo[p] <= d < pdo[p + 1]
        assert len(a) >= 1 and len(b) >= 1 and len(a) + len(b) + 3 <= seq
        # unswap: first + second is a contiguous run of the document's token stream, the chunk short of trimmed ends
        first, second = (b, a) if swap else (a, b)
        l_first, l_second = (t.lb, t.la) if swap else (t.la, t.lb)
        chunk_toks = [x for s in t.chunk for x in s]
        assert l_first == sum(len(s) for s in t.chunk[:t.a_end]) and l_first + l_second == len(chunk_toks)
        # each side is a window of its own part of the chunk
        assert _is_sublist_at(chunk_toks[:l_first], first) and _is_sublist_at(chunk_toks[l_first:], second)
        if len(chunk_toks) <= max_num:
          assert first + second == chunk_toks
        doc_toks = [x for s in docs[d] for x in s]
        assert _is_sublist_at(doc_toks, chunk_toks)
        if first == chunk_toks[l_first - len(first):l_first] and second == chunk_toks[l_first:l_first + len(second)]:
          assert _is_sublist_at(doc_toks, first + second)  # only outer ends trimmed: one contiguous run
        n_excess += max(0, len(chunk_toks) - max_num)
        # the flush rule: >= 2 sentences; below the target before the last sentence unless the chunk has just two
        assert len(t.chunk) >= 2
        if len(t.chunk) > 2:
          assert sum(len(s) for s in t.chunk[:-1]) < t.target
      # the closed draw count: one random per document pass (+ a randint when it fell below short_seq_prob), one
      # randint + one random per row, one random per excess token
      visits = dup * len(kept)
      n_short = rnd.n_randint - len(rows)
      assert 0 <= n_short <= visits
      if ssp == 0.0:
        assert n_short == 0
      if ssp == 1.0:
        assert n_short == visits
      assert rnd.n_random == visits + len(rows) + n_excess
      assert 2 * len(rows) <= dup * sum(len(d) for _, d in kept)  # rows per pass <= kept sentences / 2


def test_contiguous_when_nothing_is_trimmed_inside():
  """a corpus that never truncates: undoing the swap gives the chunk itself, and a document's chunks in
  generation order tile the document up to a trailing one-sentence chunk"""
  docs, pdo = sm.build([[[2, 0, 3], [1], [], [4, 4, 4], [1, 1, 1, 1, 1]], [[5, 5], [6, 6, 1]]])
  for p in range(2):
    kept = sm.kept_documents(docs, pdo, p)
    rnd = sm.CountingRandom(3)
    rows = sm.generate(kept, 16, 0.0, 1, rnd)
    by_doc = {}
    for a, b, swap, d in rows:
      by_doc.setdefault(d, []).extend(b + a if swap else a + b)
    for d, doc in kept:
      full = [t for s in doc for t in s]
      assert by_doc[d] == full or by_doc[d] == full[:len(full) - len(doc[-1])]
    assert rnd.n_random == len(kept) + len(rows)


def test_no_rows_and_no_draws_from_single_sentences():
  # one-sentence documents only (after the filter): nothing is drawn at all
  docs, pdo = sm.build([[[5], [0, 3, 0], [], [0], [7]]])
  stats = []
  assert sm.pack((docs, pdo), 16, 1.0, 3, 1, stats=stats) == [[]]
  assert stats == [(0, 0)]
  # a trailing one-sentence chunk: [13, 1] is a row, the [4] behind it neither a row nor a draw
  docs, pdo = sm.build([[[13, 1, 4]]])
  stats, trace = [], []
  rows = sm.pack((docs, pdo), 16, 0.0, 1, 1, stats=stats, trace=trace)[0]
  assert len(rows) == 1 and [len(s) for s in trace[0].chunk] == [13, 1]
  assert stats == [(1 + 1 + 1, 1)]  # document draw, swap, one coin (14 tokens > 13); a_end
  # the same stream position afterwards as a document without the trailing sentence
  docs2, pdo2 = sm.build([[[13, 1]]])
  stats2 = []
  rows2 = sm.pack((docs2, pdo2), 16, 0.0, 1, 1, stats=stats2)[0]
  assert stats2 == stats and [(r.A, r.B, r.swap) for r in rows2] == [(r.A, r.B, r.swap) for r in rows]


SHARE_SEED = 21


def test_swap_share():
  """the swap is a fair coin: over n rows its share lies within 4 standard deviations of 1/2 (binomial:
  sd = sqrt(0.25 / n)), a bound derived from the draw, not from the outcome"""
  rows = [r for part in sm.pack(sm.corpus_share(), 16, 0.1, 2, SHARE_SEED) for r in part]
  n = len(rows)
  assert n >= 2000
  share = sum(r.swap for r in rows) / n
  assert abs(share - 0.5) <= 4 * math.sqrt(0.25 / n), (share, n)


def test_regime_corpora_reach_their_regimes():
  """what tests/test_pack_sop_gpu.py relies on"""
  # chunks of exactly two sentences among several chunks per document
  trace = []
  sm.pack(sm.corpus_small(5), 16, 0.1, 2, 12345, trace=trace)
  assert sum(len(t.chunk) == 2 for t in trace) > 10 and sum(len(t.chunk) > 2 for t in trace) > 10
  by_doc = {}
  for t in trace:
    by_doc[t.doc] = by_doc.get(t.doc, 0) + 1
  assert max(by_doc.values()) >= 4
  # chunks of more than 64 sentences, a_end from a wide range, documents of 64 / 65 / 128 kept sentences
  docs, pdo = sm.corpus_long_docs()
  kept_n = [len([s for s in d if s]) for d in docs]
  assert {64, 65, 128} <= set(kept_n) and max(kept_n) > 64 * 4 and 1 in kept_n
  for ssp in (0.0, 0.5):
    trace = []
    sm.pack(sm.corpus_long_docs(), 512, ssp, 2, 7, trace=trace)
    assert sum(len(t.chunk) > 64 for t in trace) >= 4 and sum(len(t.chunk) > 128 for t in trace) >= 2
    assert any(t.a_end > 64 for t in trace)
    assert any(len(t.chunk) == 64 for t in trace) and any(len(t.chunk) == 65 for t in trace)
  # truncation: the listed excesses, > 312 coins per partition, every order of the lengths swapped and not
  for seed in (3, 4):
    seen, excess = set(), set()
    for ssp, dup in ((0.0, 2), (0.3, 1)):
      stats, trace = [], []
      sm.pack(sm.corpus_trunc(), 16, ssp, dup, seed, stats=stats, trace=trace)
      assert all(n > 312 for n, _ in stats)  # every partition's coins cross the end of an MT19937 state
      for t in trace:
        seen.add(((t.la > t.lb) - (t.la < t.lb), t.swap))
        excess.add(t.la + t.lb - 13)
      if ssp == 0.0:
        assert {1, 63, 64, 65, 129} <= excess and max(excess) > 312
        assert any(len(t.chunk) == 2 and len(t.chunk[0]) >= t.target for t in trace)
    assert seen == {(c, s) for c in (-1, 0, 1) for s in (False, True)}, (seed, seen)
  docs, pdo = sm.corpus_filter()
  assert pdo[5] - pdo[4] > 512 and pdo[4] == pdo[3]
  parts = sm.pack(sm.corpus_filter(), 16, 0.1, 2, 5, bin_size=4)
  assert parts[1] == [] and parts[3] == [] and parts[0] and parts[2] and parts[4]
  assert any(len([s for s in d if s]) == 1 for d in docs[pdo[0] + 1:pdo[1] - 1])
  for seq in (16, 128, 512):
    parts = sm.pack(sm.corpus_bins(seq), seq, 0.5, 1, 1, bin_size=4)
    assert {r.bin for part in parts for r in part} >= {1, seq // 8, seq // 4 - 1}
  n = sum(len(p) for p in sm.pack(sm.corpus_rows(), 32, 0.1, 2, 21, bin_size=8))
  assert 150 <= n <= 300
  # the smallest target: every row is trimmed to one token a side
  rows = [r for part in sm.pack(sm.corpus_small(5), 5, 0.5, 1, 2) for r in part]
  assert rows and all(len(r.A) == 1 and len(r.B) == 1 for r in rows)


# ---- host-only surface ------------------------------------------------------------
def test_cli_flag():
  from lddl_amd import preprocess
  assert preprocess.parse_args(['--sink', 'x']).sop is False
  assert preprocess.parse_args(['--sink', 'x', '--sop']).sop is True
  assert preprocess.parse_args(['--sink', 'x', '--sop', '--output-format', 'txt']).sop is True
  with pytest.raises(SystemExit):
    preprocess.parse_args(['--sink', 'x', '--sop', '--masking'])
  with pytest.raises(SystemExit):
    preprocess.parse_args(['--sink', 'x', '--sop', '--no-nsp'])
  with pytest.raises(SystemExit):  # the BERT sub-command's flag only
    preprocess.parse_args(['--sink', 'x', '--sop'], codebert=True)
  args = preprocess.parse_args(['--sink', 'x', '--sop'])
  args.masking = True  # (a caller of main() with its own namespace)
  with pytest.raises(ValueError, match='--sop'):
    preprocess._check(args)
  args.masking, args.nsp = False, False
  with pytest.raises(ValueError, match='--sop'):
    preprocess._check(args)


def test_resume_key(tmp_path):
  from lddl_amd import preprocess
  from lddl_amd.pipeline import VOCAB_BERT
  f = tmp_path / 'in.txt'
  f.write_text('x')
  key = lambda argv: preprocess.run_key(preprocess.parse_args(argv), False, [str(f)], VOCAB_BERT, 'rules', 3)  # noqa: E731
  assert key(['--sink', 'x']) != key(['--sink', 'x', '--sop'])
  assert key(['--sink', 'x', '--sop']) != key(['--sink', 'x', '--no-nsp'])
  # a run without the flag keeps the key it had before the flag existed
  plain = preprocess.parse_args(['--sink', 'x'])
  del plain.sop
  assert preprocess.run_key(plain, False, [str(f)], VOCAB_BERT, 'rules', 3) == key(['--sink', 'x'])


def test_pack_refusals_touch_no_device():
  from lddl_amd import pipeline
  pk = pipeline.Packer.__new__(pipeline.Packer)  # no ctx, no device: the refusal comes before either is needed
  for bad in (dict(masking=True), dict(codebert=True), dict(nsp=False)):
    with pytest.raises(ValueError, match='sop=True'):
      pk.pack(None, None, None, sop=True, **bad)
    with pytest.raises(ValueError, match='sop=True'):
      pipeline.run_bert(None, sop=True, device='none', **bad)
