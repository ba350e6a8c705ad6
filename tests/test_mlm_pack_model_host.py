"""The host model of the MLM-only packer (tests/mlm_pack_model.py) against a
hand-computed case and its own invariants, and the host-only surface of the
feature: the shard schema, the --nsp / --no-nsp flag, the refusals of
nsp=False with masking or CodeBERT before a device is touched, and the
shard-kind messages of the loader classes.  Nothing here needs a GPU."""
import os
import random

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import mlm_pack_model as mm


# ---- the hand-computed case ---------------------------------------------------
# target_seq_length 8 (max_num 6), short_seq_prob 0, duplicate_factor 1, seed 5, one partition.
#   doc 0  sentences of 2, 4, 3, 1 tokens: 2 + 4 = 6 >= 6 flushes [1000..1005]; 3 + 1 = 4 flushes at the end
#   doc 1  an empty document: dropped, no draw
#   doc 2  one sentence of 1 token (after an empty one): [1010]
#   doc 3  one sentence of 8 tokens [1011..1018]: two coins cut it to a window of 6
HAND = ([[[1000, 1001], [1002, 1003, 1004, 1005], [1006, 1007, 1008], [1009]],
         [[], []],
         [[], [1010]],
         [[1011, 1012, 1013, 1014, 1015, 1016, 1017, 1018]]], [0, 4])
# generation order: random.Random(5) gives 0.62, 0.74, 0.80 (the three kept documents' short_seq draws: no effect at
# probability 0), then the coins 0.94 and 0.74 (both >= 0.5: the last token goes, twice)
HAND_GENERATED = [([1000, 1001, 1002, 1003, 1004, 1005], 0), ([1006, 1007, 1008, 1009], 0), ([1010], 2),
                  ([1011, 1012, 1013, 1014, 1015, 1016], 3)]
# random.shuffle of those four after the five draws leaves the order 2, 3, 1, 0
HAND_ROWS = [([1010], 2), ([1011, 1012, 1013, 1014, 1015, 1016], 3), ([1006, 1007, 1008, 1009], 0),
             ([1000, 1001, 1002, 1003, 1004, 1005], 0)]
# bin_size 4: num_tokens 3, 8, 6, 8 -> bins 0, 1, 1, 1 (8 tokens: (8 - 1) // 4 = 1, the last bin)
HAND_BINS = [0, 1, 1, 1]


def test_hand_case_generation():
  kept = mm.kept_documents(*HAND, 0)
  assert [d for d, _ in kept] == [0, 2, 3] and kept[1][1] == [[1010]]
  rnd = mm.CountingRandom(5)
  assert mm.generate(kept, 8, 0.0, 1, rnd) == HAND_GENERATED
  assert (rnd.n_random, rnd.n_randint) == (3 + 2, 0)
  # the draws themselves, from the stdlib generator the way the reference seeds it
  random.seed(5)
  d = [random.random() for _ in range(5)]
  assert [round(x, 2) for x in d] == [0.62, 0.74, 0.80, 0.94, 0.74]
  order = [0, 1, 2, 3]
  random.shuffle(order)
  assert order == [2, 3, 1, 0]


def test_hand_case_rows():
  rows = mm.pack(HAND, 8, 0.0, 1, 5)
  assert [[(r.toks, r.doc, r.bin) for r in part] for part in rows] == [[t + (0,) for t in HAND_ROWS]]
  binned = mm.pack(HAND, 8, 0.0, 1, 5, bin_size=4)
  assert [[(r.toks, r.doc, r.bin) for r in part] for part in binned] == [[t + (b,) for t, b in zip(HAND_ROWS, HAND_BINS)]]
  assert mm.bin_counts(binned, 8, 4) == [[1, 3]]
  # a seed whose shuffle leaves bin 1's rows in front of bin 0's: the grouping moves them, stably
  other = mm.pack(HAND, 8, 0.0, 1, 6, bin_size=4)[0]
  flat = mm.pack(HAND, 8, 0.0, 1, 6)[0]
  assert [r.toks for r in other] == [r.toks for r in flat if len(r.toks) + 2 <= 4] + [r.toks for r in flat
                                                                                    if len(r.toks) + 2 > 4]


# ---- invariants over random corpora ---------------------------------------------
def _random_corpus(seed, longest):
  rnd = random.Random(seed)
  parts = [[[rnd.randint(0, longest) for _ in range(rnd.randint(0, 9))] for _ in range(rnd.randint(0, 12))]
           for _ in range(4)]
  return mm.build(parts)


@pytest.mark.parametrize('seq,ssp,dup', [(16, 0.0, 1), (16, 0.5, 2), (16, 1.0, 3), (64, 0.1, 2), (5, 0.3, 2)])
def test_row_lengths_and_draw_counts(seq, ssp, dup):
  for cs in range(5):
    docs, pdo = corpus = _random_corpus(100 + cs, 40)
    stats = []
    parts = mm.pack(corpus, seq, ssp, dup, 77, bin_size=None, stats=stats)
    for p, rows in enumerate(parts):
      assert all(1 <= len(r.toks) <= seq - 2 for r in rows)
      assert all(pdo[p] <= r.doc < pdo[p + 1] for r in rows)
      # the pseudo-code's draws, replayed with the model's decisions: one random() per kept document visit, one
      # randint per visit whose draw fell below short_seq_prob, one random() per excess token
      kept = mm.kept_documents(docs, pdo, p)
      rnd = random.Random(77 + p)
      n_random = n_randint = 0
      for _ in range(dup):
        for _, doc in kept:
          n_random += 1
          target = seq - 2
          if rnd.random() < ssp:
            n_randint += 1
            target = rnd.randint(2, seq - 2)
          cur = 0
          for i, s in enumerate(doc):
            cur += len(s)
            if i == len(doc) - 1 or cur >= target:
              for _ in range(max(0, cur - (seq - 2))):
                n_random += 1
                rnd.random()
              cur = 0
      assert stats[p] == (n_random, n_randint)
      assert len(rows) <= dup * sum(len(d) for _, d in kept)  # the kernel's record slots


def test_documents_are_covered_without_truncation():
  """short_seq_prob 0 and no sentence longer than max_num: a document's rows in generation order concatenate to
  the document -- unless a chunk overflows max_num, which only a flush at >= target can do (by < one sentence)"""
  for cs in range(5):
    docs, pdo = _random_corpus(200 + cs, 3)
    for p in range(len(pdo) - 1):
      kept = mm.kept_documents(docs, pdo, p)
      rnd = mm.CountingRandom(9)
      rows = mm.generate(kept, 64, 0.0, 1, rnd)  # sentences of <= 3 tokens never push a chunk past 62 by more than 2
      by_doc = {}
      for toks, d in rows:
        by_doc.setdefault(d, []).extend(toks)
      # a chunk reaches >= 62 with sentences of <= 3 tokens: at most 64 tokens, so up to 2 coins; exclude those
      if rnd.n_random == len(kept):
        assert by_doc == {d: [t for s in doc for t in s] for d, doc in kept}
  # and a corpus that provably never truncates: every document shorter than max_num
  docs, pdo = mm.build([[[2, 0, 3], [1], [], [4, 4, 4]], [[5, 5]]])
  for p in range(2):
    kept = mm.kept_documents(docs, pdo, p)
    rnd = mm.CountingRandom(3)
    rows = mm.generate(kept, 16, 0.0, 1, rnd)
    assert rnd.n_random == len(kept)
    assert [(t, d) for t, d in rows] == [([t for s in doc for t in s], d) for d, doc in kept]


def test_regime_corpora_reach_their_regimes():
  """what tests/test_pack_mlm_gpu.py relies on"""
  docs, pdo = mm.corpus_long_docs()
  assert max(len([s for s in d if s]) for d in docs) > 64 * 4 and any(len(d) == 1 for d in docs)
  assert any(len(r.toks) == 510 for part in mm.pack(mm.corpus_long_docs(), 512, 0.0, 1, 0) for r in part)
  stats = []
  mm.pack(mm.corpus_trunc(), 16, 0.0, 1, 3, stats=stats)
  assert all(n > 312 for n, _ in stats)  # every partition's coins cross the end of an MT19937 state
  docs, pdo = mm.corpus_filter()
  assert pdo[5] - pdo[4] > 512 and pdo[4] == pdo[3]
  parts = mm.pack(mm.corpus_filter(), 16, 0.1, 1, 0)
  assert parts[1] == [] and parts[3] == [] and parts[0] and parts[2] and parts[4]
  for seq in (16, 128, 512):
    parts = mm.pack(mm.corpus_bins(seq), seq, 0.5, 1, 1, bin_size=4)
    assert {r.bin for part in parts for r in part} >= {0, seq // 8, seq // 4 - 1}
  n = sum(len(p) for p in mm.pack(mm.corpus_rows(), 32, 0.1, 2, 21, bin_size=8))
  assert 150 <= n <= 300


# ---- host-only surface ------------------------------------------------------------
def test_schema_nsp_false():
  from lddl_amd import writer
  assert writer.schema(nsp=False) == pa.schema([('A', pa.string()), ('num_tokens', pa.uint16())])
  assert writer.schema(nsp=False, binned=True) == pa.schema([('A', pa.string()), ('num_tokens', pa.uint16()),
                                                            ('bin_id', pa.int64())])
  assert writer.schema().names == ['A', 'B', 'is_random_next', 'num_tokens']  # unchanged
  with pytest.raises(ValueError):
    writer.schema(nsp=False, masking=True)
  with pytest.raises(ValueError):
    writer.schema(nsp=False, codebert=True)
  with pytest.raises(ValueError):
    writer.write_txt(None, None, '/nonexistent', nsp=False)


def test_cli_flag():
  from lddl_amd import preprocess
  assert preprocess.parse_args(['--sink', 'x']).nsp is True
  assert preprocess.parse_args(['--sink', 'x', '--nsp']).nsp is True
  assert preprocess.parse_args(['--sink', 'x', '--no-nsp']).nsp is False
  with pytest.raises(SystemExit):
    preprocess.parse_args(['--sink', 'x', '--no-nsp', '--masking'])
  with pytest.raises(SystemExit):
    preprocess.parse_args(['--sink', 'x', '--no-nsp', '--output-format', 'txt'])
  assert preprocess.parse_args(['--sink', 'x', '--masking']).masking is True
  with pytest.raises(SystemExit):  # the BERT sub-command's flag only
    preprocess.parse_args(['--sink', 'x', '--no-nsp'], codebert=True)
  args = preprocess.parse_args(['--sink', 'x', '--no-nsp'])
  args.masking = True  # (a caller of main() with its own namespace)
  with pytest.raises(ValueError, match='--no-nsp'):
    preprocess._check(args)


def test_resume_key_separates_kinds(tmp_path):
  from lddl_amd import preprocess
  from lddl_amd.pipeline import VOCAB_BERT
  f = tmp_path / 'in.txt'
  f.write_text('x')
  a = preprocess.parse_args(['--sink', 'x'])
  b = preprocess.parse_args(['--sink', 'x', '--no-nsp'])
  ka, kb = (preprocess.run_key(x, False, [str(f)], VOCAB_BERT, 'rules', 3) for x in (a, b))
  assert ka != kb
  assert ka == preprocess.run_key(preprocess.parse_args(['--sink', 'x', '--nsp']), False, [str(f)], VOCAB_BERT,
                                  'rules', 3)


def test_pack_refusals_touch_no_device():
  from lddl_amd import pipeline
  pk = pipeline.Packer.__new__(pipeline.Packer)  # no ctx, no device: the refusal comes before either is needed
  with pytest.raises(ValueError, match='nsp=False'):
    pk.pack(None, None, None, nsp=False, masking=True)
  with pytest.raises(ValueError, match='nsp=False'):
    pk.pack(None, None, None, nsp=False, codebert=True)
  with pytest.raises(ValueError, match='nsp=False'):
    pipeline.run_bert(None, nsp=False, masking=True, device='none')
  with pytest.raises(ValueError, match='nsp=False'):
    pipeline.run_bert(None, nsp=False, codebert=True, device='none')
  assert pipeline.PackResult(0, 0, 1, None, None, None, None, None, None, None, None).kind == 'bert'


def _mlm_table(n=3):
  return pa.table({'A': ['the cat', 'a', 'b c d'][:n], 'num_tokens': pa.array([4, 3, 5][:n], pa.uint16())})


def _bert_table():
  return pa.table({'A': ['the cat'], 'B': ['sat'], 'is_random_next': [False], 'num_tokens': pa.array([6], pa.uint16())})


def test_shard_kind_messages(tmp_path):
  from lddl_amd import loader
  assert loader.MlmCollate.SHARD_COLUMNS == ('A', 'num_tokens')
  assert issubclass(loader.MlmCollate, loader.CodeCollate) and loader.MlmCollate.CODE
  assert loader.MlmCollate.VOCAB == loader.BertCollate.VOCAB
  with pytest.raises(ValueError, match='MlmCollate'):  # BertCollate.load_rows on an MLM-only shard
    loader._shard_columns(_mlm_table())
  with pytest.raises(ValueError, match='BertCollate'):  # MlmCollate.load_rows on a BERT shard
    loader._mlm_shard_columns(_bert_table())
  with pytest.raises(ValueError, match='CodeCollate'):
    loader._mlm_shard_columns(pa.table({'doc': ['a'], 'code': ['b'], 'num_tokens': pa.array([5], pa.uint16())}))
  cols, nt = loader._mlm_shard_columns([_mlm_table(2), _mlm_table(3)])
  assert nt.tolist() == [4, 3, 4, 3, 5] and nt.dtype == np.uint16
  assert cols[0][0].size == 0 and cols[0][1].tolist() == [0] * 6  # the empty doc column
  assert bytes(cols[1][0]) == b'the cata' + b'the catab c d' and cols[1][1].tolist() == [0, 7, 8, 15, 16, 21]
  # load_shards refuses by the columns, before the collate is used
  d = tmp_path / 'mlm'
  d.mkdir()
  pq.write_table(_mlm_table(), str(d / 'part.0.parquet'))

  class Shell:  # a collate's class attributes without its ctx
    def __init__(self, cls):
      self.SHARD_COLUMNS, self.SHARD_KIND, self.OTHER_SHARDS = cls.SHARD_COLUMNS, cls.SHARD_KIND, cls.OTHER_SHARDS

  with pytest.raises(ValueError, match='MlmCollate'):
    loader.load_shards(Shell(loader.BertCollate), str(d))
  with pytest.raises(ValueError, match='not a CodeBERT shard'):
    loader.load_shards(Shell(loader.CodeCollate), str(d))


def test_bert_collate_refuses_mlm_result_on_the_host():
  from lddl_amd import loader, pipeline
  res = pipeline.PackResult(1, 3, 1, None, None, None, None, None, None, None, None, kind='mlm')
  col = loader.BertCollate.__new__(loader.BertCollate)
  for who in ('collate_rows', 'collate_rows_unpadded'):
    with pytest.raises(ValueError, match='MlmCollate'):
      getattr(col, who)(res, [0])


def test_balancer_keeps_mlm_schema_and_rows(tmp_path):
  """the load balancer copies whatever columns a shard has: a binned MLM-only directory keeps its schema and,
  per bin, its row multiset"""
  from lddl_amd import balance, writer
  rnd = random.Random(4)
  ind, outd = tmp_path / 'in', tmp_path / 'out'
  ind.mkdir()
  sch = writer.schema(nsp=False, binned=True)
  rows = {0: [], 1: []}
  for p in range(3):
    for b in range(2):
      n = rnd.randint(0, 9)
      a = ['w%d_%d_%d' % (p, b, k) for k in range(n)]
      nt = [rnd.randint(3, 16) for _ in range(n)]
      rows[b] += list(zip(a, nt))
      pq.write_table(pa.table({'A': pa.array(a, pa.string()), 'num_tokens': pa.array(nt, pa.uint16()),
                               'bin_id': pa.array([b] * n, pa.int64())}, schema=sch),
                     str(ind / ('part.%d.parquet_%d' % (p, b))))
  balance.main(balance.attach_args().parse_args(['--indir', str(ind), '--outdir', str(outd), '--num-shards', '2',
                                                 '--keep-orig']), rank=0, world=1)
  got = {0: [], 1: []}
  for name in sorted(os.listdir(str(outd))):
    if '.parquet' not in name:
      continue
    t = pq.read_table(str(outd / name))
    assert t.schema.equals(sch), name
    b = int(name.rsplit('_', 1)[1])
    assert set(t.column('bin_id').to_pylist()) <= {b}
    got[b] += list(zip(t.column('A').to_pylist(), t.column('num_tokens').to_pylist()))
  assert {b: sorted(v) for b, v in got.items()} == {b: sorted(v) for b, v in rows.items()}
