"""The BART aggregation rule on the host: tests/bart_model.py equals the
reference's own `_generate_sequences` (tests/golden/bart_chunks.json.gz, made
by tools/gen_golden_bart.py from lddl/dask/bart/pretrain.py:82-133) on the
stripped, non-empty sentences of every golden article, and the CLI's `bart`
sub-command has the reference's flags (bart/pretrain.py:187-286)."""
import functools
import gzip
import json
import os

import numpy as np
import pytest

import bart_model as bm
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def golden_bart():
  with gzip.open(os.path.join(GOLDEN, 'bart_chunks.json.gz'), 'rt') as f:
    return json.load(f)


def golden_docs():
  """the golden articles as the front end hands them over: per article its
  stripped, non-empty sentences (bart/pretrain.py:82-86)"""
  return [[p.strip() for p in a.split('\x01') if p.strip()] for a in golden_bart()['articles']]


def test_golden_covers_what_it_should():
  g = golden_bart()
  assert sorted(map(int, g['results'])) == [3, 4, 8, 128, 512]
  assert 200 <= len(g['articles']) <= 400
  text = '\x01'.join(g['articles'])
  spaces = [chr(c) for c in range(0x3001) if chr(c).isspace()]
  assert len(spaces) == 29 and all(c in text for c in spaces)
  words = [len(s.split()) for d in golden_docs() for s in d]
  assert 1 in words and max(words) > 509  # single-word sentences, one sentence longer than any T
  assert any(' ' * 64 in a for a in g['articles']) and any('中' in a for a in g['articles'])
  assert any(p != p.strip() for a in g['articles'] for p in a.split('\x01'))
  assert any(p == '' for a in g['articles'] for p in a.split('\x01'))
  assert any(p != '' and p.strip() == '' for a in g['articles'] for p in a.split('\x01'))


@pytest.mark.parametrize('tsl', [3, 4, 8, 128, 512])
def test_model_equals_reference(tsl):
  g = golden_bart()
  docs = golden_docs()
  data, so, dso = bm.table(docs)
  pl, chunks = bm.aggregate(data, so, dso, tsl - 3)
  want = g['results'][str(tsl)]
  assert len(want) == len(docs)
  assert pl['doc_chunk_off'].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
  flat = [r for w in want for r in w]
  assert len(chunks) == len(flat) == len(pl['chunk_num_tokens'])
  for c, (text, ntok, tl) in enumerate(flat):
    assert chunks[c].decode('utf-8') == text, c
    assert int(pl['chunk_num_tokens'][c]) == ntok and tl == tsl - 3, c
  assert pl['chunk_off'][-1] == sum(len(t.encode('utf-8')) for t, _, _ in flat)


def test_model_zero_word_sentences_and_small_targets():
  # 0-word sentences add their text to a chunk; a remainder of them is dropped; a document of them yields nothing
  docs = [[b'', b'  ', b'a b', b' ', b''], [b' ', b''], [], [b'\t', b'x', b'']]
  data, so, dso = bm.table(docs)
  pl, chunks = bm.aggregate(data, so, dso, 2)
  assert chunks == [b'     a b', b' \t x ']
  assert pl['chunk_sent0'].tolist() == [0, 7] and pl['chunk_nsent'].tolist() == [3, 3]
  assert pl['chunk_num_tokens'].tolist() == [2, 1] and pl['doc_chunk_off'].tolist() == [0, 1, 1, 1, 2]
  assert pl['chunk_off'].tolist() == [0, 8, 13]
  for T in (0, -1):  # the reference's `>=`: every sentence closes a chunk, 0-word ones included
    pl, chunks = bm.aggregate(data, so, dso, T)
    assert pl['chunk_nsent'].tolist() == [1] * 10
    assert pl['chunk_num_tokens'].tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 1, 0]


REFERENCE_FLAGS = ['--schedule', '--local-n-workers', '--local-threads-per-worker', '--wikipedia', '--books',
                   '--common-crawl', '--open-webtext', '--sink', '--output-format', '--wikipedia-lang',
                   '--target-seq-length', '--short-seq-prob', '--block-size', '--num-blocks']


def test_cli_flags_are_the_references():
  from lddl_amd import preprocess
  p = preprocess.attach_bart_args()
  flags = sorted(o for a in p._actions for o in a.option_strings if o not in ('-h', '--help'))
  # the reference's flags, and the splitter choice the other two sub-commands have
  assert flags == sorted(REFERENCE_FLAGS + ['--sentence-splitter'])
  a = p.parse_args(['--sink', 's'])
  assert (a.target_seq_length, a.short_seq_prob, a.output_format, a.wikipedia_lang, a.schedule) == \
      (128, 0.1, 'parquet', 'en', 'mpi')
  assert a.block_size is None and a.num_blocks is None and a.open_webtext is None
  assert p.parse_args(['--sink', 's', '--block-size', '64M']).block_size == 64 << 20
  with pytest.raises(SystemExit):
    p.parse_args(['--sink', 's', '--output-format', 'csv'])
  with pytest.raises(SystemExit):
    p.parse_args([])  # --sink is required


def test_cli_block_size_and_num_blocks_together(tmp_path):
  from lddl_amd import preprocess
  (tmp_path / 'books').mkdir()
  (tmp_path / 'books' / 'a.txt').write_text('one line. of text.\n')
  args = preprocess.attach_bart_args().parse_args(['--books', str(tmp_path / 'books'), '--sink', str(tmp_path / 'o'),
                                                   '--block-size', '1M', '--num-blocks', '3'])
  with pytest.raises(ValueError):
    preprocess.plan_bart_input(args)
  with pytest.raises(ValueError):
    preprocess.bart_main(args)


def test_cli_plan_keeps_input_order_and_whole_lines(tmp_path):
  from lddl_amd import preprocess
  src = tmp_path / 'wiki' / 'en'
  src.mkdir(parents=True)
  (src / 'a.txt').write_text('id1 First doc. It has two.\n\nid2 Second doc here.\n')
  (src / 'b.txt').write_text('id3 Third. Doc!\n')
  args = preprocess.attach_bart_args().parse_args(['--wikipedia', str(tmp_path / 'wiki'), '--sink', 'x',
                                                   '--num-blocks', '3'])
  index, order, pro = preprocess.plan_bart_input(args)
  assert order.tolist() == [0, 1, 2] and pro[0] == 0 and pro[-1] == 3
  corpus, _ = preprocess.split_chunk(index, order, False, preprocess._rule_split, True)
  sents = [corpus.sentence(i) for i in range(corpus.n_sent)]
  assert sents == ['id1 First doc.', 'It has two.', 'id2 Second doc here.', 'id3 Third.', 'Doc!']
  assert corpus.doc_sent_off.tolist() == [0, 2, 3, 5]
  index.close()


def test_bart_file_plan_takes_partitions_as_files():
  """the BART writers' plan: a partition's chunks are one file (writer.FilePlan, one bin)"""
  from lddl_amd import bart
  from types import SimpleNamespace
  res = SimpleNamespace(part_chunk_off=np.array([0, 4, 4, 9, 10], np.int64))
  plan = bart._plan(res, None, 5)
  assert (plan.nfiles, plan.n_rows, plan.nbins) == (4, 10, 1)
  assert list(plan.batches(5)) == [(0, 2, 0, 4), (2, 3, 4, 9), (3, 4, 9, 10)]
  assert plan.files(0, 2, 'o', 'parquet') == [(os.path.join('o', 'part.5.parquet'), 0, 4),
                                              (os.path.join('o', 'part.6.parquet'), 4, 4)]
  assert plan.files(2, 4, 'o', 'txt') == [(os.path.join('o', '7.txt'), 0, 5), (os.path.join('o', '8.txt'), 5, 6)]
  plan = bart._plan(res, 3, 0)
  assert (plan.nfiles, plan.n_rows) == (3, 9) and list(plan.batches(1 << 16)) == [(0, 3, 0, 9)]
  assert bart._plan(res, 9, 0).nfiles == 4


def test_write_bart_shards_executor_needs_pending(tmp_path):
  import concurrent.futures
  from lddl_amd import bart
  out = tmp_path / 'o'
  with concurrent.futures.ThreadPoolExecutor(1) as ex:
    with pytest.raises(ValueError):
      bart.write_bart_shards(None, str(out), executor=ex)
  assert not out.exists()
