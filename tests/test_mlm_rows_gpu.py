"""The layers above the MLM-only packer on a corpus of about 200 rows
(tests/mlm_pack_model.py corpus_rows, target_seq_length 32): the parquet
writer (nsp=False), MlmCollate over the pack result and over the shards
(padded and padding-free, modes 0 and 2, whole-word masking, compact MLM
targets) against the host models, BertCollate's refusals, and the
``--no-nsp`` command line end to end with the load balancer behind it.
Every expectation comes from the model's rows, never from a kernel's output."""
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import code_collate_model as ccm
import mlm_pack_model as mm
import mlm_targets_model as tm
import wwm_model as wm
from conftest import ROOT
from test_pack_gpu import shards_from_docs

pytestmark = pytest.mark.gpu

SEQ, SSP, DUP, SEED, BIN = 32, 0.1, 2, 21, 8
BASE_SEED = 777


@pytest.fixture(scope='module')
def packer(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_BERT
  return Packer(VOCAB_BERT, 0)


@pytest.fixture(scope='module')
def vocab(packer):
  with open(packer.tok.vocab_file, encoding='utf-8') as f:
    return [l.rstrip('\n').rstrip('\r') for l in f]


@pytest.fixture(scope='module')
def world(packer):
  """(pack result with spans, the model's partitions, the model's rows as PackResult.rows() would give them)"""
  from lddl_amd.pipeline import PackHandle
  corpus = mm.corpus_rows()
  sh, ids, ntok = shards_from_docs(corpus[0], part_doc_off=corpus[1])
  res = packer.pack(sh, ids, ntok, target_seq_length=SEQ, short_seq_prob=SSP, duplicate_factor=DUP, seed=SEED,
                    bin_size=BIN, spans=True, nsp=False, into=PackHandle(packer.tok))
  torch.cuda.synchronize()
  res.shards = sh
  parts = mm.pack(corpus, SEQ, SSP, DUP, SEED, BIN)
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  rows = [(p, [], r.toks, 0, r.bin, [cls] + r.toks + [sep]) for p, part in enumerate(parts) for r in part]
  assert res.n_pairs == len(rows) and 150 <= len(rows) <= 300
  return res, parts, rows


@pytest.fixture(scope='module')
def shard_dir(packer, world, tmp_path_factory):
  from lddl_amd import writer
  out = str(tmp_path_factory.mktemp('mlm_shards'))
  writer.write_shards(packer, world[0], out, bin_size=BIN, nsp=False)
  return out


def collate(packer, **kw):
  """an MlmCollate over the packer's ctx (constructing one sets the ctx's whole-word switch, on or off)"""
  from lddl_amd.loader import MlmCollate
  return MlmCollate(tokenizer=packer.tok, sequence_length_alignment=8, base_seed=BASE_SEED, **kw)


def draw_kw(col, counter):
  return dict(seed=col.seed, counter=counter, p=col.mlm_probability, mask_id=col.tok.mask_id,
              n_random=col.tok.vocab_size, ignore=col.ignore_index)


def assert_batch(out, exp):
  assert set(out) == set(exp), (sorted(out), sorted(exp))  # (no next_sentence_labels among them)
  for k, v in exp.items():
    if k == 'max_seqlen':
      assert out[k] == v and isinstance(out[k], int)
      continue
    got = out[k].cpu().numpy()
    assert got.shape == v.shape and got.dtype == v.dtype, (k, got.shape, got.dtype, v.shape, v.dtype)
    assert np.array_equal(got, v), k


def batches(rows):
  """row picks: one bin's run, a mix across bins and partitions with a repeat, the shortest and longest rows"""
  n = len(rows)
  lens = [len(r[5]) for r in rows]
  return [list(range(0, 9)), [n - 1, 0, n // 2, 0, 7, n // 3], [int(np.argmin(lens)), int(np.argmax(lens))],
          list(range(n - 70, n))]


# ---- writer ---------------------------------------------------------------------
@pytest.mark.parametrize('binned', [True, False])
def test_write_shards(packer, world, vocab, tmp_path, binned):
  from lddl_amd import writer
  res, parts, rows = world
  if not binned:  # an unbinned pack of the same corpus: other rows in another order
    corpus = mm.corpus_rows()
    res = packer.pack(*shards_from_docs(corpus[0], part_doc_off=corpus[1]), target_seq_length=SEQ, short_seq_prob=SSP,
                      duplicate_factor=DUP, seed=SEED, spans=True, nsp=False)
    parts = mm.pack(corpus, SEQ, SSP, DUP, SEED, None)
  out = str(tmp_path / 'out')
  files = writer.write_shards(packer, res, out, bin_size=BIN if binned else None, nsp=False)
  nb = SEQ // BIN
  names = ['part.%d.parquet_%d' % (p, b) for p in range(len(parts)) for b in range(nb)] if binned else [
      'part.%d.parquet' % p for p in range(len(parts))]
  assert sorted(os.listdir(out)) == sorted(names) and [os.path.basename(f) for f in files] == names
  tok_id = {t: i for i, t in enumerate(vocab)}
  sch = writer.schema(nsp=False, binned=binned)
  assert sch.names == ['A', 'num_tokens'] + (['bin_id'] if binned else [])
  for p, part in enumerate(parts):
    for b in range(nb if binned else 1):
      t = pq.read_table(os.path.join(out, names[p * nb + b] if binned else names[p]))
      assert t.schema.equals(sch)
      want = [r for r in part if r.bin == b] if binned else part
      d = t.to_pydict()
      assert [[tok_id[w] for w in a.split(' ')] for a in d['A']] == [r.toks for r in want]
      assert d['num_tokens'] == [len(r.toks) + 2 for r in want]
      if binned:
        assert d['bin_id'] == [b] * len(want)
  with pytest.raises(ValueError):  # an MLM-only result is not written as NSP pairs, nor a txt sink
    writer.write_shards(packer, res, str(tmp_path / 'never'), bin_size=BIN if binned else None)
  with pytest.raises(ValueError):
    writer.write_txt(packer, res, str(tmp_path / 'never'), nsp=False)
  assert not os.path.exists(str(tmp_path / 'never'))


def test_write_shards_from_materialised_rows(packer, world, tmp_path):
  """the same files from a result with materialised rows (segment 1 behind [CLS], no [SEP] in front of it)"""
  from lddl_amd import writer
  corpus = mm.corpus_rows()
  res = packer.pack(*shards_from_docs(corpus[0], part_doc_off=corpus[1]), target_seq_length=SEQ, short_seq_prob=SSP,
                    duplicate_factor=DUP, seed=SEED, bin_size=BIN, nsp=False)
  a, b = str(tmp_path / 'mat'), str(tmp_path / 'spans')
  writer.write_shards(packer, res, a, bin_size=BIN, nsp=False)
  writer.write_shards(packer, world[0], b, bin_size=BIN, nsp=False)
  for f in sorted(os.listdir(b)):
    assert pq.read_table(os.path.join(a, f)).equals(pq.read_table(os.path.join(b, f))), f


# ---- loader, pack route -----------------------------------------------------------
@pytest.mark.parametrize('k', range(4))
def test_collate_rows_vs_models(packer, world, k):
  res, _, rows = world
  idx = batches(rows)[k]
  col = collate(packer)
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  assert_batch(col.collate_rows(res, idx, mode=0), ccm.padded(rows, idx, 8, 0, cls, sep))
  assert_batch(col.collate_rows_unpadded(res, idx, mode=0), ccm.unpadded(rows, idx, 0, cls, sep))
  assert col.counter == 0
  for counter in (0, 5):
    col.counter = counter
    out = col.collate_rows(res, idx)  # (mode 2 by default)
    assert_batch(out, ccm.padded(rows, idx, 8, 2, cls, sep, **draw_kw(col, counter)))
    assert not out['token_type_ids'].any() and col.counter == counter + 1
    col.counter = counter
    assert_batch(col.collate_rows_unpadded(res, idx), ccm.unpadded(rows, idx, 2, cls, sep, **draw_kw(col, counter)))
  with pytest.raises(ValueError):
    col.collate_rows(res, idx, mode=1)


def wwm_expected(packer, vocab, rows, idx, col, counter):
  """padded planes masked by whole words (tests/wwm_model.py) -> (padded dict, unpadded dict)"""
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  base = ccm.padded(rows, idx, 8, 0, cls, sep)
  kw = draw_kw(col, counter)
  m = wm.mask(base['input_ids'], base['special_tokens_mask'], wm.cont_table(vocab), kw['seed'], counter, kw['p'],
              kw['mask_id'], kw['n_random'], kw['ignore'])
  pad = {'input_ids': m[0], 'labels': m[1], 'token_type_ids': base['token_type_ids'],
         'attention_mask': base['attention_mask']}
  keep = base['attention_mask'] == 1
  un = ccm.unpadded(rows, idx, 0, cls, sep)
  del un['special_tokens_mask']
  un['input_ids'], un['labels'] = m[0][keep], m[1][keep]
  return pad, un


@pytest.mark.parametrize('k', range(5))
def test_whole_word_mask(packer, world, vocab, k):
  res, _, rows = world
  if k < 4:
    idx = batches(rows)[k]
  else:  # the rows that hold '##' pieces (the corpus' ids are consecutive vocabulary entries): words of several tokens
    table = wm.cont_table(vocab)
    idx = [g for g, r in enumerate(rows) if any(table[t] for t in r[2])][:16]
    assert len(idx) >= 4
  col = collate(packer, whole_word_mask=True, mlm_probability=0.3)
  try:
    pad, un = wwm_expected(packer, vocab, rows, idx, col, 3)
    col.counter = 3
    assert_batch(col.collate_rows(res, idx), pad)
    col.counter = 3
    assert_batch(col.collate_rows_unpadded(res, idx), un)
  finally:
    collate(packer)  # the ctx's switch off again


@pytest.mark.parametrize('k', range(4))
def test_compact_mlm(packer, world, k):
  res, _, rows = world
  idx = batches(rows)[k]
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  col = collate(packer, compact_mlm=True, mlm_probability=0.25)
  col.counter = 2
  exp = ccm.padded(rows, idx, 8, 2, cls, sep, **draw_kw(col, 2))
  t = tm.targets(exp['labels'], col.ignore_index)
  exp.update(masked_lm_positions=t.positions, masked_lm_labels=t.target_labels, masked_lm_offsets=t.offsets)
  assert_batch(col.collate_rows(res, idx), exp)
  col.counter = 2
  exp = ccm.unpadded(rows, idx, 2, cls, sep, **draw_kw(col, 2))
  t = tm.targets(exp['labels'], col.ignore_index, cu_seqlens=exp['cu_seqlens'])
  exp.update(masked_lm_positions=t.positions, masked_lm_labels=t.target_labels, masked_lm_offsets=t.offsets)
  assert_batch(col.collate_rows_unpadded(res, idx), exp)
  assert 'special_tokens_mask' in col.collate_rows(res, idx, mode=0)  # (no labels, no targets)


# ---- loader, shard route ----------------------------------------------------------
def test_load_shards_and_batches(packer, world, shard_dir):
  from lddl_amd.loader import RowBatches, load_shards
  res, parts, rows = world
  col = collate(packer)
  got = load_shards(col, shard_dir)
  assert got.kind == 'mlm' and got.spans and got.n_pairs == len(rows) and got.nbins == SEQ // BIN
  assert got.rows() == rows
  assert got.bin_count.cpu().numpy().tolist() == mm.bin_counts(parts, SEQ, BIN)
  assert got.bins[:got.n_pairs].cpu().numpy().tolist() == [r[4] for r in rows]
  assert got.part[:got.n_pairs].cpu().numpy().tolist() == [r[0] for r in rows]
  for idx in batches(rows):
    for fn in ('collate_rows', 'collate_rows_unpadded'):
      for mode in (0, 2):
        col.counter = 4
        a = getattr(col, fn)(res, idx, mode=mode)
        col.counter = 4
        b = getattr(col, fn)(got, idx, mode=mode)
        assert set(a) == set(b) and 'next_sentence_labels' not in a
        for key in a:
          assert a[key] == b[key] if key == 'max_seqlen' else torch.equal(a[key], b[key]), (fn, mode, key)
  # an epoch of binned batches over the table
  seen = []
  for idx in RowBatches(got, 32, seed=1):
    batch = col.collate_rows(got, idx)
    assert batch['input_ids'].shape[1] <= SEQ
    seen += idx.cpu().tolist()
  assert sorted(seen) == list(range(len(rows)))


def test_other_kinds_are_refused(packer, world, shard_dir, tmp_path):
  from lddl_amd.loader import BertCollate, CodeCollate, load_shards
  res = world[0]
  bert = BertCollate(tokenizer=packer.tok)
  for fn in (bert.collate_rows, bert.collate_rows_unpadded):
    with pytest.raises(ValueError, match='MlmCollate'):
      fn(res, [0, 1])
  with pytest.raises(ValueError, match='MlmCollate'):
    load_shards(bert, shard_dir)
  with pytest.raises(ValueError, match='MlmCollate'):
    bert.load_rows(pq.read_table(os.path.join(shard_dir, 'part.0.parquet_1')))
  # MlmCollate on shards of the other kinds
  col = collate(packer)
  d = tmp_path / 'bert'
  d.mkdir()
  pq.write_table(pa.table({'A': ['the cat'], 'B': ['sat'], 'is_random_next': [False],
                           'num_tokens': pa.array([6], pa.uint16())}), str(d / 'part.0.parquet'))
  with pytest.raises(ValueError, match='BertCollate'):
    load_shards(col, str(d))
  c = tmp_path / 'code'
  c.mkdir()
  pq.write_table(pa.table({'id': ['x'], 'doc': ['the'], 'code': ['cat'], 'num_tokens': pa.array([5], pa.uint16())}),
                 str(c / 'part.0.parquet'))
  with pytest.raises(ValueError, match='CodeCollate'):
    load_shards(col, str(c))
  with pytest.raises(ValueError):
    load_shards(CodeCollate(tokenizer=packer.tok), shard_dir)
  # a row whose num_tokens is not len(A.split()) + 2: refused by the C call, or (+ 3, a CodeBERT row with an
  # empty docstring and its [SEP]) by load_rows
  with pytest.raises(RuntimeError):
    col.load_rows(pa.table({'A': ['the cat'], 'num_tokens': pa.array([7], pa.uint16())}))
  with pytest.raises(ValueError, match='num_tokens'):
    col.load_rows(pa.table({'A': ['the cat'], 'num_tokens': pa.array([5], pa.uint16())}))


# ---- command line -----------------------------------------------------------------
def test_cli_no_nsp_end_to_end(packer, vocab, tmp_path):
  from lddl_amd import balance, writer
  from lddl_amd.loader import load_shards
  src = tmp_path / 'wiki' / 'en'
  src.mkdir(parents=True)
  words = ['alpha', 'beta', 'gamma', 'delta', 'river', 'stone', 'house', 'green', 'walks', 'reads']
  for k in range(3):  # (a block does not span files: at least three partitions)
    with open(str(src / ('wiki_%d.txt' % k)), 'w', encoding='utf-8') as f:
      for d in range(8 * k, 8 * k + 8):
        sents = [' '.join(words[(d + s + j) % 10] for j in range(3 + (d + s) % 6)).capitalize() + '.'
                 for s in range(2 + d % 7)]
        f.write('doc%d %s\n' % (d, ' '.join(sents)))
  sink = tmp_path / 'sink'
  env = dict(os.environ, LDDL_ENCODE_PROCS='0', LDDL_CPU_SHARE='2',
             PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
  argv = ['--wikipedia', str(tmp_path / 'wiki'), '--sink', str(sink), '--target-seq-length', '32', '--bin-size', '8',
          '--num-blocks', '3', '--sentence-splitter', 'rules', '--seed', '5', '--split-workers', '0',
          '--sample-ratio', '1.0', '--duplicate-factor', '2']
  r = subprocess.run([sys.executable, '-m', 'lddl_amd.preprocess', '--no-nsp'] + argv, cwd=ROOT, env=env,
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-2000:]
  names = sorted(f for f in os.listdir(str(sink)) if '.parquet' in f)
  n_part = 1 + max(int(f.split('.')[1]) for f in names)  # (the partitions the front end cut the source into)
  assert names == sorted('part.%d.parquet_%d' % (p, b) for p in range(n_part) for b in range(4))  # every bin's file
  assert n_part >= 3
  sch = writer.schema(nsp=False, binned=True)
  rows = []
  for f in names:
    t = pq.read_table(str(sink / f))
    assert t.schema.equals(sch), f
    rows += list(zip(t.column('A').to_pylist(), t.column('num_tokens').to_pylist(), t.column('bin_id').to_pylist()))
  assert len(rows) >= 24 * 2  # at least a row per document visit
  known = set(vocab)
  for a, n, b in rows:
    assert n == len(a.split(' ')) + 2 <= 32 and b == (n - 1) // 8 and all(w in known for w in a.split(' '))
  got = load_shards(collate(packer), str(sink))
  assert got.kind == 'mlm' and got.n_pairs == len(rows)
  batch = collate(packer).collate_rows(got, list(range(8)))
  assert 'next_sentence_labels' not in batch and not batch['token_type_ids'].any()
  # --masking with --no-nsp is an argument error, before anything is read or written
  bad = subprocess.run([sys.executable, '-m', 'lddl_amd.preprocess', '--no-nsp', '--masking', '--sink',
                        str(tmp_path / 'never')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
  assert bad.returncode == 2 and '--no-nsp' in bad.stderr and not os.path.exists(str(tmp_path / 'never'))
  # the load balancer over the sink: same schema, same rows per bin
  outd = tmp_path / 'balanced'
  balance.main(balance.attach_args().parse_args(['--indir', str(sink), '--outdir', str(outd), '--num-shards', '2',
                                                 '--keep-orig']), rank=0, world=1)
  back = []
  for f in sorted(os.listdir(str(outd))):
    if '.parquet' in f:
      t = pq.read_table(str(outd / f))
      assert t.schema.equals(sch), f
      back += list(zip(t.column('A').to_pylist(), t.column('num_tokens').to_pylist(), t.column('bin_id').to_pylist()))
  assert sorted(back) == sorted(rows)
  assert load_shards(collate(packer), str(outd)).n_pairs == len(rows)
