"""The layers above the sentence-order packer on a corpus of about 200 rows
(tests/sop_pack_model.py corpus_rows, target_seq_length 32): the rows are BERT
rows, so the parquet writer, load_shards, RowBatches and every BertCollate
route take them with no argument of their own -- checked against the model's
rows, never against a kernel's output -- and the ``--sop`` command line end to
end against the Packer route."""
import os
import subprocess
import sys

import numpy as np
import pyarrow.parquet as pq
import pytest
import torch

import sop_pack_model as sm
from conftest import ROOT
from test_collate_rows_gpu import assert_model, model
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


def model_rows(packer, parts):
  """the model's partitions as PackResult.rows() would give them"""
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  return [(p, r.A, r.B, 2 | int(r.swap), r.bin, [cls] + r.A + [sep] + r.B + [sep])
          for p, part in enumerate(parts) for r in part]


@pytest.fixture(scope='module')
def world(packer):
  """(pack result with spans, the model's partitions, the model's rows)"""
  from lddl_amd.pipeline import PackHandle
  corpus = sm.corpus_rows()
  sh, ids, ntok = shards_from_docs(corpus[0], part_doc_off=corpus[1])
  res = packer.pack(sh, ids, ntok, target_seq_length=SEQ, short_seq_prob=SSP, duplicate_factor=DUP, seed=SEED,
                    bin_size=BIN, spans=True, sop=True, into=PackHandle(packer.tok))
  torch.cuda.synchronize()
  res.shards = sh
  parts = sm.pack(corpus, SEQ, SSP, DUP, SEED, BIN)
  rows = model_rows(packer, parts)
  assert res.kind == 'bert' and res.n_pairs == len(rows) and 150 <= len(rows) <= 300
  assert any(r[3] & 1 for r in rows) and not all(r[3] & 1 for r in rows)
  return res, parts, rows


@pytest.fixture(scope='module')
def shard_dir(packer, world, tmp_path_factory):
  from lddl_amd import writer
  out = str(tmp_path_factory.mktemp('sop_shards'))
  writer.write_shards(packer, world[0], out, bin_size=BIN)
  return out


def collate(packer, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=packer.tok, sequence_length_alignment=8, base_seed=BASE_SEED, **kw)


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
  res, parts, _ = world
  if not binned:  # an unbinned pack of the same corpus: other rows in another order
    corpus = sm.corpus_rows()
    res = packer.pack(*shards_from_docs(corpus[0], part_doc_off=corpus[1]), target_seq_length=SEQ, short_seq_prob=SSP,
                      duplicate_factor=DUP, seed=SEED, spans=True, sop=True)
    parts = sm.pack(corpus, SEQ, SSP, DUP, SEED, None)
  out = str(tmp_path / 'out')
  files = writer.write_shards(packer, res, out, bin_size=BIN if binned else None)
  nb = SEQ // BIN
  names = ['part.%d.parquet_%d' % (p, b) for p in range(len(parts)) for b in range(nb)] if binned else [
      'part.%d.parquet' % p for p in range(len(parts))]
  assert sorted(os.listdir(out)) == sorted(names) and [os.path.basename(f) for f in files] == names
  sch = writer.schema(binned=binned)  # the NSP pairs' schema
  assert sch.names == ['A', 'B', 'is_random_next', 'num_tokens'] + (['bin_id'] if binned else [])
  join = lambda toks: ' '.join(vocab[t] for t in toks)  # noqa: E731
  for p, part in enumerate(parts):
    for b in range(nb if binned else 1):
      t = pq.read_table(os.path.join(out, names[p * nb + b] if binned else names[p]))
      assert t.schema.equals(sch)
      want = [r for r in part if r.bin == b] if binned else part
      d = t.to_pydict()
      assert d['A'] == [join(r.A) for r in want]
      assert d['B'] == [join(r.B) for r in want]
      assert d['is_random_next'] == [r.swap for r in want]
      assert d['num_tokens'] == [len(r.A) + len(r.B) + 3 for r in want]
      if binned:
        assert d['bin_id'] == [b] * len(want)


# ---- loader -----------------------------------------------------------------------
@pytest.mark.parametrize('k', range(4))
def test_collate_rows_mode0_vs_model(packer, world, k):
  """[CLS] A [SEP] B [SEP] from the model, next_sentence_labels = swap, token_type_ids 1 on B and its [SEP]"""
  res, _, rows = world
  idx = batches(rows)[k]
  out = collate(packer).collate_rows(res, idx, mode=0)
  assert_model(out, model(rows, idx, 8, 0))
  nsl = out['next_sentence_labels'].cpu().tolist()
  assert nsl == [rows[g][3] & 1 for g in idx]
  tt = out['token_type_ids'].cpu().numpy()
  for r, g in enumerate(idx):
    a, b = len(rows[g][1]), len(rows[g][2])
    assert not tt[r, :a + 2].any() and tt[r, a + 2:a + 2 + b].all()


def assert_same(a, b):
  assert set(a) == set(b)
  for key in a:
    assert a[key] == b[key] if not torch.is_tensor(a[key]) else (a[key].shape == b[key].shape and
                                                                 torch.equal(a[key], b[key])), key


def test_load_shards_and_batches(packer, world, shard_dir):
  from lddl_amd.loader import RowBatches, load_shards
  res, parts, rows = world
  col = collate(packer)
  got = load_shards(col, shard_dir)
  assert got.kind == 'bert' and got.spans and got.n_pairs == len(rows) and got.nbins == SEQ // BIN
  # (a table loaded from shards knows is_random_next, not the packer's bit 1)
  assert [(p, a, b, fl & 1, bn, tok) for p, a, b, fl, bn, tok in got.rows()] == [
      (p, a, b, fl & 1, bn, tok) for p, a, b, fl, bn, tok in rows]
  assert got.bin_count.cpu().numpy().tolist() == sm.bin_counts(parts, SEQ, BIN)
  for idx in batches(rows):
    for mode in (0, 2):
      col.counter = 4
      a = col.collate_rows(res, idx, mode=mode)
      col.counter = 4
      b = col.collate_rows(got, idx, mode=mode)
      assert_same(a, b)
  # an epoch of binned batches over the table
  seen = []
  for idx in RowBatches(got, 32, seed=1):
    batch = col.collate_rows(got, idx)
    assert batch['input_ids'].shape[1] <= SEQ
    seen += idx.cpu().tolist()
  assert sorted(seen) == list(range(len(rows)))


@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('mode', [0, 2])
def test_unpadded_and_fixed_agree_with_padded(packer, world, k, mode):
  res, _, rows = world
  idx = batches(rows)[k]
  col = collate(packer)
  col.counter = 6
  pad = col.collate_rows(res, idx, mode=mode)
  col.counter = 6
  un = col.collate_rows_unpadded(res, idx, mode=mode)
  total = sum(len(rows[g][5]) for g in idx)
  T, N, S = total + 45, len(idx) + 4, SEQ
  col.counter = 6
  fx = col.collate_rows_fixed(res, idx, mode=mode, max_tokens=T, max_seqs=N, max_seqlen=S)
  keep = pad['attention_mask'] == 1
  lab = 'special_tokens_mask' if mode == 0 else 'labels'
  lens = [len(rows[g][5]) for g in idx]
  assert un['cu_seqlens'].cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
  assert un['max_seqlen'] == max(lens)
  for key in ('input_ids', 'token_type_ids', lab):
    assert torch.equal(un[key], pad[key][keep]), key
    assert torch.equal(fx[key][:total], un[key]), key
  assert torch.equal(un['next_sentence_labels'], pad['next_sentence_labels'])
  n = len(idx)
  assert torch.equal(fx['next_sentence_labels'][:n], pad['next_sentence_labels'])
  assert torch.equal(fx['cu_seqlens'][:n + 1], un['cu_seqlens'])
  assert (fx['num_tokens'], fx['num_rows']) == (total, n)
  if mode == 0:  # the real tokens are the model's rows back to back
    assert un['input_ids'].cpu().tolist() == [t for g in idx for t in rows[g][5]]


def test_span_mask_labels_only_non_special_positions(packer, world):
  res, _, rows = world
  idx = list(range(0, len(rows), 3))
  col = collate(packer, span_mask=True, mlm_probability=0.3)
  try:
    out = col.collate_rows(res, idx)  # (mode 2)
    spec = collate(packer, span_mask=True).collate_rows(res, idx, mode=0)['special_tokens_mask']
  finally:
    collate(packer)  # the ctx's switch off again
  labelled = out['labels'] != col.ignore_index
  assert bool(labelled.any()) and not bool((labelled & (spec == 1)).any())
  # a labelled position's label is the model's token there; the others show it unchanged
  want = torch.from_numpy(model(rows, idx, 8, 0)['input_ids']).to(out['input_ids'].device)
  assert torch.equal(out['labels'][labelled], want[labelled])
  assert torch.equal(out['input_ids'][~labelled], want[~labelled])
  assert out['next_sentence_labels'].cpu().tolist() == [rows[g][3] & 1 for g in idx]


# ---- command line -----------------------------------------------------------------
def _read(path):
  return pq.read_table(path)


def test_cli_sop_end_to_end(packer, tmp_path):
  """`preprocess --sop` writes the files of Packer.run(sop=True) + write_shards over the same planned, split
  corpus; --sop with --masking or --no-nsp is an argument error"""
  from lddl_amd import pipeline, preprocess, writer
  src = tmp_path / 'wiki' / 'en'
  src.mkdir(parents=True)
  words = ['alpha', 'beta', 'gamma', 'delta', 'river', 'stone', 'house', 'green', 'walks', 'reads']
  for k in range(2):  # (a block does not span files: two partitions)
    with open(str(src / ('wiki_%d.txt' % k)), 'w', encoding='utf-8') as f:
      for d in range(8 * k, 8 * k + 8):
        sents = [' '.join(words[(d + s + j) % 10] for j in range(3 + (d + s) % 6)).capitalize() + '.'
                 for s in range(1 + d % 7)]
        f.write('doc%d %s\n' % (d, ' '.join(sents)))
  sink = tmp_path / 'sink'
  env = dict(os.environ, LDDL_ENCODE_PROCS='0', LDDL_CPU_SHARE='2',
             PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
  argv = ['--wikipedia', str(tmp_path / 'wiki'), '--target-seq-length', '32', '--bin-size', '8',
          '--num-blocks', '2', '--sentence-splitter', 'rules', '--seed', '5', '--split-workers', '0',
          '--sample-ratio', '1.0', '--duplicate-factor', '2']
  r = subprocess.run([sys.executable, '-m', 'lddl_amd.preprocess', '--sop', '--sink', str(sink)] + argv, cwd=ROOT,
                     env=env, capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-2000:]
  # the Packer route over the same plan
  args = preprocess.parse_args(['--sop', '--sink', str(tmp_path / 'unused')] + argv)
  idx, order, pdo = preprocess.plan_input(args)
  assert len(pdo) - 1 == 2
  corpus, _ = preprocess.split_records(idx.texts(order), splitter=preprocess._rule_split)
  sh = pipeline.upload(corpus, pdo, torch.device('cuda', 0))
  res = packer.run(sh, target_seq_length=32, short_seq_prob=args.short_seq_prob, duplicate_factor=2, seed=5,
                   bin_size=8, spans=True, sop=True)
  torch.cuda.synchronize()
  assert res.n_pairs >= 10
  flags = res.flags[:res.n_pairs].cpu().numpy()
  assert (flags & 1).any() and not (flags & 1).all()
  mine = tmp_path / 'mine'
  files = writer.write_shards(packer, res, str(mine), bin_size=8)
  names = sorted(os.path.basename(f) for f in files)
  assert names == sorted('part.%d.parquet_%d' % (p, b) for p in range(2) for b in range(4))
  assert sorted(f for f in os.listdir(str(sink)) if '.parquet' in f) == names
  for f in names:
    assert _read(str(sink / f)).equals(_read(str(mine / f))), f
  for extra in (['--masking'], ['--no-nsp']):
    bad = subprocess.run([sys.executable, '-m', 'lddl_amd.preprocess', '--sop', '--sink', str(tmp_path / 'never')] +
                         extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and '--sop' in bad.stderr and not os.path.exists(str(tmp_path / 'never'))
