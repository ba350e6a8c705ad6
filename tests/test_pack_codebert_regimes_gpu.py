"""The CodeBERT packer (pack_codebert_wave_kernel) in every regime of its
docstring scan, chunk loop, truncation rounds and error exits, against the
oracle and against the reference's own rows: the configurations of
tests/codebert_regimes.py (tests/test_codebert_regimes_host.py shows that each
one reaches its regimes; tests/test_pack_oracle.py pins the oracle on them)
packed on the GPU and compared by exact equality -- partition, docstring ids,
code ids, num_tokens, bin, the docstring flag, the whole token row and the
per-partition bin counts -- materialised and as spans; the two error exits as
exactly their exceptions, beside partitions that pack, with the handles'
state afterwards; several seeds; and the rows through the parquet writer, the
shard loader and a collate."""
import os

import numpy as np
import pytest
import torch

import codebert_regimes as cr
from oracle import pack_oracle as po
from test_pack_gpu import shards_from_docs
from test_pack_oracle import REGIMES

pytestmark = pytest.mark.gpu

EXC = {'AssertionError': AssertionError, 'IndexError': IndexError}


@pytest.fixture(scope='module')
def cpacker(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_CODEBERT
  return Packer(VOCAB_CODEBERT, 0)


def pack(pk, corpus, seq, ssp, seed, spans=False, into=None):
  docs, ndoc, pdo = corpus
  sh, ids, ntok = shards_from_docs(docs, ndoc, part_doc_off=pdo)
  res = pk.pack(sh, ids, ntok, target_seq_length=seq, short_seq_prob=ssp, duplicate_factor=cr.DUP, seed=seed,
                codebert=True, bin_size=cr.bin_size(seq), spans=spans, into=into)
  torch.cuda.synchronize()
  # lddl_row_docs reads the pack call's own input arrays (sent_off, doc_sent_off,
  # part_doc_off) through the handle: they live as long as the result does
  res.shards = sh
  return res


def doc_of_token(docs):
  """token id -> document (every token of a regime corpus has its own id)"""
  return {t: d for d, doc in enumerate(docs) for s in doc for t in s}


def check(pk, res, exp, counts, seq, spans):
  """res against rows (partition, docstring ids, code ids, num_tokens, has_docstring) in the binned order"""
  assert res.spans == spans and (res.tokens is None) == spans
  rows = res.rows()
  assert len(rows) == len(exp) == res.n_pairs
  bs = cr.bin_size(seq)
  for g, ((p, a, b, fl, bn, tok), e) in enumerate(zip(rows, exp)):
    assert (p, a, b, len(tok)) == e[:4], g
    assert fl == (2 if e[4] else 0), g  # [SEP] after the docstring, empty or not; never is_random_next
    assert bn == po.bin_of(e[3], bs, seq // bs), g
    assert tok == cr.row_tokens(e, pk.tok.cls_id, pk.tok.sep_id), g
  assert res.bin_count.cpu().numpy().tolist() == counts
  assert np.diff(res.tok_off[:res.n_pairs + 1].cpu().numpy()).tolist() == [e[3] for e in exp]
  assert res.n_tokens == sum(e[3] for e in exp)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,ssp', cr.CONFIGS)
def test_codebert_regimes_vs_oracle(cpacker, seq, ssp, spans):
  _, exp, counts = cr.oracle_rows(seq, ssp)
  res = pack(cpacker, cr.corpus(seq), seq, ssp, cr.PACK_SEEDS.get((seq, ssp), cr.PACK_SEED), spans)
  check(cpacker, res, exp, counts, seq, spans)


@pytest.mark.parametrize('k', range(len(REGIMES['cases'])))
def test_codebert_regimes_vs_reference_rows(cpacker, k):
  """the same packs against the rows the reference's create_pairs_from_document gave"""
  case = REGIMES['cases'][k]
  seq, ssp = case['seq'], case['ssp']
  corpus = cr.corpus(seq)
  assert [[len(s) for s in d] for d in corpus[0]] == case['corpus'] and corpus[1] == case['ndoc']
  exp, counts = cr.golden_rows(case)
  res = pack(cpacker, corpus, seq, ssp, case['seed'], k % 2 == 1)
  check(cpacker, res, exp, counts, seq, k % 2 == 1)


@pytest.mark.parametrize('seq,ssp,exc', cr.ERROR_CONFIGS)
def test_error_partition_beside_partitions_that_pack(cpacker, seq, ssp, exc):
  """The failing document sits in partition 1 of 3.  The pack raises exactly
  the reference's exception; the handle then reports no result; a handle
  packed before the failure still serves its rows; and the same packer and
  handle pack the main corpus again, equal to the oracle."""
  from lddl_amd import writer
  from lddl_amd.pipeline import PackHandle
  pk = cpacker
  main = cr.corpus(128)
  _, exp, counts = cr.oracle_rows(128, 0.0)
  where = doc_of_token(main[0])
  exp_docs = [where[e[2][0]] for e in exp]
  other = PackHandle(pk.tok)
  before = pack(pk, main, 128, 0.0, cr.PACK_SEED, into=other)
  assert other.rows() == len(exp)
  with pytest.raises(EXC[exc]) as ei:
    pack(pk, cr.error_corpus(seq, exc), seq, ssp, cr.PACK_SEED)
  assert type(ei.value) is EXC[exc]
  assert pk.result.rows() == -1
  third = PackHandle(pk.tok)  # and into a handle that held a result
  pack(pk, main, 128, 0.0, cr.PACK_SEED, into=third)
  assert third.rows() == len(exp)
  with pytest.raises(EXC[exc]) as ei:
    pack(pk, cr.error_corpus(seq, exc), seq, ssp, cr.PACK_SEED, spans=True, into=third)
  assert type(ei.value) is EXC[exc] and third.rows() == -1
  third.close()
  # the earlier handle: its count, its rows, and a post-pack call that reads the handle itself
  assert other.rows() == len(exp)
  check(pk, before, exp, counts, 128, False)
  assert writer.row_docs(pk, before).tolist() == exp_docs
  after = pack(pk, main, 128, 0.0, cr.PACK_SEED, spans=True)
  assert pk.result.rows() == len(exp)
  check(pk, after, exp, counts, 128, True)
  assert writer.row_docs(pk, after).tolist() == exp_docs
  other.close()


@pytest.mark.parametrize('seed', [0, 1, 2**32 - 2, 2**40 + 3])
def test_codebert_regime_seeds_vs_oracle(cpacker, seed):
  """random.seed(seed + p): 0, and 2**32 - 2 + p crossing into two key words"""
  _, exp, counts = cr.oracle_rows(128, 0.1, seed)
  res = pack(cpacker, cr.corpus(128), 128, 0.1, seed)
  check(cpacker, res, exp, counts, 128, False)


def layout(rows, idx, S, cls_id, sep_id):
  """input_ids, token_type_ids, attention_mask, special_tokens_mask of rows
  [CLS] doc [SEP] code [SEP], padded to S: a plain restatement (bert.py:129-152)"""
  out = np.zeros((4, len(idx), S), np.int64)
  for k, g in enumerate(idx):
    _, dt, ct, n, has = rows[g]
    assert has
    out[0, k, :n] = [cls_id] + dt + [sep_id] + ct + [sep_id]
    out[1, k, len(dt) + 2:n] = 1
    out[2, k, :n] = 1
    out[3, k, [0, len(dt) + 1, n - 1]] = 1
    out[3, k, n:] = 1  # padding counts as special (get_special_tokens_mask)
  return out


def test_codebert_rows_downstream(cpacker, tmp_path):
  """(128, 0.0) as spans through write_shards and a parquet read (id, doc,
  code, num_tokens, bin_id of every row); then the rows that have a docstring
  -- an empty one included: [CLS] [SEP] code [SEP] -- as A / B shards through
  load_shards and a collate_rows batch, and straight from the pack result.
  A CodeBERT shard itself has no loader and a row without a docstring no
  collate: both refusals are asserted, not worked around."""
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd import writer
  from lddl_amd.loader import BertCollate, load_shards
  pk = cpacker
  seq, ssp = 128, 0.0
  docs, ndoc, pdo = cr.corpus(seq)
  _, exp, counts = cr.oracle_rows(seq, ssp)
  res = pack(pk, (docs, ndoc, pdo), seq, ssp, cr.PACK_SEED, spans=True)
  check(pk, res, exp, counts, seq, True)
  where = doc_of_token(docs)
  out = str(tmp_path / 'codebert')
  writer.write_shards(pk, res, out, bin_size=cr.bin_size(seq), codebert=True, doc_ids=['py_%d' % d for d in range(len(docs))])
  names = [(p, b, os.path.join(out, 'part.%d.parquet_%d' % (p, b))) for p in range(cr.N_PART) for b in range(4)]
  tables = [pq.read_table(n) for _, _, n in names]
  assert [t.num_rows for t in tables] == [c for part in counts for c in part]
  d = pa.concat_tables(tables).to_pydict()
  with open(pk.tok.vocab_file, encoding='utf-8') as f:
    vocab = {l.rstrip('\n').rstrip('\r'): i for i, l in enumerate(f)}
  bs = cr.bin_size(seq)
  for g, (p, dt, ct, n, has) in enumerate(exp):
    assert ([vocab[t] for t in d['doc'][g].split(' ')] if d['doc'][g] else []) == dt, g
    assert [vocab[t] for t in d['code'][g].split(' ')] == ct, g
    assert (d['num_tokens'][g], d['bin_id'][g], d['id'][g]) == (n, po.bin_of(n, bs, 4), 'py_%d' % where[ct[0]]), g
  with pytest.raises(ValueError):
    load_shards(BertCollate(tokenizer=pk.tok), out)
  # rows with a docstring are BERT-shaped rows: doc -> A, code -> B
  has = [g for g, e in enumerate(exp) if e[4]]
  empty = [g for g in has if not exp[g][1]]
  assert empty and len(has) < len(exp)
  ab = str(tmp_path / 'ab')
  os.makedirs(ab)
  g0, kept = 0, []
  for (p, b, _), t in zip(names, tables):
    sel = [k for k in range(t.num_rows) if exp[g0 + k][4]]
    kept += [g0 + k for k in sel]
    g0 += t.num_rows
    t = t.take(pa.array(sel, pa.int64()))
    pq.write_table(pa.table({'A': t.column('doc'), 'B': t.column('code'),
                             'is_random_next': pa.array([False] * len(sel), pa.bool_()),'num_tokens': t.column('num_tokens')}),
                   os.path.join(ab, 'part.%d.parquet_%d' % (p, b)))
  assert kept == has
  col = BertCollate(tokenizer=pk.tok, sequence_length_alignment=8)
  got = load_shards(col, ab)
  assert got.n_pairs == len(has)
  for (p, a, b, fl, bn, tok), g in zip(got.rows(), has):
    assert (p, a, b, fl, bn, tok) == (exp[g][0], exp[g][1], exp[g][2], 2, po.bin_of(exp[g][3], bs, 4),
                                      cr.row_tokens(exp[g], pk.tok.cls_id, pk.tok.sep_id)), g
  pick = [has.index(g) for g in empty[:4]] + list(range(0, len(has), 5))
  S = (max(exp[has[k]][3] for k in pick) + 7) // 8 * 8
  want = layout(exp, [has[k] for k in pick], S, pk.tok.cls_id, pk.tok.sep_id)
  keys = ('input_ids', 'token_type_ids', 'attention_mask', 'special_tokens_mask')
  batch = col.collate_rows(got, pick, mode=0)
  for k, name in enumerate(keys):
    assert np.array_equal(batch[name].cpu().numpy(), want[k]), name
  assert not batch['next_sentence_labels'].cpu().numpy().any()
  # the same batch straight from the pack result
  batch = col.collate_rows(res, [has[k] for k in pick], mode=0)
  for k, name in enumerate(keys):
    assert np.array_equal(batch[name].cpu().numpy(), want[k]), name
  none = next(g for g, e in enumerate(exp) if not e[4])
  with pytest.raises(RuntimeError, match='CodeBERT'):
    col.collate_rows(res, [has[0], none], mode=0)
