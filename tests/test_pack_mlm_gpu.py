"""The MLM-only packer (lddl_pack_mlm, pack_mlm_wave_kernel) against its
exact host model (tests/mlm_pack_model.py; the reference has no such mode):
the same rows in the same order, and the same len0 / len1 / flags / bins /
part / tok_off / bin_count, bit for bit, as spans (src1 points at the row's
ids) and materialised ([CLS] toks [SEP]), in every regime of the kernel's
chunk scan, truncation rounds, filter and binning.
tests/test_mlm_pack_model_host.py shows that each corpus reaches its regime."""
import numpy as np
import pytest
import torch

import mlm_pack_model as mm
from test_pack_gpu import shards_from_docs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def packer(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_BERT
  return Packer(VOCAB_BERT, 0)


@pytest.fixture(scope='module')
def uploaded():
  """corpus -> its device arrays, uploaded once per corpus"""
  cache = {}

  def get(corpus):
    key = id(corpus[0])
    if key not in cache:
      cache[key] = (corpus, shards_from_docs(corpus[0], part_doc_off=corpus[1]))
    return cache[key][1]
  return get


def check(pk, res, want, seq, bin_size, corpus, spans):
  """a pack result against the model's partitions of rows"""
  flat = [(p, r) for p, part in enumerate(want) for r in part]
  n = len(flat)
  assert res.kind == 'mlm' and res.spans == spans and (res.tokens is None) == spans
  assert res.n_pairs == n and res.nbins == (seq // bin_size if bin_size else 1) and res.n_masked == 0
  u16 = lambda t: t[:n].cpu().numpy().view(np.uint16).astype(np.int64)  # noqa: E731
  lens = [len(r.toks) for _, r in flat]
  assert not u16(res.len0).any()
  assert u16(res.len1).tolist() == lens
  assert not res.flags[:n].cpu().numpy().any()
  assert res.bins[:n].cpu().numpy().tolist() == [r.bin for _, r in flat]
  assert res.part[:n].cpu().numpy().tolist() == [p for p, _ in flat]
  assert res.tok_off[:n + 1].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum([k + 2 for k in lens])]).tolist()
  assert res.n_tokens == sum(lens) + 2 * n
  assert res.bin_count.cpu().numpy().tolist() == mm.bin_counts(want, seq, bin_size)
  cls, sep = pk.tok.cls_id, pk.tok.sep_id
  if spans:
    ids = res.ids.cpu().numpy().view(np.uint16).astype(np.int64)
    src1 = res.src1[:n].cpu().numpy()
    assert not res.src0[:n].cpu().numpy().any()  # an empty segment's offset is 0
    for g, (_, r) in enumerate(flat):
      assert ids[src1[g]:src1[g] + len(r.toks)].tolist() == r.toks, g
    tok = res.host_tokens()
  else:
    tok = res.tokens[:res.n_tokens].cpu().numpy().view(np.uint16).astype(np.int64)
  rows = np.concatenate([np.array([cls] + r.toks + [sep], np.int64) for _, r in flat]) if n else np.zeros(0, np.int64)
  assert np.array_equal(tok, rows)


def run(pk, uploaded, corpus, seq, ssp, dup, seed, bin_size, spans):
  sh, ids, ntok = uploaded(corpus)
  res = pk.pack(sh, ids, ntok, target_seq_length=seq, short_seq_prob=ssp, duplicate_factor=dup, seed=seed,
                bin_size=bin_size, spans=spans, nsp=False)
  torch.cuda.synchronize()
  check(pk, res, mm.pack(corpus, seq, ssp, dup, seed, bin_size), seq, bin_size, corpus, spans)
  return res


@pytest.mark.parametrize('spans', [False, True])
def test_several_chunks_per_document(packer, uploaded, spans):
  """(a) target_seq_length 16, sentences of 1-6 tokens"""
  run(packer, uploaded, mm.corpus_small(5), 16, 0.1, 2, 12345, 4, spans)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('ssp', [0.0, 0.5])
def test_chunks_of_more_than_64_sentences(packer, uploaded, ssp, spans):
  """(b) target_seq_length 512: find_over over several rounds of 64 sentences, one-sentence documents"""
  run(packer, uploaded, mm.corpus_long_docs(), 512, ssp, 2, 7, 64, spans)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seed', [3, 4])
def test_truncation_rounds_across_the_twist(packer, uploaded, seed, spans):
  """(c) up to 311 excess tokens per sentence, more than 312 coins per partition"""
  run(packer, uploaded, mm.corpus_trunc(), 16, 0.0, 2, seed, None, spans)
  run(packer, uploaded, mm.corpus_trunc(), 16, 0.3, 1, seed, 8, spans)


@pytest.mark.parametrize('spans', [False, True])
def test_filter_edges(packer, uploaded, spans):
  """(d) empty sentences, documents and partitions; a partition of 600 documents"""
  res = run(packer, uploaded, mm.corpus_filter(), 16, 0.1, 2, 5, 4, spans)
  counts = res.bin_count.cpu().numpy().sum(axis=1)
  assert counts[1] == 0 and counts[3] == 0 and counts[0] and counts[2] and counts[4]


@pytest.mark.parametrize('n_part', [1, 5])
@pytest.mark.parametrize('seed', [0, 2**40 + 3])
@pytest.mark.parametrize('dup', [1, 3])
@pytest.mark.parametrize('ssp', [0.0, 0.1, 1.0])
def test_parameter_sweep(packer, uploaded, ssp, dup, seed, n_part):
  """(e)"""
  run(packer, uploaded, mm.corpus_small(n_part), 16, ssp, dup, seed, 4, (dup + n_part) % 2 == 0)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,bin_size', [(16, None), (16, 4), (128, 4), (512, 4)])
def test_binning(packer, uploaded, seq, bin_size, spans):
  """(f) unbinned, 4 bins, 32 bins, 128 bins (more than a wave's lanes: a pass per bin)"""
  run(packer, uploaded, mm.corpus_bins(seq), seq, 0.5, 1, 1, bin_size, spans)


def test_smallest_and_largest_target(packer, uploaded):
  """target_seq_length 5 (max_num 3, the smallest accepted) and 32768 (the largest: u16 fields)"""
  run(packer, uploaded, mm.corpus_small(5), 5, 0.5, 1, 2, None, True)
  run(packer, uploaded, mm.corpus_long_docs(), 32768, 0.5, 1, 2, None, True)
