"""The sentence-order packer (lddl_pack_sop, pack_sop_wave_kernel) against its
exact host model (tests/sop_pack_model.py; the reference has no such mode):
the same rows in the same order -- tokens of A and B, the swap flag,
num_tokens, bin, partition, tok_off, bin_count -- bit for bit, as spans (src0 /
src1 point at the segments' ids) and materialised ([CLS] A [SEP] B [SEP]), in
every regime of the kernel's chunk scan, pair truncation, filter and binning;
then lddl_pack_sop at the C API: its argument refusals, lddl_masked_lm[_spans]
refusing its result, lddl_row_docs, and a d_sent_off that does not start at 0.
tests/test_sop_pack_model_host.py shows that each corpus reaches its regime."""
import ctypes

import numpy as np
import pytest
import torch

import sop_pack_model as sm
from test_pack_gpu import shards_from_docs

pytestmark = pytest.mark.gpu

LDDL_EINVAL = -1


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


@pytest.fixture(scope='module')
def modelled():
  """the model's rows per (corpus, parameters), computed once"""
  cache = {}

  def get(corpus, *args):
    key = (id(corpus[0]),) + args
    if key not in cache:
      cache[key] = (corpus, sm.pack(corpus, *args))
    return cache[key][1]
  return get


def check(pk, res, want, seq, bin_size, spans):
  """a pack result against the model's partitions of rows"""
  flat = [(p, r) for p, part in enumerate(want) for r in part]
  n = len(flat)
  assert res.kind == 'bert' and res.spans == spans and (res.tokens is None) == spans
  assert res.n_pairs == n and res.nbins == (seq // bin_size if bin_size else 1) and res.n_masked == 0
  u16 = lambda t: t[:n].cpu().numpy().view(np.uint16).astype(np.int64)  # noqa: E731
  la, lb = [len(r.A) for _, r in flat], [len(r.B) for _, r in flat]
  assert u16(res.len0).tolist() == la
  assert u16(res.len1).tolist() == lb
  assert res.flags[:n].cpu().numpy().tolist() == [2 | int(r.swap) for _, r in flat]
  assert res.bins[:n].cpu().numpy().tolist() == [r.bin for _, r in flat]
  assert res.part[:n].cpu().numpy().tolist() == [p for p, _ in flat]
  nt = [a + b + 3 for a, b in zip(la, lb)]
  assert all(k <= seq for k in nt)
  assert res.tok_off[:n + 1].cpu().numpy().tolist() == np.concatenate([[0], np.cumsum(nt)]).tolist()
  assert res.n_tokens == sum(nt)
  assert res.bin_count.cpu().numpy().tolist() == sm.bin_counts(want, seq, bin_size)
  cls, sep = pk.tok.cls_id, pk.tok.sep_id
  if spans:
    ids = res.ids.cpu().numpy().view(np.uint16).astype(np.int64)
    src0, src1 = res.src0[:n].cpu().numpy(), res.src1[:n].cpu().numpy()
    for g, (_, r) in enumerate(flat):
      assert ids[src0[g]:src0[g] + len(r.A)].tolist() == r.A, g
      assert ids[src1[g]:src1[g] + len(r.B)].tolist() == r.B, g
    tok = res.host_tokens()
  else:
    tok = res.tokens[:res.n_tokens].cpu().numpy().view(np.uint16).astype(np.int64)
  rows = (np.concatenate([np.array([cls] + r.A + [sep] + r.B + [sep], np.int64) for _, r in flat]) if n
          else np.zeros(0, np.int64))
  assert np.array_equal(tok, rows)


def run(pk, uploaded, modelled, corpus, seq, ssp, dup, seed, bin_size, spans):
  sh, ids, ntok = uploaded(corpus)
  res = pk.pack(sh, ids, ntok, target_seq_length=seq, short_seq_prob=ssp, duplicate_factor=dup, seed=seed,
                bin_size=bin_size, spans=spans, sop=True)
  torch.cuda.synchronize()
  check(pk, res, modelled(corpus, seq, ssp, dup, seed, bin_size), seq, bin_size, spans)
  return res


@pytest.mark.parametrize('spans', [False, True])
def test_several_chunks_per_document(packer, uploaded, modelled, spans):
  """target_seq_length 16, sentences of 1-6 tokens, chunks of exactly 2 sentences among them"""
  run(packer, uploaded, modelled, sm.corpus_small(5), 16, 0.1, 2, 12345, 4, spans)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('ssp', [0.0, 0.5])
def test_chunks_of_more_than_64_sentences(packer, uploaded, modelled, ssp, spans):
  """target_seq_length 512: the chunk scan past its first 64 sentences, a_end from a wide range, documents of
  exactly 64, 65 and 128 kept sentences, one-sentence documents"""
  run(packer, uploaded, modelled, sm.corpus_long_docs(), 512, ssp, 2, 7, 64, spans)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seed', [3, 4])
def test_pair_truncation_across_the_twist(packer, uploaded, modelled, seed, spans):
  """an excess of 1 .. 387 coins per row, more than 312 coins per partition; A longer than, as long as and shorter
  than B, swapped and not; a first sentence alone >= target"""
  run(packer, uploaded, modelled, sm.corpus_trunc(), 16, 0.0, 2, seed, None, spans)
  run(packer, uploaded, modelled, sm.corpus_trunc(), 16, 0.3, 1, seed, 8, spans)


@pytest.mark.parametrize('spans', [False, True])
def test_filter_edges(packer, uploaded, modelled, spans):
  """empty sentences, documents and partitions, one-sentence documents; a partition of 600 documents"""
  res = run(packer, uploaded, modelled, sm.corpus_filter(), 16, 0.1, 2, 5, 4, spans)
  counts = res.bin_count.cpu().numpy().sum(axis=1)
  assert counts[1] == 0 and counts[3] == 0 and counts[0] and counts[2] and counts[4]


@pytest.mark.parametrize('n_part', [1, 5])
@pytest.mark.parametrize('seed', [0, 2**40 + 3])
@pytest.mark.parametrize('dup', [1, 3])
@pytest.mark.parametrize('ssp', [0.0, 0.1, 1.0])
def test_parameter_sweep(packer, uploaded, modelled, ssp, dup, seed, n_part):
  run(packer, uploaded, modelled, sm.corpus_small(n_part), 16, ssp, dup, seed, 4, (dup + n_part) % 2 == 0)


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,bin_size', [(16, None), (16, 4), (128, 4), (512, 4)])
def test_binning(packer, uploaded, modelled, seq, bin_size, spans):
  """unbinned, 4 bins, 32 bins, 128 bins (more than a wave's lanes: a pass per bin)"""
  run(packer, uploaded, modelled, sm.corpus_bins(seq), seq, 0.5, 1, 1, bin_size, spans)


@pytest.mark.parametrize('spans', [False, True])
def test_smallest_and_largest_target(packer, uploaded, modelled, spans):
  """target_seq_length 5 (max_num 2, the smallest the C checks admit: every row is cut to one token a side) and
  32768 (the largest: u16 fields, whole documents as one chunk)"""
  run(packer, uploaded, modelled, sm.corpus_small(5), 5, 0.5, 1, 2, None, spans)
  run(packer, uploaded, modelled, sm.corpus_long_docs(), 32768, 0.5, 1, 2, None, spans)


# ---- the C ABI ------------------------------------------------------------------
def _ptr(t):
  return ctypes.c_void_p(0 if t is None else t.data_ptr())


def call(pk, handle, sh, d_ntok, d_toff, **over):
  """lddl_pack_sop with valid arguments, those named in `over` replaced -> (rc, message, totals)"""
  from lddl_amd import _lib
  L = _lib.lib()
  a = dict(ctx=pk.tok.handle, pack=handle, ntok=_ptr(d_ntok), tok_off=_ptr(d_toff), sent_off=_ptr(sh.sent_off),
           n_sent=sh.n_sent, doc_sent_off=_ptr(sh.doc_sent_off), n_doc=sh.n_doc, part_doc_off=_ptr(sh.part_doc_off),
           n_part=sh.n_part, seq=16, ssp=0.1, dup=2, seed=3, bin_size=4, totals=(ctypes.c_int64 * 4)(*([-5] * 4)),
           stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  a.update(over)
  rc = L.lddl_pack_sop(a['ctx'], a['pack'], a['ntok'], a['tok_off'], a['sent_off'], a['n_sent'], a['doc_sent_off'],
                       a['n_doc'], a['part_doc_off'], a['n_part'], a['seq'], a['ssp'], a['dup'], a['seed'],
                       a['bin_size'], a['totals'], a['stream'])
  return rc, L.lddl_last_error().decode(), (list(a['totals']) if a['totals'] is not None else None)


@pytest.fixture(scope='module')
def inputs(packer, uploaded):
  corpus = sm.corpus_small(5)
  sh, ids, ntok = uploaded(corpus)
  toff = torch.zeros(sh.n_sent + 1, dtype=torch.int64, device='cuda')
  torch.cumsum(ntok.to(torch.int64), 0, out=toff[1:])
  return corpus, sh, ids, ntok, toff


def test_einval_code_matches_header():
  import os
  import re
  from conftest import ROOT
  src = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  m = re.search(r"#define\s+LDDL_EINVAL\s+(-?\d+)", src)
  assert m and int(m.group(1)) == LDDL_EINVAL


NULL = ctypes.c_void_p(0)
REFUSALS = [
    ('null ctx', dict(ctx=NULL), 'null'),
    ('null ntok', dict(ntok=NULL), 'null pointer'),
    ('null tok_off', dict(tok_off=NULL), 'null pointer'),
    ('null sent_off', dict(sent_off=NULL), 'null pointer'),
    ('null doc_sent_off', dict(doc_sent_off=NULL), 'null pointer'),
    ('null part_doc_off', dict(part_doc_off=NULL), 'null pointer'),
    ('null totals', dict(totals=None), 'null pointer'),
    ('target_seq_length 4', dict(seq=4), 'target_seq_length 4'),
    ('target_seq_length 32769', dict(seq=32769, bin_size=0), 'target_seq_length 32769'),
    ('bin_size not dividing', dict(bin_size=5), 'divide'),
    ('bin_size above target', dict(bin_size=32), '<= target-seq-length'),
    ('more than 255 bins', dict(seq=512, bin_size=1), '255 bins'),
    ('duplicate_factor 0', dict(dup=0), 'duplicate_factor 0'),
    ('n_part 0', dict(n_part=0), 'bad sizes'),
]


@pytest.mark.parametrize('name,over,msg', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_argument_refusals(packer, inputs, modelled, name, over, msg):
  from lddl_amd.pipeline import PackHandle
  corpus, sh, ids, ntok, toff = inputs
  h = PackHandle(packer.tok)
  rc, err, tot = call(packer, h.handle, sh, ntok, toff, **over)
  assert rc == LDDL_EINVAL and msg in err, (rc, err)
  assert tot is None or tot == [-5] * 4  # nothing written
  assert h.rows() == -1
  # the same handle then packs
  rc, err, tot = call(packer, h.handle, sh, ntok, toff)
  assert rc == 0, err
  want = modelled(corpus, 16, 0.1, 2, 3, 4)
  assert tot == [sum(map(len, want)), sum(len(r.A) + len(r.B) + 3 for p in want for r in p), 4, 0]
  assert h.rows() == tot[0]
  h.close()


def test_masked_lm_refused_and_row_docs(packer, inputs, modelled):
  from lddl_amd import _lib, writer
  corpus, sh, ids, ntok, toff = inputs
  L = _lib.lib()
  kw = dict(target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=3, bin_size=4, sop=True)
  res = packer.pack(sh, ids, ntok, toff, **kw)  # materialised: lddl_masked_lm's other precondition holds
  want = [r for part in modelled(corpus, 16, 0.1, 2, 3, 4) for r in part]
  assert res.n_pairs == len(want) and res.kind == 'bert'
  n = res.n_pairs
  off = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
  pos = torch.zeros(1024, dtype=torch.int16, device='cuda')
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  rc = L.lddl_masked_lm(packer.tok.handle, res.pack.handle, _ptr(off), _ptr(pos), _ptr(pos), st)
  assert rc == LDDL_EINVAL and 'masking=1' in L.lddl_last_error().decode()
  sp = packer.pack(sh, ids, ntok, toff, spans=True, **kw)
  rc = L.lddl_masked_lm_spans(packer.tok.handle, sp.pack.handle, _ptr(ids), _ptr(sp.src0), _ptr(sp.src1), _ptr(sp.len0),
                              _ptr(sp.part), _ptr(off), _ptr(pos), _ptr(pos), _ptr(pos), st)
  assert rc == LDDL_EINVAL and 'masking=1' in L.lddl_last_error().decode()
  assert writer.row_docs(packer, sp).tolist() == [r.doc for r in want]


@pytest.mark.parametrize('base', [1, 1025, 1 << 33])
def test_sent_off_base(packer, inputs, modelled, base):
  """d_sent_off that starts at `base`: the same rows and, from lddl_row_docs (the one reader of the byte offsets),
  the same documents"""
  from lddl_amd import pipeline, writer
  corpus, sh, ids, ntok, toff = inputs
  moved = pipeline.ShardSet(sh.data, sh.sent_off + base, sh.doc_sent_off, sh.part_doc_off, None, sh.nbytes)
  res = packer.pack(moved, ids, ntok, toff, target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=3,
                    bin_size=4, spans=True, sop=True)
  torch.cuda.synchronize()
  want = modelled(corpus, 16, 0.1, 2, 3, 4)
  check(packer, res, want, 16, 4, True)
  assert writer.row_docs(packer, res).tolist() == [r.doc for part in want for r in part]


def test_bert_sop_bert_on_one_handle(packer, inputs, modelled):
  """the kinds share the ctx and the handle's workspace: a sentence-order pack in between leaves the NSP pack's
  rows what they were"""
  corpus, sh, ids, ntok, toff = inputs
  kw = dict(target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=9, bin_size=4)

  def bert():
    res = packer.pack(sh, ids, ntok, toff, **kw)
    torch.cuda.synchronize()
    return res.rows(), res.bin_count.cpu().numpy().tolist()

  first = bert()
  assert first[0]
  res = packer.pack(sh, ids, ntok, toff, sop=True, **kw)
  check(packer, res, modelled(corpus, 16, 0.1, 2, 9, 4), 16, 4, False)
  assert bert() == first
