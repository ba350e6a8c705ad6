"""lddl_row_spans over the row table the wave packers' last binning pass
writes (SpanRec per binned position, pack_wave.hip bin_pairs): small packs
against the pack oracle and against the rows lddl_materialize writes from the
same pack result.

Partition sizes are exact by construction: a document of one sentence gives
one row per pass (bert_pairs: a chunk of one sentence is a pair with a random
next), so a partition of N such documents at duplicate_factor 1 has N rows --
1, 63, 64, 65 and 129 (the 64-row store step and its remainder), with empty
partitions before, between and after them, and one partition of longer
documents (actual next sentences).  Every packer is a wave packer and fills the table
(BERT unmasked, both masked instantiations, CodeBERT): no handle takes another path."""
import numpy as np
import pytest
import torch

from oracle import pack_oracle as po
from test_pack_gpu import shards_from_docs, codebert_oracle_rows

pytestmark = pytest.mark.gpu

MASK = (0.15, 30522, 101, 102, 103)  # ratio, |vocab|, [CLS], [SEP], [MASK] of bert-base-uncased
SIZES = [0, 1, 0, 63, 64, 65, 0, 129, 0]  # one-sentence documents per partition; a tenth partition follows


def _corpus():
  rng = np.random.default_rng(11)
  sent = lambda lo, hi: [int(x) for x in rng.integers(1000, 2000, int(rng.integers(lo, hi + 1)))]
  docs, pdo = [], [0]
  for n in SIZES:
    docs += [[sent(1, 100)] for _ in range(n)]
    pdo.append(len(docs))
  docs += [[sent(1, 40) for _ in range(int(rng.integers(2, 13)))] + [[]] for _ in range(10)]
  pdo.append(len(docs))
  return docs, pdo


DOCS, PDO = _corpus()
_exp = {}


def expected(seq, bin_size, masking=None):
  """the oracle's rows (seed 7, dup 1) in output order: (partition, A, B,
  is_random_next, num_tokens[, (A', B', positions, labels)]); once per config"""
  key = (seq, bin_size, masking)
  if key not in _exp:
    exp = []
    for p in range(len(PDO) - 1):
      D = [[s for s in DOCS[d] if s] for d in range(PDO[p], PDO[p + 1]) if any(DOCS[d])]
      prs = po.partition_pairs(D, 7 + p, lambda X, di, r: po.bert_pairs(X, di, seq, 0.1, r, masking), 1)
      rr = []
      for pr in prs:
        a, b, rn = po.pair_tokens(D, pr)
        rr.append((p, a, b, rn, len(a) + len(b) + 3) + ((pr[5],) if masking else ()))
      if bin_size:
        order, _ = po.binned_order([r[4] for r in rr], bin_size, seq // bin_size)
        rr = [rr[i] for i in order]
      exp += rr
    _exp[key] = exp
  return _exp[key]


def test_partition_sizes_from_the_oracle():
  counts = np.bincount([e[0] for e in expected(64, 8)], minlength=len(PDO) - 1).tolist()
  assert counts[:len(SIZES)] == SIZES and counts[-1] > 10
  part = [e[0] for e in expected(64, 8)]
  assert any(part[g] != part[min(g + 63, len(part) - 1)] for g in range(0, len(part), 64))  # a chunk of two partitions


@pytest.fixture(scope='module')
def packer(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_BERT
  return Packer(VOCAB_BERT, 0)


def materialized(pk, res):
  """lddl_materialize on the pack result res was read from (no new pack):
  the rows' tokens and offsets on the host"""
  from lddl_amd import _lib
  from lddl_amd.pipeline import _ptr
  n = res.n_pairs
  dev = res.ids.device
  t = {k: torch.empty(max(m, 1), dtype=dt, device=dev)
       for k, m, dt in (('tokens', res.n_tokens + 16, torch.int16), ('tok_off', n + 1, torch.int64),
                        ('len0', n, torch.int16), ('len1', n, torch.int16), ('flags', n, torch.uint8),
                        ('bins', n, torch.uint8), ('part', n, torch.int64))}
  _lib.check(_lib.lib().lddl_materialize(pk.tok.handle, res.pack.handle, _ptr(res.ids), _ptr(t['tokens']),
                                         _ptr(t['tok_off']), _ptr(t['len0']), _ptr(t['len1']), _ptr(t['flags']),
                                         _ptr(t['bins']), _ptr(t['part']), None, None))
  torch.cuda.synchronize(dev)
  return {k: v.cpu().numpy() for k, v in t.items()}


def span_columns(res):
  n = res.n_pairs
  c = {k: getattr(res, k)[:n].cpu().numpy() for k in ('src0', 'src1', 'len0', 'len1', 'flags', 'bins', 'part')}
  c['tok_off'] = res.tok_off[:n + 1].cpu().numpy()
  return c


def check_against_materialize(pk, res):
  """ids[src0 : src0 + len0] is the row's A as lddl_materialize copied it, and
  likewise B; every other per-row output is the same"""
  m = materialized(pk, res)
  s = span_columns(res)
  n = res.n_pairs
  for k in ('len0', 'len1', 'flags', 'bins', 'part'):
    assert np.array_equal(s[k], m[k][:n]), k
  assert np.array_equal(s['tok_off'], m['tok_off'][:n + 1])
  ids = res.ids.cpu().numpy().view(np.uint16)
  tok = m['tokens'].view(np.uint16)
  l0, l1 = s['len0'].view(np.uint16).astype(np.int64), s['len1'].view(np.uint16).astype(np.int64)
  for g in range(n):
    o = int(s['tok_off'][g])
    b1 = o + 1 + l0[g] + (1 if s['flags'][g] & 2 else 0)
    assert np.array_equal(ids[s['src0'][g]:s['src0'][g] + l0[g]], tok[o + 1:o + 1 + l0[g]]), ('A', g)
    assert np.array_equal(ids[s['src1'][g]:s['src1'][g] + l1[g]], tok[b1:b1 + l1[g]]), ('B', g)
    assert l0[g] > 0 or s['src0'][g] == 0
    assert s['tok_off'][g + 1] - o == b1 - o + l1[g] + 1


# one bin, 8 bins, 65 bins (the pass per bin); the order in global memory
# (the default), in LDS where a partition fits 64 pairs, in LDS for all
@pytest.mark.parametrize('caps', [None, '0,0,64', '8192,512,8192'])
@pytest.mark.parametrize('seq,bin_size', [(64, None), (64, 8), (130, 2)])
def test_row_spans_vs_oracle_and_materialize(packer, monkeypatch, seq, bin_size, caps):
  if caps:
    monkeypatch.setenv('LDDL_PACK_CAPS', caps)
  exp = expected(seq, bin_size)
  sh, ids, ntok = shards_from_docs(DOCS, part_doc_off=PDO)
  res = packer.pack(sh, ids, ntok, target_seq_length=seq, duplicate_factor=1, seed=7, bin_size=bin_size, spans=True)
  assert res.spans and res.nbins == (seq // bin_size if bin_size else 1)
  rows = res.rows()
  assert [(r[0], r[1], r[2], bool(r[3] & 1), len(r[5])) for r in rows] == [e[:5] for e in exp]
  if bin_size:
    assert [r[4] for r in rows] == [po.bin_of(e[4], bin_size, res.nbins) for e in exp]
  check_against_materialize(packer, res)


# MASK = 1 (<= 256 picks per row at seq <= 512) and MASK = 2 (seq > 512)
@pytest.mark.parametrize('seq,bin_size', [(64, 8), (520, 65)])
def test_masked_row_spans_then_masked_lm_spans(packer, seq, bin_size):
  exp = expected(seq, bin_size, MASK)
  sh, ids, ntok = shards_from_docs(DOCS, part_doc_off=PDO)
  res = packer.pack(sh, ids, ntok, target_seq_length=seq, duplicate_factor=1, seed=7, bin_size=bin_size, spans=True,
                    masking=True)
  rows = res.rows()
  assert res.n_masked == sum(len(e[5][2]) for e in exp)
  assert [(r[0], r[1], r[2], r[6], r[7]) for r in rows] == [(e[0],) + tuple(list(x) for x in e[5]) for e in exp]
  check_against_materialize(packer, res)


def test_codebert_rows_with_and_without_docstring(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_CODEBERT
  pk = Packer(VOCAB_CODEBERT, 0)
  rng = np.random.default_rng(3)
  docs, ndoc = [], []
  for d in range(150):
    nds = int(rng.choice([0, 0, 1, 3]))
    segs = [[int(x) for x in rng.integers(1000, 2000, int(rng.choice([0, 2, 9, 30])))] for _ in range(nds + 1 + d % 4)]
    segs[-1] = segs[-1] or [1500] * 7
    docs.append(segs)
    ndoc.append(nds)
  pdo = [0, 0, 1, 66, 66, 150]
  exp, counts = codebert_oracle_rows(docs, ndoc, pdo, 128, 0.1, 1, 77, 32, 4)
  sh, ids, ntok = shards_from_docs(docs, ndoc, part_doc_off=pdo)
  res = pk.pack(sh, ids, ntok, target_seq_length=128, duplicate_factor=1, seed=77, codebert=True, bin_size=32,
                spans=True)
  rows = res.rows()
  assert [(r[0], r[1], r[2], len(r[5])) for r in rows] == exp and len(exp) > 128
  flags = {r[3] for r in rows}
  assert flags == {0, 2}  # rows without and with a docstring
  assert all((r[3] == 2) == (len(r[5]) - len(r[1]) - len(r[2]) == 3) for r in rows)
  assert res.bin_count.cpu().numpy().tolist() == counts
  check_against_materialize(pk, res)


def test_first_handle_read_after_packing_into_a_second(packer):
  from lddl_amd import _lib
  from lddl_amd.pipeline import PackHandle, _ptr
  sh, ids, ntok = shards_from_docs(DOCS, part_doc_off=PDO)
  h1, h2 = PackHandle(packer.tok), PackHandle(packer.tok)
  a = packer.pack(sh, ids, ntok, target_seq_length=64, duplicate_factor=1, seed=7, bin_size=8, spans=True, into=h1)
  first = span_columns(a)
  b = packer.pack(sh, ids, ntok, target_seq_length=130, duplicate_factor=2, seed=9, bin_size=2, spans=True, into=h2)
  assert b.n_pairs != a.n_pairs
  for t in (a.src0, a.src1, a.tok_off, a.len0, a.len1, a.flags, a.bins, a.part):
    t.fill_(-1 if t.dtype != torch.uint8 else 255)
  _lib.check(_lib.lib().lddl_row_spans(packer.tok.handle, h1.handle, _ptr(a.src0), _ptr(a.src1), _ptr(a.tok_off),
                                       _ptr(a.len0), _ptr(a.len1), _ptr(a.flags), _ptr(a.bins), _ptr(a.part), None,
                                       None))
  torch.cuda.synchronize()
  again = span_columns(a)
  for k, v in first.items():
    assert np.array_equal(again[k], v), k
  assert [(r[0], r[1], r[2]) for r in a.rows()] == [e[:3] for e in expected(64, 8)]
  h1.close()
  h2.close()


def test_row_spans_refuse_after_an_assertion_error(gpu):
  """one partition of three reports PACK_EASSERT (a docstring line that leaves
  the code nothing): the pack raises and the handle serves no row spans"""
  import codebert_regimes as cr
  from lddl_amd import _lib
  from lddl_amd.pipeline import Packer, PackHandle, VOCAB_CODEBERT, _ptr
  pk = Packer(VOCAB_CODEBERT, 0)
  docs, ndoc, pdo = cr.error_corpus(128, 'AssertionError')
  sh, ids, ntok = shards_from_docs(docs, ndoc, part_doc_off=pdo)
  h = PackHandle(pk.tok)
  with pytest.raises(AssertionError):
    pk.pack(sh, ids, ntok, target_seq_length=128, short_seq_prob=1.0, duplicate_factor=cr.DUP, seed=cr.PACK_SEED,
            codebert=True, bin_size=cr.bin_size(128), spans=True, into=h)
  assert h.rows() == -1
  o = {k: torch.zeros(64, dtype=dt, device=ids.device)
       for k, dt in (('src0', torch.int64), ('src1', torch.int64), ('tok_off', torch.int64), ('len0', torch.int16),
                     ('len1', torch.int16), ('flags', torch.uint8), ('bins', torch.uint8), ('part', torch.int64))}
  L = _lib.lib()
  rc = L.lddl_row_spans(pk.tok.handle, h.handle, *[_ptr(o[k]) for k in
                                                   ('src0', 'src1', 'tok_off', 'len0', 'len1', 'flags', 'bins', 'part')],
                        None, None)
  assert rc != 0 and b'no successful lddl_pack_' in L.lddl_last_error()
  assert all(int(v.abs().sum()) == 0 for v in o.values())  # nothing written
  h.close()
