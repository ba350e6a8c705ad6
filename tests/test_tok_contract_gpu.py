"""Four promises of include/lddl_amd.h in front of the kernels, by exact
equality with the oracle: a corpus that does not start at offset 0 of a buffer
that is only 4-byte aligned, the out_cap cut, the max_tok range, and the
packers on the same un-rebased offsets.  Inputs and outputs lie inside margins
(tests/tok_contract.py), so a wrong offset shows as wrong ids or a trampled
guard; tests/test_tok_contract_host.py shows that the cases are not vacuous."""
import numpy as np
import pytest
import torch

import tok_contract as tc
from oracle import pack_oracle as po
from oracle.oracle import OracleTokenizer, compact
from test_oracle_golden import VOCABS

pytestmark = pytest.mark.gpu

LDDL_EINVAL = -1


@pytest.fixture(scope='module')
def toks(gpu):
  """one Tokenizer per vocabulary for the module (timing on: stats() counts the listed windows)"""
  from lddl_amd.tokenizer import Tokenizer
  made = {}

  def get(name):
    if name not in made:
      made[name] = Tokenizer(VOCABS[name])
      made[name].set_timing(True)
    return made[name]
  return get


@pytest.fixture(scope='module')
def dense_oracle():
  """(dense ids, ntok) of a corpus under a vocabulary and max_tok, computed once"""
  cache = {}

  def get(case, name, max_tok=512):
    key = (id(case), name, max_tok)
    if key not in cache:
      oids, ontok = OracleTokenizer(VOCABS[name]).run(case.data, case.sent_off, max_tok, nthreads=8)
      parts = compact(oids, ontok, case.sent_off)
      cache[key] = (np.concatenate(parts).astype(np.uint16) if parts else np.zeros(0, np.uint16), ontok.copy())
    return cache[key]
  return get


class Outputs:
  """guarded ids / ntok / tok_off of one call shape, reused across calls"""

  def __init__(self, cap, n_sent, device):
    self.ids = tc.Guarded(cap, torch.int16, tc.IDS_SENTINEL, device)
    self.ntok = tc.Guarded(n_sent, torch.int32, tc.NTOK_SENTINEL, device)
    self.toff = tc.Guarded(n_sent + 1, torch.int64, tc.TOFF_SENTINEL, device)

  def refill(self):
    for g in (self.ids, self.ntok, self.toff):
      g.refill()


def call(tok, data, nbytes, sent_off, n_sent, max_tok, out, cap, null_ids=False):
  """lddl_tokenize through the C ABI (the Python wrapper turns a short buffer into an exception)"""
  from lddl_amd import _lib
  from lddl_amd.tokenizer import _ptr, _stream
  rc = _lib.lib().lddl_tokenize(tok.handle, _ptr(data), nbytes, _ptr(sent_off), n_sent, max_tok,
                                None if null_ids else _ptr(out.ids.view), cap, _ptr(out.ntok.view),
                                _ptr(out.toff.view), _stream())
  torch.cuda.synchronize()
  return rc


def check(out, cap, want_ids, want_ntok, what):
  """ntok and tok_off complete, the ids below min(cap, T) the oracle's, the
  sentinel in every guard and in every ids entry from min(cap, T) on"""
  n, T = len(want_ntok), len(want_ids)
  ntok = out.ntok.check(n, what + ' ntok')
  bad = np.flatnonzero(ntok != want_ntok)
  assert bad.size == 0, (what, [(int(i), int(ntok[i]), int(want_ntok[i])) for i in bad[:5]])
  toff = out.toff.check(n + 1, what + ' tok_off')
  assert toff[0] == 0 and np.array_equal(np.diff(toff), want_ntok) and toff[n] == T, what
  k = min(cap, T)
  ids = out.ids.check(k, what + ' ids').view(np.uint16)
  bad = np.flatnonzero(ids != want_ids[:k])
  assert bad.size == 0, (what, 'ids differ from token %d on' % bad[0], ids[bad[:8]].tolist(), want_ids[bad[:8]].tolist())


def set_env(monkeypatch, seg):
  monkeypatch.delenv('LDDL_SPLIT_CHUNKS', raising=False)
  if seg is None:
    monkeypatch.delenv('LDDL_SPLIT_SEG', raising=False)
  else:
    monkeypatch.setenv('LDDL_SPLIT_SEG', str(seg))


# (algorithm, LDDL_SPLIT_SEG)
MODES = [(5, None), (5, 16), (5, 1), (0, None)]


@pytest.mark.parametrize('name', ['bert', 'codebert'])
def test_base_and_alignment(gpu, monkeypatch, toks, dense_oracle, name):
  """m in {0, 4, 8, 12} bytes past a 16-byte boundary, sent_off[0] = B: the
  same ntok, tok_off and ids as the oracle's on the rebased corpus at every
  placement, guards intact, and (algorithm 5) exactly the windows listed that
  the model lists at base_align = m.  CodeBERT: the four corners."""
  case = tc.base_corpus()
  want_ids, want_ntok = dense_oracle(case, name)
  T = len(want_ids)
  cap = (T + 64 + 7) & ~7
  out = Outputs(cap, case.n_sent, gpu)
  tok = toks(name)
  ms, Bs = (tc.M_VALUES, tc.B_VALUES) if name == 'bert' else ((0, 12), (0, 2053))
  for m in ms:
    for B in Bs:
      p = tc.placed(case, m, B)
      whole, view, so = tc.device_view(p, gpu)
      for algo, seg in MODES:
        set_env(monkeypatch, seg)
        assert tok.set_algo(algo) == algo
        out.refill()
        what = '%s m=%d B=%d algo=%d seg=%s' % (name, m, B, algo, seg)
        assert call(tok, view, p.nbytes, so, p.n_sent, 512, out, cap) == 0, what
        check(out, cap, want_ids, want_ntok, what)
        if algo == 5:
          assert tok.stats()['fallback_tiles'] == sum(tc.listed(case, p.sent_off, seg or (1 << 40), m)), what
      assert np.array_equal(whole.cpu().numpy(), p.buf)  # the input is read, never written


def test_out_cap_cut(gpu, monkeypatch, toks, dense_oracle):
  """ids past out_cap are not written, the offsets are still complete, the ids
  below the cut are right; then a full call on the same ctx: nothing stale"""
  case = tc.base_corpus()
  want_ids, want_ntok = dense_oracle(case, 'bert')
  T = len(want_ids)
  oids, ontok = OracleTokenizer(VOCABS['bert']).run(case.data, case.sent_off, 512, nthreads=8)
  cuts = tc.cut_points(oids, ontok)
  p = tc.placed(case, 4, 17)
  whole, view, so = tc.device_view(p, gpu)
  size = (T + 64 + 7) & ~7
  out = Outputs(size, case.n_sent, gpu)
  tok = toks('bert')
  for algo, seg in [(5, None), (5, 7), (0, None)]:
    set_env(monkeypatch, seg)
    assert tok.set_algo(algo) == algo
    for cname, cap in list(cuts.items()) + [('zero_null', 0)]:
      what = 'cut %s=%d algo=%d seg=%s' % (cname, cap, algo, seg)
      out.refill()
      assert call(tok, view, p.nbytes, so, p.n_sent, 512, out, cap, null_ids=cname == 'zero_null') == 0, what
      check(out, cap, want_ids, want_ntok, what)
      if cap < T:  # after a truncated call: the whole result, on the same ctx
        out.refill()
        assert call(tok, view, p.nbytes, so, p.n_sent, 512, out, T) == 0, what
        check(out, T, want_ids, want_ntok, what + ', then cap=T')


@pytest.mark.parametrize('algo', [5, 0])
def test_max_tok_range(gpu, monkeypatch, toks, dense_oracle, algo):
  """max_tok from 1 to the 16-bit edge on sentences of up to 70 000 tokens,
  window path and serial path; 0 and 65535 are refused"""
  case = tc.long_corpus()
  set_env(monkeypatch, None)
  tok = toks('bert')
  assert tok.set_algo(algo) == algo
  data = torch.from_numpy(np.concatenate([case.data, np.zeros(16, np.uint8)])).to(gpu)
  so = torch.from_numpy(np.ascontiguousarray(case.sent_off)).to(gpu)
  cap = (case.nbytes + 64 + 7) & ~7
  out = Outputs(cap, case.n_sent, gpu)
  for max_tok in (1, 2, 4, 5, 511, 512, 513, 2047, 2048, 65534):
    want_ids, want_ntok = dense_oracle(case, 'bert', max_tok)
    out.refill()
    what = 'max_tok=%d algo=%d' % (max_tok, algo)
    assert call(tok, data, case.nbytes, so, case.n_sent, max_tok, out, cap) == 0, what
    check(out, cap, want_ids, want_ntok, what)
  for max_tok in (0, 65535):
    out.refill()
    assert call(tok, data, case.nbytes, so, case.n_sent, max_tok, out, cap) == LDDL_EINVAL
    out.ids.check(0, 'refused ids')
    out.ntok.check(0, 'refused ntok')
    out.toff.check(0, 'refused tok_off')


# ------------------------------------------------------------ the packers --
SEQ, BIN, DUP, SEED, SSP = 128, 32, 2, 7, 0.1
MASK = (0.15, 30522, 101, 102, 103)  # ratio, |vocab|, [CLS], [SEP], [MASK] of the BERT vocabulary
CONFIGS = {'bert': dict(), 'bert_spans': dict(spans=True), 'bert_masked_spans': dict(spans=True, masking=True),
           'codebert': dict(codebert=True), 'mlm': dict(nsp=False)}
COLUMNS = ('tokens', 'tok_off', 'len0', 'len1', 'flags', 'bins', 'part', 'src0', 'src1', 'mlm_off', 'mlm_pos',
           'mlm_label', 'mlm_token')


def snapshot(res, n_sent):
  """every PackResult column and bin_count on the host (the Packer reuses its buffers)"""
  n, out = res.n_pairs, {}
  size = {'tokens': res.n_tokens, 'tok_off': n + 1, 'mlm_off': n + 1, 'mlm_pos': res.n_masked,
          'mlm_label': res.n_masked, 'mlm_token': res.n_masked}
  for k in COLUMNS:
    t = getattr(res, k)
    out[k] = None if t is None else t[:size.get(k, n)].cpu().numpy().copy()
  out['bin_count'] = res.bin_count.cpu().numpy().copy()
  total = int(res.ids_off[n_sent].item())
  out['ids'] = res.ids[:total].cpu().numpy().copy()
  out['ntok'] = res.ntok[:n_sent].cpu().numpy().copy()
  out['ids_off'] = res.ids_off[:n_sent + 1].cpu().numpy().copy()
  out['totals'] = np.array([res.n_pairs, res.n_tokens, res.nbins, res.n_masked])
  return out


def token_docs(c, oids, ontok):
  """documents as lists of id lists (empty sentences kept)"""
  sents = [[int(x) for x in s] for s in compact(oids, ontok, c.sent_off)]
  return [sents[c.doc_sent_off[d]:c.doc_sent_off[d + 1]] for d in range(c.n_doc)]


def bert_row_docs(docs, pdo, masking):
  """the document of A's first sentence per row, in output order, and the rows' (A, B) for a cross-check"""
  out, rows = [], []
  for p in range(len(pdo) - 1):
    kept = [d for d in range(pdo[p], pdo[p + 1]) if any(docs[d])]
    D = [[s for s in docs[d] if s] for d in kept]
    prs = po.partition_pairs(D, SEED + p, lambda X, di, r: po.bert_pairs(X, di, SEQ, SSP, r, masking), DUP)
    toks = [po.pair_tokens(D, pr) for pr in prs]
    order, _ = po.binned_order([len(a) + len(b) + 3 for a, b, _ in toks], BIN, SEQ // BIN)
    out += [kept[prs[i][0][0][0]] for i in order]
    rows += [toks[i][:2] for i in order]
  return out, rows


def code_row_docs(docs, ndoc, pdo):
  """the row's own document per row of the CodeBERT packer, in output order"""
  out = []
  for p in range(len(pdo) - 1):
    kept, D, nd = [], [], []
    for d in range(pdo[p], pdo[p + 1]):
      ds, cs = [x for x in docs[d][:ndoc[d]] if x], [x for x in docs[d][ndoc[d]:] if x]
      if cs:
        kept.append(d)
        D.append(ds + cs)
        nd.append(len(ds))
    prs = po.partition_pairs(D, SEED + p, lambda X, di, r: po.codebert_pairs(X, nd, di, SEQ, SSP, r), DUP)
    lens = [(dw[1] - dw[0]) + (cw[1] - cw[0]) + (3 if nd[code_s[0][0]] else 2) for _, code_s, dw, cw in prs]
    order, _ = po.binned_order(lens, BIN, SEQ // BIN)
    out += [kept[prs[i][1][0][0]] for i in order]
  return out


def check_oracle(pk, res, cfg, c, pdo, oids, ontok):
  """a pack result against the oracle's rows, by the helpers of the packers' own tests"""
  from lddl_amd import pipeline, writer
  from test_pack_gpu import codebert_oracle_rows
  import mlm_pack_model as mm
  import test_pack_mlm_gpu
  docs = token_docs(c, oids, ontok)
  if cfg.startswith('bert'):
    masking = MASK if 'masked' in cfg else None
    exp = po.run_bert_shards(c, oids, ontok, pdo, SEQ, SSP, DUP, SEED, BIN, masking=masking)
    pipeline.assert_same_pairs(res, exp)
    row_docs, rows = bert_row_docs(docs, pdo, masking)
    if masking is None:
      assert rows == [(list(r[0]), list(r[1])) for part in exp for r in part]
    assert writer.row_docs(pk, res).tolist() == row_docs
    assert len(set(row_docs)) > 40
  elif cfg == 'codebert':
    ndoc = [int(x) for x in c.doc_nseg_doc]
    exp, counts = codebert_oracle_rows(docs, ndoc, [int(x) for x in pdo], SEQ, SSP, DUP, SEED, BIN, SEQ // BIN)
    rows = res.rows()
    assert len(rows) == len(exp) > 50
    cls_id, sep_id = pk.tok.cls_id, pk.tok.sep_id
    for (p, a, b, fl, bn, tok), e in zip(rows, exp):
      assert (p, a, b, len(tok)) == e
      assert fl == (2 if e[3] - len(a) - len(b) == 3 else 0)
      assert tok == [cls_id] + (a + [sep_id] if fl & 2 else []) + b + [sep_id]
      assert bn == po.bin_of(e[3], BIN, SEQ // BIN)
    assert res.bin_count.cpu().numpy().tolist() == counts
    assert any(fl == 0 for _, _, _, fl, _, _ in rows)  # the document without docstring segments
    assert writer.row_docs(pk, res).tolist() == code_row_docs(docs, ndoc, pdo)
  else:
    corpus = (docs, [int(x) for x in pdo])
    test_pack_mlm_gpu.check(pk, res, mm.pack(corpus, SEQ, SSP, DUP, SEED, BIN), SEQ, BIN, corpus, False)


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_pack_on_unrebased_shards(gpu, monkeypatch, cfg):
  """Packer.run on a hand-built ShardSet whose sent_off starts at B in a data
  view m past a 16-byte boundary (pipeline.upload would rebase): the oracle's
  rows, lddl_row_docs' documents, and bit for bit the result of the same run
  on pipeline.upload's rebased shards"""
  from lddl_amd import pipeline
  set_env(monkeypatch, None)
  monkeypatch.delenv('LDDL_TOKENIZE_ALGO', raising=False)
  c, pdo = tc.pack_corpus()
  vocab = 'codebert' if cfg == 'codebert' else 'bert'
  oids, ontok = OracleTokenizer(VOCABS[vocab]).run(c.data, c.sent_off, 512, nthreads=8)
  pk = pipeline.Packer(VOCABS[vocab], 0, masking='masked' in cfg)
  kw = dict(target_seq_length=SEQ, short_seq_prob=SSP, duplicate_factor=DUP, seed=SEED, bin_size=BIN, **CONFIGS[cfg])
  up = pipeline.upload(c, pdo, gpu)
  res = pk.run(up, **kw)
  torch.cuda.synchronize()
  check_oracle(pk, res, cfg, c, pdo, oids, ontok)
  ref = snapshot(res, c.n_sent)
  assert np.array_equal(ref['ntok'], ontok)
  for m, B in ((4, 1), (12, 1025), (8, 2053)):
    p = tc.placed(c, m, B)
    whole, view, so = tc.device_view(p, gpu)
    sh = pipeline.ShardSet(view, so, up.doc_sent_off, up.part_doc_off, up.doc_nseg_doc, p.nbytes)
    assert int(sh.sent_off[0].item()) == B and sh.data.data_ptr() % 16 == m
    res = pk.run(sh, **kw)
    torch.cuda.synchronize()
    check_oracle(pk, res, cfg, c, pdo, oids, ontok)
    got = snapshot(res, c.n_sent)
    for k, v in ref.items():
      assert (v is None) == (got[k] is None) and (v is None or np.array_equal(v, got[k])), (cfg, m, B, k)
