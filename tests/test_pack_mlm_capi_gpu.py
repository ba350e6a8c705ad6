"""lddl_pack_mlm at the C API: its argument refusals (LDDL_EINVAL with a
message, nothing launched), what the calls that read a pack result do after
it (lddl_masked_lm refused, lddl_row_docs = the model's document per row), and
a handle that serves a BERT pack, an MLM-only pack and a BERT pack again."""
import ctypes

import numpy as np
import pytest
import torch

import mlm_pack_model as mm
from test_pack_gpu import shards_from_docs

pytestmark = pytest.mark.gpu

LDDL_EINVAL = -1


@pytest.fixture(scope='module')
def packer(gpu):
  from lddl_amd.pipeline import Packer, VOCAB_BERT
  return Packer(VOCAB_BERT, 0)


def _ptr(t):
  return ctypes.c_void_p(0 if t is None else t.data_ptr())


def call(pk, handle, sh, d_ntok, d_toff, **over):
  """lddl_pack_mlm with valid arguments, those named in `over` replaced -> (rc, message, totals)"""
  from lddl_amd import _lib
  L = _lib.lib()
  a = dict(ctx=pk.tok.handle, pack=handle, ntok=_ptr(d_ntok), tok_off=_ptr(d_toff), sent_off=_ptr(sh.sent_off),
           n_sent=sh.n_sent, doc_sent_off=_ptr(sh.doc_sent_off), n_doc=sh.n_doc, part_doc_off=_ptr(sh.part_doc_off),
           n_part=sh.n_part, seq=16, ssp=0.1, dup=2, seed=3, bin_size=4, totals=(ctypes.c_int64 * 4)(*([-5] * 4)),
           stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  a.update(over)
  rc = L.lddl_pack_mlm(a['ctx'], a['pack'], a['ntok'], a['tok_off'], a['sent_off'], a['n_sent'], a['doc_sent_off'],
                       a['n_doc'], a['part_doc_off'], a['n_part'], a['seq'], a['ssp'], a['dup'], a['seed'],
                       a['bin_size'], a['totals'], a['stream'])
  return rc, L.lddl_last_error().decode(), (list(a['totals']) if a['totals'] is not None else None)


@pytest.fixture(scope='module')
def inputs(packer):
  corpus = mm.corpus_small(5)
  sh, ids, ntok = shards_from_docs(corpus[0], part_doc_off=corpus[1])
  toff = torch.zeros(sh.n_sent + 1, dtype=torch.int64, device='cuda')
  torch.cumsum(ntok.to(torch.int64), 0, out=toff[1:])
  return corpus, sh, ids, ntok, toff


def test_einval_codes_match_header():
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
def test_argument_refusals(packer, inputs, name, over, msg):
  from lddl_amd.pipeline import PackHandle
  _, sh, ids, ntok, toff = inputs
  h = PackHandle(packer.tok)
  rc, err, tot = call(packer, h.handle, sh, ntok, toff, **over)
  assert rc == LDDL_EINVAL and msg in err, (rc, err)
  assert tot is None or tot == [-5] * 4  # nothing written
  assert h.rows() == -1
  # the same handle then packs
  rc, err, tot = call(packer, h.handle, sh, ntok, toff)
  assert rc == 0, err
  want = mm.pack(inputs[0], 16, 0.1, 2, 3, 4)
  assert tot == [sum(map(len, want)), sum(len(r.toks) + 2 for p in want for r in p), 4, 0]
  assert h.rows() == tot[0]
  h.close()


def test_masked_lm_refused_and_row_docs(packer, inputs):
  from lddl_amd import _lib, writer
  corpus, sh, ids, ntok, toff = inputs
  L = _lib.lib()
  res = packer.pack(sh, ids, ntok, toff, target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=3,
                    bin_size=4, nsp=False)  # materialised: lddl_masked_lm's other precondition holds
  want = [r for part in mm.pack(corpus, 16, 0.1, 2, 3, 4) for r in part]
  assert res.n_pairs == len(want) and res.kind == 'mlm'
  n = res.n_pairs
  off = torch.zeros(n + 1, dtype=torch.int64, device='cuda')
  pos = torch.zeros(1024, dtype=torch.int16, device='cuda')
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
  rc = L.lddl_masked_lm(packer.tok.handle, res.pack.handle, _ptr(off), _ptr(pos), _ptr(pos), st)
  assert rc == LDDL_EINVAL and 'masking=1' in L.lddl_last_error().decode()
  sp = packer.pack(sh, ids, ntok, toff, target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=3,
                   bin_size=4, nsp=False, spans=True)
  rc = L.lddl_masked_lm_spans(packer.tok.handle, sp.pack.handle, _ptr(ids), _ptr(sp.src0), _ptr(sp.src1), _ptr(sp.len0),
                              _ptr(sp.part), _ptr(off), _ptr(pos), _ptr(pos), _ptr(pos), st)
  assert rc == LDDL_EINVAL and 'masking=1' in L.lddl_last_error().decode()
  assert writer.row_docs(packer, sp).tolist() == [r.doc for r in want]


def test_bert_mlm_bert_on_one_handle(packer, inputs):
  """the kinds share the ctx and the handle's workspace: an MLM-only pack in between leaves the BERT pack's rows
  what they were, and its own rows are the model's"""
  corpus, sh, ids, ntok, toff = inputs
  kw = dict(target_seq_length=16, short_seq_prob=0.1, duplicate_factor=2, seed=9, bin_size=4)

  def bert():
    res = packer.pack(sh, ids, ntok, toff, **kw)
    torch.cuda.synchronize()
    assert res.kind == 'bert'
    return res.rows(), res.bin_count.cpu().numpy().tolist()

  first = bert()
  assert first[0]
  res = packer.pack(sh, ids, ntok, toff, nsp=False, **kw)
  want = [(p, r) for p, part in enumerate(mm.pack(corpus, 16, 0.1, 2, 9, 4)) for r in part]
  cls, sep = packer.tok.cls_id, packer.tok.sep_id
  assert [(p, a, b, fl, bn, tok) for p, a, b, fl, bn, tok in res.rows()] == [
      (p, [], r.toks, 0, r.bin, [cls] + r.toks + [sep]) for p, r in want]
  assert bert() == first
