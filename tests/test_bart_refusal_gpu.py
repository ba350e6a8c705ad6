"""lddl_bart_plan's checks of doc_chunk_off / n_chunks (capi_bart.hip, bart.hip
bart_plan_fill_kernel) where tests/test_bart_gpu.py does not go, and the word
count with a multi-byte character across every 64-byte step of one long
sentence.

  a  n_chunks = 0 with an all-zero doc_chunk_off on a table that has chunks
     is LDDL_EINVAL (the fill's walk runs whatever n_chunks is), and so is a
     doc_chunk_off that does not run forward there
  b  a table without chunks and n_chunks = 0 is accepted, chunk_off = [0]
  c  after a refused plan (one document's span a chunk too long, the next
     one's a chunk too short) chunk_off is the scan of what the walk stored
     inside the spans as given and of 0 elsewhere: the lengths' scratch slot,
     which the length pass has just used, is cleared first
  d  a 2- / 3-byte whitespace character and a 2- / 3-byte letter across each
     of the 16 steps of a 1100-byte sentence, one at a time and all at once
"""
import ctypes

import numpy as np
import pytest
import torch

import bart_model as bm
from lddl_amd import _lib
from test_bart_gpu import CH2, CH3, EINVAL, WS2, WS3, check_count, dev, last_error, plan_docs, ptr, shard_set, tok  # noqa: F401

pytestmark = pytest.mark.gpu

TSL = 8  # T = 5, what plan_docs is made for


def plan_len(tok, sh, nw):
  dco = torch.empty(sh.n_doc + 1, dtype=torch.int64, device='cuda')
  tot = (ctypes.c_int64 * 2)()
  rc = _lib.lib().lddl_bart_plan_len(tok.handle, ptr(nw), ptr(sh.sent_off), ptr(sh.doc_sent_off), sh.n_doc, sh.n_sent,
                                     TSL, ptr(dco), tot, None)
  assert rc == 0, last_error()
  return dco, int(tot[0])


def plan_fill(tok, sh, nw, dco, n_chunks, cap):
  """lddl_bart_plan into fresh arrays of cap chunks, pre-set to -1 -> (rc, sent0, nsent, ntok, chunk_off)"""
  outs = [torch.full((cap + 1,), -1, dtype=t, device='cuda') for t in (torch.int64, torch.int32, torch.int32, torch.int64)]
  rc = _lib.lib().lddl_bart_plan(tok.handle, ptr(nw), ptr(sh.sent_off), ptr(sh.doc_sent_off), ptr(dco), sh.n_doc,
                                 sh.n_sent, TSL, n_chunks, *[ptr(o) for o in outs], None)
  return (rc,) + tuple(o.cpu().numpy() for o in outs)


@pytest.fixture(scope='module')
def table(tok):
  docs, pdo = plan_docs()
  sh, host = shard_set(docs, pdo)
  nw = bm.count_words(host[0], host[1])
  return sh, host, dev(nw, np.int32), bm.plan(nw, host[1], host[2], TSL - 3)


def test_plan_with_no_chunks_still_walks(tok, table):
  sh, host, nw, want = table
  nc = len(want['chunk_sent0'])
  assert nc > 100
  zeros = torch.zeros(sh.n_doc + 1, dtype=torch.int64, device='cuda')
  rc, s0, ns, nt, co = plan_fill(tok, sh, nw, zeros, 0, nc)
  assert rc == EINVAL and 'lddl_bart_plan_len' in last_error(), (rc, last_error())
  assert (s0 == -1).all() and (ns == -1).all() and (nt == -1).all()  # no chunk array was written
  back = np.zeros(sh.n_doc + 1, dtype=np.int64)
  back[3] = 1  # runs backwards after document 2, ends at 0
  rc = plan_fill(tok, sh, nw, dev(back, np.int64), 0, nc)[0]
  assert rc == EINVAL, (rc, last_error())
  # the next call on the ctx is right
  dco, n = plan_len(tok, sh, nw)
  assert n == nc
  rc, s0, ns, nt, co = plan_fill(tok, sh, nw, dco, nc, nc)
  assert rc == 0, last_error()
  assert np.array_equal(co, want['chunk_off']) and np.array_equal(s0[:nc], want['chunk_sent0'])


def test_plan_of_a_table_without_chunks(tok):
  sh, host = shard_set([[b' ', b''], [], [b'\t']], [0, 3])
  nw = dev(bm.count_words(host[0], host[1]), np.int32)
  dco, n = plan_len(tok, sh, nw)
  assert n == 0 and dco.cpu().tolist() == [0, 0, 0, 0]
  rc, s0, ns, nt, co = plan_fill(tok, sh, nw, dco, 0, 0)
  assert rc == 0 and co.tolist() == [0], (rc, last_error(), co)


def test_chunk_off_after_a_refused_plan(tok, table):
  sh, host, nw, want = table
  nc = len(want['chunk_sent0'])
  dco_w = want['doc_chunk_off']
  lens = np.diff(want['chunk_off'])
  k = np.diff(dco_w)
  d = int(np.nonzero((k[:-1] >= 1) & (k[1:] >= 2))[0][0])  # a document with chunks, whose successor has two or more
  assert dco_w[d + 1] > dco_w[d] and dco_w[d + 2] - dco_w[d + 1] >= 2
  wrong = dco_w.copy()
  wrong[d + 1] += 1
  # what the walk stores inside the spans as given: document d's chunks and an unclaimed slot (0); the first
  # chunks of document d + 1, moved up by one, its last dropped; every other document as planned
  exp = lens.copy()
  a, b, c = int(dco_w[d]), int(dco_w[d + 1]), int(dco_w[d + 2])
  exp[b] = 0
  exp[b + 1:c] = lens[b:c - 1]
  # the slot the lengths share holds values of earlier calls, none of them 0: a whole plan's lengths (every
  # chunk has 2 bytes or more), then the length pass's chunks per document over its first entries
  assert lens.min() >= 2
  assert plan_fill(tok, sh, nw, dev(dco_w, np.int64), nc, nc)[0] == 0, last_error()
  plan_len(tok, sh, nw)
  rc, s0, ns, nt, co = plan_fill(tok, sh, nw, dev(wrong, np.int64), nc, nc)
  assert rc == EINVAL and 'lddl_bart_plan_len' in last_error(), (rc, last_error())
  assert np.array_equal(np.diff(co), exp), (np.nonzero(np.diff(co) != exp)[0][:8], a, b, c)
  assert co[0] == 0
  dco, n = plan_len(tok, sh, nw)
  rc, s0, ns, nt, co = plan_fill(tok, sh, nw, dco, nc, nc)  # and the next call is right
  assert rc == 0 and np.array_equal(co, want['chunk_off']), (rc, last_error())


def test_count_every_step_of_a_long_sentence(tok):
  total = 1100
  sents = []
  for ch in (WS2, WS3, CH2, CH3):
    for before in range(1, len(ch)):  # `before` bytes of the character lie ahead of the step's edge
      every = b''
      for edge in range(64, 1025, 64):
        head = edge - before
        sents.append(b'x' * head + ch + b'y' * (total - head - len(ch)))
        sents.append(b'x' * (head - 1) + b' ' + ch + ch + b' z' + b'y' * (total - head - 2 * len(ch) - 2))
        every += b'w' * (head - len(every)) + ch
      sents.append(every + b'v' * (total - len(every)))
  assert all(len(s) == total for s in sents)
  check_count(tok, sents)
