"""Every entry point that reads a value back through the ctx's pinned words
(lddl_ctx::h_tot, allocated by lddl_create: capi_ctx.h HostWord), as the
first call of a new ctx.

The reference is the same call on a second ctx that has already completed a
pack and a render; the results are compared exactly.  The inputs are the
smallest valid ones: 3 rows with segment lengths (1, 1), (0, 5), (7, 2) over
the 'tiny64' vocabulary (tests/synth_vocab.py), 5 lengths in 2 bins, 2
partitions of 2 documents.  lddl_render_strings / lddl_render_masked are in
test_render_gpu.py (case g).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import synth_vocab as sv
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEGS = ((1, 1), (0, 5), (7, 2))
VOCAB = 'tiny64'
DOCS = [[[10, 11, 12], [13, 14]], [[15, 16, 17, 18]], [[19], [20, 21, 22], [23, 24]], [[25, 26], [27, 28, 29]]]


def new_packer():
  from lddl_amd import pipeline
  return pipeline.Packer(sv.vocab_path(VOCAB), 0)


def pack(pk):
  from test_pack_gpu import shards_from_docs
  sh, ids, ntok = shards_from_docs(DOCS, part_doc_off=[0, 2, 4])
  res = pk.pack(sh, ids, ntok, target_seq_length=16, duplicate_factor=2, seed=7, bin_size=8)
  return res.rows()


@functools.lru_cache(maxsize=None)
def warm():
  """the ctx of the references: it has packed and rendered"""
  from test_render_gpu import ROW, rows_table
  from lddl_amd import writer
  pk = new_packer()
  assert len(pack(pk)) > 0
  t = rows_table([[5, 6], [7]])
  assert writer.render(pk, t.tokens, t.tok_off, 0, t.n, ROW)[1].size > 0
  return pk


@functools.lru_cache(maxsize=None)
def table():
  """the 3 rows as a PackResult with spans and one static mask per row, built as test_collate_rows_gpu.hand_made
  builds its own (device tensors: no ctx involved)"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  n = len(SEGS)
  lens = np.asarray([a + b + 3 for a, b in SEGS], np.int64)
  src0 = np.asarray([1, 3, 9], np.int64)
  src1 = np.asarray([2, 3, 16], np.int64)
  ids = np.concatenate([6 + np.arange(18) % 50, np.zeros(16, np.int64)]).astype(np.uint16)

  def t(a, dt=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.astype(dt or a.dtype)).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t(np.asarray([a for a, _ in SEGS], np.uint16)), t(np.asarray([b for _, b in SEGS], np.uint16)),
      t(np.asarray([2, 3, 2], np.uint8)), t(np.zeros(n, np.uint8)), t(np.zeros(n, np.int64)), t(np.asarray([[n]], np.int64)))
  res.ids, res.src0, res.src1 = t(ids), t(src0), t(src1)
  res.cls_id, res.sep_id = 2, 3
  res.n_masked, res.mlm_off = n, t(np.arange(n + 1, dtype=np.int64))
  res.mlm_pos = t(np.asarray([1, 2, 3], np.uint16))
  res.mlm_label = t(np.asarray([30, 31, 32], np.uint16))
  res.mlm_token = t(np.asarray([4, 33, 4], np.uint16))
  return res


def host(x):
  if isinstance(x, dict):
    return {k: host(v) for k, v in sorted(x.items())}
  if isinstance(x, (tuple, list)):
    return [host(v) for v in x]
  return x.cpu().numpy().tolist() if torch.is_tensor(x) else x.tolist() if isinstance(x, np.ndarray) else x


def collate(pk, **kw):
  from lddl_amd.loader import BertCollate
  col = BertCollate(tokenizer=pk.tok, sequence_length_alignment=1, base_seed=31, **kw)
  col.counter = 9
  return col


SAMPLES = [('a', 'b', False), ('', 'a b c d e', True), ('a b c d e f g', 'the of', False)]
ROWS = [2, 0, 1]


def op_bin(pk):
  return pk.bin(torch.tensor([3, 9, 5, 12, 7], dtype=torch.int64, device='cuda'), 8, 2)


def op_render_npy(pk):
  from lddl_amd import writer
  return writer.render_npy(pk, table(), 0, len(SEGS))


def op_collate_seq_len(pk):
  return collate(pk)(SAMPLES)  # lddl_collate_seq_len, then lddl_collate_bert


def op_collate_bert(pk):
  from lddl_amd.loader import _column
  from lddl_amd.tokenizer import _stream
  col = collate(pk)
  rn = np.asarray([s[2] for s in SAMPLES], np.uint8)
  dev, hostbuf, p = col._upload([_column([s[0] for s in SAMPLES], True), _column([s[1] for s in SAMPLES], True)], rn)
  n, S = len(SAMPLES), 12
  out = torch.zeros((4, n, S), dtype=torch.int64, device='cuda')
  nsl = torch.zeros(n, dtype=torch.int64, device='cuda')
  P = ctypes.c_void_p
  rc = _lib.lib().lddl_collate_bert(pk.tok.handle, P(p[0]), P(p[1]), P(p[2]), P(p[3]), P(p[-1]), P(0), P(0), P(0), P(0),
                                    n, S, 2, -1, 0.15, 31, 9, P(out[0].data_ptr()), P(out[1].data_ptr()),
                                    P(out[2].data_ptr()), P(out[3].data_ptr()), P(nsl.data_ptr()), _stream())
  return rc, out, nsl


def op_collate_rows_seq_len(pk):
  return collate(pk).collate_rows(table(), ROWS, mode=1)  # lddl_collate_rows_seq_len, then lddl_collate_rows


def op_collate_rows(pk):
  from test_collate_rows_gpu import raw_collate
  return raw_collate(collate(pk), table(), ROWS, 12, mode=2)


def op_cu_seqlens(pk):
  from test_collate_unpadded_gpu import raw_cu
  cu = torch.zeros(len(ROWS) + 1, dtype=torch.int32, device='cuda')
  return raw_cu(pk, table(), torch.tensor(ROWS, dtype=torch.int64, device='cuda'), cu=cu), cu


def op_unpadded(pk):
  from test_collate_unpadded_gpu import raw_fill
  res = table()
  total = sum(a + b + 3 for a, b in SEGS)
  cu = torch.tensor(np.concatenate([[0], np.cumsum([sum(SEGS[g]) + 3 for g in ROWS])]), dtype=torch.int32, device='cuda')
  outs = [torch.zeros(total, dtype=torch.int64, device='cuda') for _ in range(4)]
  nsl = torch.zeros(len(ROWS), dtype=torch.int64, device='cuda')
  rc = raw_fill(pk, res, torch.tensor(ROWS, dtype=torch.int64, device='cuda'), cu, total, 1, outs, nsl)
  return rc, outs, nsl


OPS = {'lddl_bin': op_bin, 'lddl_render_npy': op_render_npy, 'lddl_collate_seq_len': op_collate_seq_len,
       'lddl_collate_bert': op_collate_bert, 'lddl_collate_rows_seq_len': op_collate_rows_seq_len,
       'lddl_collate_rows': op_collate_rows, 'lddl_collate_rows_cu_seqlens': op_cu_seqlens,
       'lddl_collate_rows_unpadded': op_unpadded, 'lddl_pack_bert': pack}


@pytest.mark.parametrize('call', sorted(OPS))
def test_first_call_of_a_new_ctx(gpu, call):
  exp = host(OPS[call](warm()))
  got = host(OPS[call](new_packer()))
  torch.cuda.synchronize()
  assert got == exp, call
  flat = str(exp)
  assert any(ch.isdigit() and ch != '0' for ch in flat), exp  # (the call produced something)
  if call in ('lddl_collate_bert', 'lddl_collate_rows', 'lddl_collate_rows_unpadded'):
    assert exp[0] == 0, (exp[0], _lib.lib().lddl_last_error())
  if call == 'lddl_collate_rows_cu_seqlens':
    assert exp[0] == [0, 25, 12] and exp[1] == [0, 12, 17, 25], exp  # rows 2, 0, 1: 12, 5 and 8 tokens
