"""BART pretraining data: the reference's ``preprocess_bart_pretrain``
(lddl/dask/bart/pretrain.py) on MI355X.

The reference cuts every document into chunks of whole sentences close to
``target_seq_length - 3`` words (``_aggregate_sentences``, pretrain.py:88-128)
and saves the chunk text as the one column ``sentences`` (:136-152).  Here
the sentence-split corpus sits in HBM (a pipeline.ShardSet, as for BERT) and
liblddl_amd.so counts the words (lddl_bart_count), plans the chunks
(lddl_bart_plan_len / lddl_bart_plan) and renders the column
(lddl_bart_render); this module moves buffers and writes the files.

A document is one input line taken whole: unlike the BERT path the reference
does not split off the leading id here (pretrain.py:82-86), so the id is part
of the first sentence.  Nothing is drawn at random and no vocabulary is read;
rows are in input order.
"""
import ctypes
import dataclasses
import os

import numpy as np
import pyarrow as pa
import torch

from . import _lib
from .tokenizer import _on_stream, _ptr, _stream
from .writer import EncodeSink, FilePlan, render_call

SCHEMA = pa.schema([('sentences', pa.string())])  # pretrain.py:144-146


def _handle(tokenizer_or_ctx):
  """the lddl_ctx of a Tokenizer, a pipeline.Packer or a raw handle"""
  t = getattr(tokenizer_or_ctx, 'tok', tokenizer_or_ctx)
  return getattr(t, 'handle', t)


@dataclasses.dataclass
class BartResult:
  """The chunk plan of one aggregate() call, on the device.  Chunk c (chunks
  are document-major, in input order) is sentences [chunk_sent0[c],
  chunk_sent0[c] + chunk_nsent[c]) and holds num_tokens[c] words; its text is
  bytes [chunk_off[c], chunk_off[c + 1]) of the column."""
  ctx: object
  shards: object               # the pipeline.ShardSet aggregated
  target_seq_length: int
  n_chunks: int
  nbytes: int                  # bytes of the whole column
  nwords: torch.Tensor         # int32 [n_sent]
  doc_chunk_off: torch.Tensor  # int64 [n_doc + 1]
  chunk_sent0: torch.Tensor    # int64 [n_chunks]
  chunk_nsent: torch.Tensor    # int32 [n_chunks]
  num_tokens: torch.Tensor     # int32 [n_chunks]
  chunk_off: torch.Tensor      # int64 [n_chunks + 1]
  part_chunk_off: np.ndarray   # int64 [n_part + 1] (host): doc_chunk_off taken at part_doc_off

  def render(self, c0=0, n=None, stream=None, host=True):
    """(offsets int64 [n + 1] from 0, bytes uint8) of chunks [c0, c0 + n):
    numpy arrays, or device tensors with host=False"""
    n = self.n_chunks - c0 if n is None else n
    sh = self.shards
    args = (_handle(self.ctx), _ptr(sh.data), sh.nbytes, _ptr(sh.sent_off), sh.n_sent, _ptr(self.chunk_sent0),
            _ptr(self.chunk_nsent), _ptr(self.chunk_off), self.n_chunks, c0, n)
    return render_call(_lib.lib().lddl_bart_render, args, n, sh.data.device, stream, host)


@_on_stream
def aggregate(corpus_on_device, part_doc_off=None, target_seq_length=128, tokenizer_or_ctx=None, stream=None):
  """_aggregate_sentences over every document of a sentence-split corpus on
  the device (a pipeline.ShardSet).  part_doc_off: the partitions as document
  offsets (default: the ShardSet's).  tokenizer_or_ctx: a Tokenizer, Packer or
  lddl_ctx handle (any vocabulary: it is not read).  stream: the corpus need
  only be ready in stream order on `stream`, and the plan is ready in stream
  order on it."""
  sh = corpus_on_device
  if tokenizer_or_ctx is None:
    raise ValueError('aggregate needs a Tokenizer, a Packer or an lddl_ctx handle')
  if part_doc_off is None:
    part_doc_off = sh.part_doc_off
  pdo = part_doc_off.cpu().numpy() if isinstance(part_doc_off, torch.Tensor) else np.asarray(part_doc_off, np.int64)
  n_sent, n_doc = sh.n_sent, sh.n_doc
  if len(pdo) < 1 or pdo[0] != 0 or pdo[-1] != n_doc or np.any(np.diff(pdo) < 0):
    raise ValueError('part_doc_off must be a non-decreasing cover of [0, n_doc]')
  L, h, s = _lib.lib(), _handle(tokenizer_or_ctx), _stream(stream)
  dev = sh.data.device
  nwords = torch.empty(max(n_sent, 1), dtype=torch.int32, device=dev)
  _lib.check(L.lddl_bart_count(h, _ptr(sh.data), sh.nbytes, _ptr(sh.sent_off), n_sent, _ptr(nwords), s))
  dco = torch.empty(n_doc + 1, dtype=torch.int64, device=dev)
  tot = (ctypes.c_int64 * 2)()
  _lib.check(L.lddl_bart_plan_len(h, _ptr(nwords), _ptr(sh.sent_off), _ptr(sh.doc_sent_off), n_doc, n_sent,
                                  target_seq_length, _ptr(dco), tot, s))
  nc = int(tot[0])
  sent0 = torch.empty(max(nc, 1), dtype=torch.int64, device=dev)
  nsent = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)
  ntok = torch.empty(max(nc, 1), dtype=torch.int32, device=dev)
  coff = torch.empty(nc + 1, dtype=torch.int64, device=dev)
  _lib.check(L.lddl_bart_plan(h, _ptr(nwords), _ptr(sh.sent_off), _ptr(sh.doc_sent_off), _ptr(dco), n_doc, n_sent,
                              target_seq_length, nc, _ptr(sent0), _ptr(nsent), _ptr(ntok), _ptr(coff), s))
  pco = dco[torch.from_numpy(pdo).to(dev)].cpu().numpy()
  return BartResult(tokenizer_or_ctx, sh, target_seq_length, nc, int(tot[1]), nwords[:n_sent], dco, sent0[:nc],
                    nsent[:nc], ntok[:nc], coff, pco)


def _plan(result, max_parts, part_base):
  """writer.FilePlan of a BartResult: a partition is one file of its chunks"""
  return FilePlan(np.diff(result.part_chunk_off)[:, None], False, max_parts, part_base)


def write_bart_shards(result, out_dir, part_base=0, compression='snappy', batch_rows=1 << 16, max_parts=None,
                      stream=None, executor=None, pending=None):
  """``to_parquet`` of the reference (pretrain.py:137-147): partition p of the
  result becomes ``part.{part_base + p}.parquet`` with the one string column
  ``sentences``; every partition's file is created, empty ones included.
  executor / pending as writer.write_shards: a writer.ProcessEncoder or a
  thread pool takes the encodes and their futures go to `pending` (an
  executor without that list is a ValueError); without one the files are
  written before the call returns.  Returns the files."""
  sink = EncodeSink(executor, pending)
  os.makedirs(out_dir, exist_ok=True)
  plan = _plan(result, max_parts, part_base)
  files = []
  for f, g, c0, c1 in plan.batches(batch_rows):
    flist = plan.files(f, g, out_dir, 'parquet')
    specs = [('sentences', 'str') + tuple(result.render(c0, c1 - c0, stream, host=sink.host))]
    sink.submit_batch(c1 - c0, specs, SCHEMA, flist, compression, [], stream)  # (no dictionary pages)
    files.extend(f_[0] for f_ in flist)
  sink.close()
  return files


def write_bart_txt(result, out_dir, part_base=0, batch_rows=1 << 20, max_parts=None, stream=None):
  """The reference's txt sink (pretrain.py:148-150): one chunk per line in
  ``{part_base + p}.txt``, lines joined by '\\n' with no final newline (dask's
  to_textfiles, the convention writer.write_txt documents).  Every
  partition's file is created.  Returns the files."""
  os.makedirs(out_dir, exist_ok=True)
  plan = _plan(result, max_parts, part_base)
  files = []
  for f, g, c0, c1 in plan.batches(batch_rows):
    off, data = result.render(c0, c1 - c0, stream)
    raw = data.tobytes()
    for path, lo, hi in plan.files(f, g, out_dir, 'txt'):
      with open(path, 'wb') as fh:
        fh.write(b'\n'.join(raw[off[i]:off[i + 1]] for i in range(lo, hi)))
      files.append(path)
  return files
