"""The CLI's sentence split on the GPU (lddl_split_len / lddl_split,
lddl_amd/csrc/split.hip): raw records -> a sentence-split pipeline.ShardSet
resident in HBM, with the exact result of the host path
(preprocess.split_records with preprocess._rule_split, or
splitnative.split_raw) followed by pipeline.upload.  The rule-based splitter
only; NLTK Punkt and the CodeBERT line split stay on the host."""
import ctypes

import numpy as np
import torch

from . import _lib, pipeline, splitnative
from .tokenizer import _ptr, _stream


def set_props(tok):
  """uploads splitnative.props_table() to tok's ctx, once per ctx"""
  if getattr(tok, '_split_props', False):
    return
  tab = np.ascontiguousarray(splitnative.props_table(), dtype=np.uint8)
  _lib.check(_lib.lib().lddl_set_split_props(tok.handle, ctypes.c_void_p(tab.ctypes.data), tab.size))
  tok._split_props = True


def join_records(raws):
  """records as bytes -> (uint8 array of them back to back, int64 rec_off)"""
  n = len(raws)
  rec_off = np.zeros(n + 1, dtype=np.int64)
  np.cumsum(np.fromiter((len(r) for r in raws), dtype=np.int64, count=n), out=rec_off[1:])
  return np.frombuffer(b''.join(raws), dtype=np.uint8), rec_off


def split_device(tok, records, whole_line=False, part_rec_off=None, stream=None):
  """records: a list of bytes, or (buf, rec_off) -- the records back to back
  (uint8 array / bytes) and their int64 offsets.  -> (pipeline.ShardSet, doc
  ids): document i is record i, so part_doc_off = part_rec_off (default: one
  partition); the ids are decoded on the host (empty strings with
  whole_line, as split_records gives).  A record that is not valid UTF-8
  raises the UnicodeDecodeError the host path's decode raises."""
  with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(tok.device)):
    return _split(tok, records, whole_line, part_rec_off)


def _split(tok, records, whole_line, part_rec_off):
  """split_device on the current stream (every buffer is allocated on it)"""
  buf, rec_off = records if isinstance(records, tuple) else join_records(records)
  buf = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf, np.uint8)
  rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
  n_rec, nbytes = len(rec_off) - 1, int(buf.size)
  part = np.asarray([0, n_rec] if part_rec_off is None else part_rec_off, dtype=np.int64)
  if part[0] != 0 or part[-1] != n_rec or np.any(np.diff(part) < 0):
    raise ValueError('part_rec_off must be a non-decreasing cover of [0, n_rec]')
  set_props(tok)
  device, L, s = tok.device, _lib.lib(), _stream()
  # one pinned staging copy of the records, async H2D on the current stream
  stage = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
  stage.numpy()[:nbytes] = buf
  d_buf = stage.to(device, non_blocking=True)
  d_rec = torch.from_numpy(rec_off).pin_memory().to(device, non_blocking=True)
  d_part = torch.from_numpy(part).pin_memory().to(device, non_blocking=True)
  dso = torch.empty(n_rec + 1, dtype=torch.int64, device=device)
  id_end = None if whole_line else torch.empty(max(n_rec, 1), dtype=torch.int64, device=device)
  mode = 1 if whole_line else 0
  tot, bad = (ctypes.c_int64 * 2)(), ctypes.c_int64(-1)
  rc = L.lddl_split_len(tok.handle, _ptr(d_buf), nbytes, _ptr(d_rec), n_rec, mode, _ptr(dso), _ptr(id_end), tot,
                        ctypes.byref(bad), s)
  if rc == -3 and 0 <= bad.value < n_rec:  # LDDL_EFORMAT: the host path's error for that record
    a, b = int(rec_off[bad.value]), int(rec_off[bad.value + 1])
    bytes(buf[a:b]).decode('utf-8')
  _lib.check(rc)
  n_sent, out_bytes = int(tot[0]), int(tot[1])
  data = torch.empty(out_bytes + 16, dtype=torch.uint8, device=device)
  sent_off = torch.empty(n_sent + 1, dtype=torch.int64, device=device)
  _lib.check(L.lddl_split(tok.handle, _ptr(d_buf), nbytes, _ptr(d_rec), n_rec, mode, _ptr(dso), n_sent, out_bytes,
                          _ptr(data), _ptr(sent_off), s))
  if whole_line:
    ids = [''] * n_rec
  else:
    ends = id_end[:n_rec].cpu().numpy()
    raw = memoryview(buf)
    ids = [str(raw[a:b], 'utf-8') for a, b in zip(rec_off[:-1].tolist(), ends.tolist())]
  return pipeline.ShardSet(data, sent_off, dso, d_part, None, out_bytes), ids
