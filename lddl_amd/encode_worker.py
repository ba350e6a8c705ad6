"""Parquet encode worker (writer.ProcessEncoder): runs in a pool of host
processes, so the per-file Python work of pyarrow's writer (the part that
holds the GIL: writer construction, schema, file open / close) runs in
parallel instead of serialising a thread pool on small files.

A batch's columns arrive in a shared slot file under /dev/shm (mapped here
once per slot generation): string / binary columns as int64 offsets + bytes,
fixed-width columns as raw values.  Each task writes a run of the batch's
files, each a row range, zero-copy from the mapping.  Imports only numpy and
pyarrow (no torch, no GPU).
"""
import mmap
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from .arrow_cols import fixed_column, var_column

_MAPS = {}  # slot path -> (mmap, size)

_FIXED = {'bool': np.bool_, 'u16': np.uint16, 'i64': np.int64}
_VAR = {'str': pa.string(), 'bin': pa.binary()}


def _map(path, size):
  m = _MAPS.get(path)
  if m is None or m[1] < size:
    if m is not None:
      try:
        m[0].close()
      except BufferError:  # (a view still alive: leave it to the collector)
        pass
    fd = os.open(path, os.O_RDONLY)
    try:
      mm = mmap.mmap(fd, size, prot=mmap.PROT_READ)
    finally:
      os.close(fd)
    m = (mm, size)
    _MAPS[path] = m
  return m[0]


def write_file(path, lo, hi, cols, schema, compression, dict_cols):
  """Rows [lo, hi) of a batch as one parquet file.  cols: (kind, a, b) per
  schema column in order: 'str' / 'bin' with a = int64 offsets [n + 1] and
  b = the bytes (numpy, or a memoryview of the slot mapping), or 'bool' /
  'u16' / 'i64' with a = the values [n].  The encodes of a thread pool and of
  the worker processes both end here.  Returns the bytes written."""
  arrs = [var_column(_VAR[kind], a, b, lo, hi) if kind in _VAR else fixed_column(a[lo:hi]) for kind, a, b in cols]
  pq.write_table(pa.Table.from_arrays(arrs, schema=schema), path, compression=compression, use_dictionary=dict_cols)
  return os.path.getsize(path)


def encode(slot, size, n, cols, schema, files, compression, dict_cols):
  """cols: (name, kind, pos, data_pos) per schema column in order; kind
  'str' / 'bin' (offsets at pos, bytes at data_pos) or 'bool' / 'u16' / 'i64';
  files: (path, lo, hi) row ranges of the batch.  Returns the bytes written."""
  mm = _map(slot, size)
  view = [(kind, np.frombuffer(mm, dtype=np.int64, count=n + 1, offset=pos), memoryview(mm)[dpos:]) if kind in _VAR
          else (kind, np.frombuffer(mm, dtype=_FIXED[kind], count=n, offset=pos), None)
          for _, kind, pos, dpos in cols]
  return sum(write_file(path, lo, hi, view, schema, compression, dict_cols) for path, lo, hi in files)
