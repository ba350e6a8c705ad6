"""Arrow columns to and from plain buffers: what the parquet writer, its
encode workers and the shard loader share.  A string / binary column is
(int64 offsets, bytes); a fixed-width one is a numpy array.  Arrays are made
from buffers, never with pa.array(), which imports pandas on its first call
(~0.4-0.5 s per process).  Imports only numpy and pyarrow (the encode workers
have no torch and no GPU).
"""
import numpy as np
import pyarrow as pa

OFF32_LIMIT = 2**31  # bytes a string / binary array's 32-bit offsets can address
_FIXED = {np.dtype(np.uint16): pa.uint16(), np.dtype(np.int32): pa.int32(), np.dtype(np.int64): pa.int64()}
_LARGE = {pa.string(): pa.large_string(), pa.binary(): pa.large_binary()}


def var_column(typ, off, data, lo, hi):
  """Rows [lo, hi) of an (int64 offsets, bytes) column as an Arrow array of
  `typ` (pa.string() or pa.binary()), offsets rebased to row lo.  data: a
  numpy uint8 array or a memoryview (the workers' slot mapping), not copied.
  Bytes past the 32-bit offsets go through the large type and are cast back:
  a slice of a large column keeps absolute offsets, which that cast rejects
  past 2^31, so the rebase comes first."""
  o = off[lo:hi + 1] - off[lo]
  b0 = int(off[lo])
  d = pa.py_buffer(data[b0:b0 + int(o[-1])])
  if o[-1] < OFF32_LIMIT:
    return pa.Array.from_buffers(typ, hi - lo, [None, pa.py_buffer(o.astype(np.int32)), d])
  return pa.Array.from_buffers(_LARGE[typ], hi - lo, [None, pa.py_buffer(o), d]).cast(typ)


def fixed_column(x):
  """Arrow array of a 1-D numpy array (bool, uint16, int32 or int64), no copy
  except bools (bit-packed)"""
  x = np.ascontiguousarray(x)
  if x.dtype == np.bool_:
    return pa.Array.from_buffers(pa.bool_(), len(x), [None, pa.py_buffer(np.packbits(x, bitorder='little'))])
  return pa.Array.from_buffers(_FIXED[x.dtype], len(x), [None, pa.py_buffer(x)])


def var_buffers(arr):
  """pa.StringArray / BinaryArray, their large types or a ChunkedArray of
  them -> (uint8 bytes, int64 offsets [len + 1]): the array's whole data
  buffer, zero-copy, and its rows' absolute offsets into it (arr.offset
  honoured; they start at 0 only for an unsliced array)"""
  if isinstance(arr, pa.ChunkedArray):
    arr = arr.combine_chunks()
  wide = pa.types.is_large_string(arr.type) or pa.types.is_large_binary(arr.type)
  _, obuf, dbuf = arr.buffers()
  # (Arrow may leave the offsets out of an array of no rows, and the data
  # buffer out when every string is empty)
  off = np.frombuffer(obuf, dtype=np.int64 if wide else np.int32)[arr.offset:arr.offset + len(arr) + 1] \
      if obuf is not None else np.zeros(1, np.int64)
  data = np.frombuffer(dbuf, dtype=np.uint8) if dbuf is not None else np.zeros(0, np.uint8)
  return data, off.astype(np.int64)
