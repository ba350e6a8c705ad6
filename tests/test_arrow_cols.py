"""lddl_amd/arrow_cols.py (no GPU): the one column builder of the parquet
writer and its encode workers, the one Arrow-to-buffers decode of the writer
and the shard loader, and the two encode sinks on the same batch."""
import concurrent.futures

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from lddl_amd import arrow_cols, loader, writer

ROWS = ['ab', '', 'é☃x', 'c', '']  # an empty string, a multi-byte one, an empty last row


def _column(rows):
  b = [r.encode('utf-8') if isinstance(r, str) else r for r in rows]
  off = np.zeros(len(b) + 1, np.int64)
  np.cumsum([len(x) for x in b], out=off[1:])
  return off, np.frombuffer(b''.join(b), np.uint8)


def test_var_column_over_numpy_and_memoryview():
  """every [lo, hi) of a 5-row column, from numpy arrays and from a mapping's
  views (offsets read out of the buffer, bytes a memoryview of it)"""
  off, data = _column(ROWS)
  slot = bytearray(64) + off.tobytes() + data.tobytes()  # (as a worker's slot: the column somewhere inside)
  mv = memoryview(slot)
  m_off = np.frombuffer(mv, dtype=np.int64, count=len(ROWS) + 1, offset=64)
  m_data = mv[64 + off.nbytes:]
  for typ, want in ((pa.string(), ROWS), (pa.binary(), [r.encode('utf-8') for r in ROWS])):
    for lo in range(len(ROWS) + 1):
      for hi in range(lo, len(ROWS) + 1):
        a = arrow_cols.var_column(typ, off, data, lo, hi)
        b = arrow_cols.var_column(typ, m_off, m_data, lo, hi)
        assert a.type == typ and b.type == typ and a.equals(b), (lo, hi)
        assert a.to_pylist() == want[lo:hi], (lo, hi)
        a.validate(full=True)
        b.validate(full=True)


def test_fixed_column():
  for x in (np.array([True, False, True, True, False, False, True, False, True]), np.array([0, 7, 65535], np.uint16),
            np.array([-3, 2**31 - 1], np.int32), np.array([-3, 2**40], np.int64), np.zeros(0, np.uint16)):
    a = arrow_cols.fixed_column(x)
    assert a.to_pylist() == x.tolist() and a.type.to_pandas_dtype() == x.dtype.type
    assert arrow_cols.fixed_column(x[1:]).to_pylist() == x[1:].tolist()  # (a view that starts inside a buffer)
  assert writer.np_array is arrow_cols.fixed_column


def _rows(data, off):
  return [bytes(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize('typ', [pa.string(), pa.large_string(), pa.binary()])
def test_var_buffers(typ):
  """the rows of (bytes, offsets) are to_pylist()'s, whatever the array's
  type, offset and chunking, and when Arrow leaves the data buffer out"""
  vals = ['x', '', 'é☃', '', '', 'yz', 'w']
  if typ == pa.binary():
    vals = [v.encode('utf-8') for v in vals]
  want = [v if isinstance(v, bytes) else v.encode('utf-8') for v in vals]
  arr = pa.array(vals, typ)
  cases = {'whole': (arr, want), 'offset': (arr.slice(2, 4), want[2:6]), 'empty rows': (arr.slice(3, 2), want[3:5]),
           'no rows': (arr.slice(4, 0), []), 'all empty': (pa.array(['', ''] if typ != pa.binary() else [b'', b''], typ),
                                                           [b'', b'']),
           'chunks': (pa.chunked_array([arr.slice(1, 3), arr.slice(4, 3)]), want[1:4] + want[4:7])}
  for name, (a, rows) in cases.items():
    data, off = arrow_cols.var_buffers(a)
    assert off.dtype == np.int64 and data.dtype == np.uint8 and len(off) == len(rows) + 1, name
    assert _rows(data, off) == rows, name
  data, off = arrow_cols.var_buffers(arr.slice(2, 4))
  assert off[0] == 1 and np.shares_memory(data, np.frombuffer(arr.buffers()[2], np.uint8))  # zero-copy, absolute offsets


def test_shard_columns_of_a_sliced_table():
  """the loader stages the same rows from a slice of a table (array offsets
  not 0, two chunks) as from a copy of those rows"""
  n = 40
  rng = np.random.default_rng(3)
  words = ['a', 'bc', '', 'é☃', 'xyz ##w']

  def col():
    return [' '.join(words[k] for k in rng.integers(0, len(words), rng.integers(0, 6))) for _ in range(n)]
  names = ['A', 'B', 'masked_lm_positions', 'masked_lm_labels']
  t = pa.table({'A': pa.array(col(), pa.string()), 'B': pa.array(col(), pa.string()),
                'is_random_next': pa.array((rng.random(n) < 0.5).tolist(), pa.bool_()),
                'masked_lm_positions': pa.array([c.encode() for c in col()], pa.binary()),
                'masked_lm_labels': pa.array(col(), pa.string())})
  sl = pa.concat_tables([t.slice(5, 9), t.slice(20, 13)])
  copy = sl.combine_chunks().take(list(range(sl.num_rows)))
  (cs, rn_s, static_s), (cc, rn_c, static_c) = loader._shard_columns(sl), loader._shard_columns(copy)
  assert static_s and static_c and np.array_equal(rn_s, rn_c)
  for k, (a, b) in enumerate(zip(cs, cc)):
    want = [v.encode() if isinstance(v, str) else v for v in sl.column(names[k]).to_pylist()]
    assert _rows(*a) == _rows(*b) == want, names[k]


def test_thread_sink_and_process_encoder_write_the_same_files(tmp_path):
  """one batch of 7 rows cut into 3 files, one of them empty, with every
  column kind, through writer.EncodeSink over a thread pool and over a
  ProcessEncoder: equal tables, the expected rows, the same parquet schema"""
  sch = pa.schema([('s', pa.string()), ('b', pa.binary()), ('f', pa.bool_()), ('u', pa.uint16()), ('i', pa.int64())])
  s = ['ab', '', 'é☃x', 'c', '', 'hello world', 'z']
  b = [b'\x00\x01', b'', b'\xff', b'abc', b'', b'\x93NUMPY', b'q']
  f = np.array([True, False, False, True, True, False, True])
  u = np.array([0, 1, 65535, 7, 7, 512, 3], np.uint16)
  i = np.array([0, -1, 2**40, 7, 7, 7, 3], np.int64)
  specs = [('s', 'str') + _column(s), ('b', 'bin') + _column(b), ('f', 'bool', f, None), ('u', 'u16', u, None),
           ('i', 'i64', i, None)]
  cuts = [(0, 3), (3, 3), (3, 7)]
  want = {'s': s, 'b': b, 'f': f.tolist(), 'u': u.tolist(), 'i': i.tolist()}

  def write(executor, sub):
    (tmp_path / sub).mkdir()
    files = [(str(tmp_path / sub / ('part.%d.parquet' % k)), lo, hi) for k, (lo, hi) in enumerate(cuts)]
    pending = []
    sink = writer.EncodeSink(executor, pending)
    assert sink.host == (sub == 'threads')
    assert sink.submit_batch(7, specs, sch, files, 'snappy', ['f', 'u', 'i']) >= 0.0
    sink.close()
    for fu in pending:
      fu.result()
    return [p for p, _, _ in files]

  with concurrent.futures.ThreadPoolExecutor(2) as ex:
    threads = write(ex, 'threads')
  enc = writer.ProcessEncoder(workers=2, slots=2)
  try:
    procs = write(enc, 'procs')
  finally:
    enc.close()
  for pt, pp, (lo, hi) in zip(threads, procs, cuts):
    tt, tp = pq.read_table(pt), pq.read_table(pp)
    assert tt.schema == sch and tt.equals(tp), (lo, hi)
    assert tt.to_pydict() == {k: v[lo:hi] for k, v in want.items()}, (lo, hi)
    mt, mp = pq.read_metadata(pt), pq.read_metadata(pp)
    assert mt.schema.equals(mp.schema) and mt.num_rows == mp.num_rows == hi - lo
    assert mt.schema.to_arrow_schema() == sch
