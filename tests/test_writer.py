"""Host side of the parquet writer (no GPU): the masked_lm_positions bytes
equal lddl/utils.py:98-102 serialize_np_array, schemas match
pretrain.py:450-471 / pretrain_codebert.py:499-510."""
import io
import os

import numpy as np
import pyarrow as pa
import pytest

from lddl_amd import arrow_cols, writer


def _serialize(a):
  b = io.BytesIO()
  np.save(b, a)
  return b.getvalue()


def test_npy_positions_match_np_save():
  rng = np.random.default_rng(0)
  k = rng.integers(0, 160, 300)
  k[:3] = 0
  off = np.zeros(len(k) + 1, dtype=np.int64)
  np.cumsum(k, out=off[1:])
  pos = rng.integers(0, 1024, int(off[-1])).astype(np.uint16)
  o, d = writer.npy_positions(off, pos)
  for r in range(len(k)):
    assert d[o[r]:o[r + 1]].tobytes() == _serialize(pos[off[r]:off[r + 1]].astype(np.uint16))
  col = arrow_cols.var_column(pa.binary(), o, d, 10, 20)
  assert col.to_pylist() == [_serialize(pos[off[r]:off[r + 1]]) for r in range(10, 20)]


def test_npy_positions_empty():
  o, d = writer.npy_positions(np.zeros(1, np.int64), np.zeros(0, np.uint16))
  assert o.tolist() == [0] and len(d) == 0


def test_schemas():
  assert writer.schema().names == ['A', 'B', 'is_random_next', 'num_tokens']
  assert writer.schema(masking=True, binned=True).names == [
      'A', 'B', 'is_random_next', 'num_tokens', 'masked_lm_positions', 'masked_lm_labels', 'bin_id']
  s = writer.schema(codebert=True, binned=True)
  assert s.names == ['id', 'doc', 'code', 'num_tokens', 'bin_id']
  assert s.field('num_tokens').type == pa.uint16() and s.field('bin_id').type == pa.int64()


def test_arrow_slices_and_large_offsets():
  data = np.frombuffer(b'abcdefghij', dtype=np.uint8)
  off = np.array([0, 2, 2, 5, 10], dtype=np.int64)
  assert arrow_cols.var_column(pa.string(), off, data, 1, 4).to_pylist() == ['', 'cde', 'fghij']
  assert arrow_cols.var_column(pa.string(), off, data, 2, 2).to_pylist() == []


def test_process_encoder_writes_what_pyarrow_writes(tmp_path):
  """writer.ProcessEncoder (forked workers, the batch's columns in a shared
  slot file) writes files with the same tables as pq.write_table of the same
  row ranges, for every column kind, across slot reuse and growth"""
  import pyarrow.parquet as pq
  rng = np.random.default_rng(5)
  enc = writer.ProcessEncoder(workers=2, slots=2)
  try:
    sch = writer.schema(masking=True, binned=True)
    for batch, n in enumerate((50, 3000, 0, 700)):
      def var(binary=False):
        lens = rng.integers(0, 40, size=n)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        data = rng.integers(97, 123, size=int(off[-1])).astype(np.uint8)
        return off, data
      cols = {nm: var() for nm in ('A', 'B', 'masked_lm_positions', 'masked_lm_labels')}
      fixed = {'is_random_next': ('bool', rng.random(n) < 0.5), 'num_tokens': ('u16', rng.integers(0, 600, n).astype(np.uint16)),
               'bin_id': ('i64', rng.integers(0, 8, n).astype(np.int64))}
      specs = [(nm, 'bin' if nm == 'masked_lm_positions' else 'str') + cols[nm] if nm in cols else
               (nm, fixed[nm][0], fixed[nm][1], None) for nm in sch.names]
      cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n + 1, size=7)]))
      files = [(str(tmp_path / ('b%d_f%d.parquet' % (batch, i))), int(a), int(b))
               for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
      futs = enc.submit_batch(n, specs, sch, files, 'snappy', ['is_random_next', 'num_tokens', 'bin_id'])
      for f_ in futs:
        f_.result()
      for path, lo, hi in files:
        got = pq.read_table(path)
        arrs = []
        for nm, fd in zip(sch.names, sch):
          if nm in cols:
            off, data = cols[nm]
            arrs.append(arrow_cols.var_column(fd.type, off, data, lo, hi))
          else:
            arrs.append(writer.np_array(fixed[nm][1][lo:hi]))
        exp = pa.Table.from_arrays(arrs, schema=sch)
        assert got.equals(exp), (batch, path)
  finally:
    enc.close()
  assert not os.path.exists(enc.dir)


def test_process_encoder_slot_moves_to_disk_when_tmpfs_is_full(tmp_path, monkeypatch):
  """a slot that grows past the tmpfs' free space reserves it
  (posix_fallocate) and so sees ENOSPC as an OSError, and moves to a
  directory on disk instead of faulting (SIGBUS) in the copy"""
  import errno
  import pyarrow.parquet as pq
  enc = writer.ProcessEncoder(workers=1, slots=1)
  real = os.posix_fallocate
  full = enc.dir

  def falloc(fd, off, n):
    if os.readlink('/proc/self/fd/%d' % fd).startswith(full):
      raise OSError(errno.ENOSPC, 'No space left on device')
    return real(fd, off, n)
  monkeypatch.setattr(os, 'posix_fallocate', falloc)
  try:
    sch = writer.schema()
    n = 300
    off = np.arange(n + 1, dtype=np.int64) * 3
    data = np.frombuffer(b'abc' * n, dtype=np.uint8)
    specs = [('A', 'str', off, data), ('B', 'str', off, data), ('is_random_next', 'bool', np.zeros(n, bool), None),
             ('num_tokens', 'u16', np.full(n, 7, np.uint16), None)]
    f = str(tmp_path / 'x.parquet')
    for f_ in enc.submit_batch(n, specs, sch, [(f, 0, n)], 'snappy', ['is_random_next', 'num_tokens']):
      f_.result()
    assert enc.disk_dir is not None and enc.slots[0]['path'].startswith(enc.disk_dir)
    t = pq.read_table(f)
    assert t.column('A').to_pylist() == ['abc'] * n and t.column('num_tokens').to_pylist() == [7] * n
  finally:
    enc.close()
  assert not os.path.exists(enc.dir) and not os.path.exists(enc.disk_dir)


def test_host_var_all_empty_strings():
  """Arrow may leave the data buffer out of a slice whose strings
  are all empty"""
  a = pa.array(['', '', ''], pa.string())
  off, data = writer._host_var(a, 0, 3)
  assert off.tolist() == [0, 0, 0, 0] and data.size == 0
  b = pa.array(['x', '', '', 'yz'], pa.string())
  off, data = writer._host_var(b, 1, 2)
  assert off.tolist() == [0, 0, 0] and data.size == 0
  off, data = writer._host_var(b, 2, 2)
  assert off.tolist() == [0, 0, 2] and bytes(data) == b'yz'


# ---- the file plan and the encode sink ----------------------------------------
def _plan_loops(counts, binned, max_parts, batch_rows):
  """file_start, nfiles, n_rows and the batches as write_shards and write_txt
  each spelled them out"""
  counts = np.asarray(counts, np.int64)
  nbins = counts.shape[1] if binned else 1
  if not binned:
    counts = counts.sum(axis=1, keepdims=True)
  file_rows = counts.ravel()
  file_start = np.zeros(len(file_rows) + 1, dtype=np.int64)
  np.cumsum(file_rows, out=file_start[1:])
  nfiles = len(file_rows) if max_parts is None else min(len(file_rows), max_parts * nbins)
  batches, f = [], 0
  while f < nfiles:
    g = f + 1
    while g < nfiles and file_start[g + 1] - file_start[f] <= batch_rows:
      g += 1
    batches.append((f, g, int(file_start[f]), int(file_start[g])))
    f = g
  return file_start, nfiles, int(file_start[nfiles]), batches


PLAN_COUNTS = [[5, 0, 7, 1], [0, 0, 0, 0], [30, 2, 0, 4], [1, 1, 1, 1], [0, 9, 0, 0]]  # empty files, one of 30 rows


@pytest.mark.parametrize('part_base', [0, 11])
@pytest.mark.parametrize('max_parts', [None, 1, 3, 5, 9])
@pytest.mark.parametrize('binned', [False, True])
def test_file_plan(binned, max_parts, part_base):
  plan = writer.FilePlan(PLAN_COUNTS, binned, max_parts, part_base)
  nb = 4 if binned else 1
  for batch_rows in (1, 10, 29, 30, 1 << 16):  # (binned, the 30-row file is larger than the first four)
    fs, nfiles, n_rows, batches = _plan_loops(PLAN_COUNTS, binned, max_parts, batch_rows)
    assert np.array_equal(plan.file_start, fs) and (plan.nfiles, plan.n_rows, plan.nbins) == (nfiles, n_rows, nb)
    got = list(plan.batches(batch_rows))
    assert got == batches
    # whole files, each once and in order; no file split; the rows add up
    assert [b[0] for b in got] + [nfiles] == [0] + [b[1] for b in got]
    assert all((r0, r1) == (fs[f], fs[g]) and g > f for f, g, r0, r1 in got)
    assert all(r1 - r0 <= batch_rows or g == f + 1 for f, g, r0, r1 in got)
    assert sum(r1 - r0 for _, _, r0, r1 in got) == n_rows
    for f, g, r0, r1 in got:
      for kind in ('parquet', 'txt'):
        files = plan.files(f, g, 'out', kind)
        assert [(lo + r0, hi + r0) for _, lo, hi in files] == [(fs[i], fs[i + 1]) for i in range(f, g)]
        for i, (path, _, _) in zip(range(f, g), files):
          p, b = part_base + i // nb, i % nb
          want = {('parquet', False): 'part.%d.parquet' % p, ('parquet', True): 'part.%d.parquet_%d' % (p, b),
                  ('txt', False): '%d.txt' % p, ('txt', True): '%d_%d.txt' % (p, b)}[kind, binned]
          assert path == os.path.join('out', want)
  assert plan.nfiles == min(5, max_parts or 5) * nb
  assert plan.n_rows == sum(sum(r) for r in PLAN_COUNTS[:max_parts])


def test_file_plan_without_partitions():
  plan = writer.FilePlan(np.zeros((0, 4), np.int64), True)
  assert (plan.nfiles, plan.n_rows, list(plan.batches(10))) == (0, 0, [])
  assert writer.FilePlan(np.zeros((0, 1), np.int64), False).nfiles == 0


def test_write_shards_executor_needs_pending(tmp_path):
  """an executor without the list for its futures is refused before anything is written"""
  import concurrent.futures
  out = tmp_path / 'o'
  with concurrent.futures.ThreadPoolExecutor(1) as ex:
    with pytest.raises(ValueError):
      writer.write_shards(None, None, str(out), executor=ex)
    sink = writer.EncodeSink(ex, [])
    assert not sink.own and not sink.proc and sink.pool is ex
  assert not out.exists()
