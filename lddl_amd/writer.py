"""Parquet shards in the reference's schema, from GPU-rendered string columns.

The reference turns every packed instance into a dict of strings
(pretrain.py:348-360, pretrain_codebert.py:425-432) and writes them with
``to_parquet`` (unbinned: ``part.{i}.parquet``, pretrain.py:472-478) or
``to_parquet_binned`` (one file per bin, ``part.{i}.parquet_{b}``, every bin
written even when empty, binning.py:353-431):

  BERT      A string, B string, is_random_next bool, num_tokens uint16
            [, masked_lm_positions binary (np.save bytes of uint16[k],
               lddl/utils.py:98-102), masked_lm_labels string]
            [, bin_id int64]                               pretrain.py:450-498
  CodeBERT  id string, doc string, code string, num_tokens uint16
            [, bin_id int64]                       pretrain_codebert.py:495-537
  MLM-only  A string, num_tokens uint16 [, bin_id int64]
            (nsp=False: single-segment rows, no counterpart in the reference)

Here the rows of a pack call are already in file order on the device
(partition-major, bin-major, shuffled order within a bin), so a file is a
contiguous row range.  The string columns are rendered on the GPU by
``lddl_render_strings`` (Arrow layout: offsets + UTF-8 bytes) in row batches,
copied to the host once and wrapped zero-copy into Arrow arrays; the host only
slices offsets per file and runs the parquet encoder.
"""
import concurrent.futures
import ctypes
import io
import os
import time

import numpy as np
import pyarrow as pa
import torch

from . import _lib, encode_worker
from .arrow_cols import fixed_column, var_buffers, var_column
from .tokenizer import _on_stream, _ptr, _stream

SEG0, SEG1, ROW, SPAN = 0, 1, 2, 3
from .hostinfo import DENSE_COLS  # noqa: E402  (re-exported: writer.DENSE_COLS)

BERT_SCHEMA = [('A', pa.string()), ('B', pa.string()), ('is_random_next', pa.bool_()),
               ('num_tokens', pa.uint16())]
MLM_SCHEMA = [('masked_lm_positions', pa.binary()), ('masked_lm_labels', pa.string())]
CODEBERT_SCHEMA = [('id', pa.string()), ('doc', pa.string()), ('code', pa.string()), ('num_tokens', pa.uint16())]
MLM_ONLY_SCHEMA = [('A', pa.string()), ('num_tokens', pa.uint16())]


def _check_nsp(nsp, codebert, masking):
  if not nsp and (codebert or masking):
    raise ValueError('nsp=False (MLM-only rows) goes with neither codebert nor static masking')


def schema(codebert=False, masking=False, binned=False, nsp=True):
  _check_nsp(nsp, codebert, masking)
  f = list(CODEBERT_SCHEMA if codebert else BERT_SCHEMA if nsp else MLM_ONLY_SCHEMA)
  if masking and not codebert:
    f += MLM_SCHEMA
  if binned:
    f.append(('bin_id', pa.int64()))
  return pa.schema(f)


def _host(t, stream=None):
  """device tensor -> numpy on the host through pinned memory (torch's
  caching host allocator: the block returns to the cache when the last view
  of it -- the Arrow buffers of the files still encoding -- is gone);
  synchronises the stream"""
  h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
  s = stream or torch.cuda.current_stream()
  with torch.cuda.stream(s):  # (the copy on the stream the render ran on)
    h.copy_(t, non_blocking=True)
  s.synchronize()
  return h.numpy()


def render_call(fn, args, n_rows, device, stream=None, host=True):
  """One rendered column of n_rows rows: the C render entry point `fn` called
  twice, for the size (NULL bytes) and for the fill.  args: fn's arguments up
  to the offsets pointer, which is made here and follows them.  Returns
  (offsets int64[n_rows + 1] from 0, bytes uint8): numpy arrays on the host,
  or with host=False device tensors (the process encoder copies them into its
  shared slot)."""
  off = torch.empty(n_rows + 1, dtype=torch.int64, device=device)
  nb = ctypes.c_int64(0)
  s = _stream(stream)
  _lib.check(fn(*args, _ptr(off), None, 0, ctypes.byref(nb), s))
  data = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=device)
  _lib.check(fn(*args, _ptr(off), _ptr(data), nb.value, ctypes.byref(nb), s))
  if not host:
    return off, data[:nb.value]
  return _host(off, stream), _host(data[:nb.value], stream)


def render(packer, tokens, row_off, row0, n_rows, segment, len0=None, len1=None, flags=None, codebert=False,
           stream=None, host=True):
  """One string column of rows [row0, row0 + n_rows) on the GPU.

  Returns (offsets int64[n_rows + 1] starting at 0, bytes uint8) on the host.
  """
  args = (packer.tok.handle, _ptr(tokens), _ptr(row_off), _ptr(len0), _ptr(len1), _ptr(flags), row0, n_rows,
          segment, 1 if codebert else 0)
  return render_call(_lib.lib().lddl_render_strings, args, n_rows, packer.device, stream, host)


def render_masked(packer, res, row0, n_rows, segment, stream=None, host=True):
  """A (segment 0) / B (1) of span rows with the static masking applied
  (lddl_render_masked): (offsets, bytes) on the host as render()"""
  src, ln = (res.src0, res.len0) if segment == 0 else (res.src1, res.len1)
  args = (packer.tok.handle, _ptr(res.ids), _ptr(src), _ptr(ln), _ptr(res.len0), segment, _ptr(res.mlm_off),
          _ptr(res.mlm_pos), _ptr(res.mlm_token), row0, n_rows)
  return render_call(_lib.lib().lddl_render_masked, args, n_rows, packer.device, stream, host)


def seg_columns(packer, res, r0, n, codebert=False, stream=None, host=True):
  """the two segment string columns (A / B, or doc / code) of rows
  [r0, r0 + n): rendered from the spans over the dense ids (res.spans) or
  from the materialised rows"""
  if res.spans and res.mlm_token is not None:
    return (render_masked(packer, res, r0, n, 0, stream, host), render_masked(packer, res, r0, n, 1, stream, host))
  if res.spans:
    return (render(packer, res.ids, res.src0, r0, n, SPAN, len0=res.len0, stream=stream, host=host),
            render(packer, res.ids, res.src1, r0, n, SPAN, len0=res.len1, stream=stream, host=host))
  kw = dict(len0=res.len0, len1=res.len1, flags=res.flags, codebert=codebert, stream=stream, host=host)
  return (render(packer, res.tokens, res.tok_off, r0, n, SEG0, **kw),
          render(packer, res.tokens, res.tok_off, r0, n, SEG1, **kw))


def mlm_only_column(packer, res, r0, n, stream=None, host=True):
  """the one string column (A) of MLM-only rows [r0, r0 + n): their segment 1,
  which no [SEP] precedes (the CodeBERT layout of a row without docstring)"""
  if res.spans:
    return render(packer, res.ids, res.src1, r0, n, SPAN, len0=res.len1, stream=stream, host=host)
  return render(packer, res.tokens, res.tok_off, r0, n, SEG1, len0=res.len0, len1=res.len1, flags=res.flags,
                codebert=True, stream=stream, host=host)


@_on_stream
def row_docs(packer, res, n_copy=None, stream=None):
  """document index of every row of the pack result `res` (lddl_row_docs
  over res.pack, all rows on the device); the first n_copy of them copied to
  the host, on `stream` behind the kernel.  The pack need only be ready in
  stream order on `stream`."""
  n_rows = res.n_pairs
  out = torch.empty(max(n_rows, 1), dtype=torch.int64, device=packer.device)
  _lib.check(_lib.lib().lddl_row_docs(packer.tok.handle, res.pack.handle, _ptr(out), _stream(stream)))
  return out[:n_rows if n_copy is None else min(n_copy, n_rows)].cpu().numpy()


_NPY_HDR = {}  # device -> (uint16 tensor [(kmax + 1) * H / 2], H bytes, kmax)


def npy_header_table(device, kmax=1024):
  """np.save's header of a uint16[k] array for every k <= kmax, back to
  back on the device (what lddl_render_npy prepends to each row), or None
  when the headers differ in length (then the host path builds the column)"""
  t = _NPY_HDR.get(device)
  if t is None or t[2] < kmax:
    hdr = [_npy_header(k) for k in range(kmax + 1)]
    if len({len(h) for h in hdr}) != 1 or len(hdr[0]) % 2:
      return None
    flat = np.concatenate(hdr).view(np.uint16)
    t = (torch.from_numpy(flat.view(np.int16).copy()).to(device), len(hdr[0]), kmax)
    _NPY_HDR[device] = t
  return t


def render_npy(packer, res, row0, n_rows, stream=None, host=True):
  """masked_lm_positions of rows [row0, row0 + n_rows) as np.save bytes
  per row on the GPU (lddl_render_npy): (offsets, bytes) on the host as
  render(), or None when the header table does not apply"""
  if os.environ.get('LDDL_NPY_HOST'):  # (A/B: the host path)
    return None
  kmax = 1024
  t = npy_header_table(packer.device, kmax)
  if t is None:
    return None
  hdr, hlen, kmax = t
  args = (packer.tok.handle, _ptr(res.mlm_off), _ptr(res.mlm_pos), row0, n_rows, _ptr(hdr), hlen, kmax)
  return render_call(_lib.lib().lddl_render_npy, args, n_rows, packer.device, stream, host)


def _npy_header(k):
  b = io.BytesIO()
  np.save(b, np.zeros(k, dtype=np.uint16))  # serialize_np_array, lddl/utils.py:98-102
  return np.frombuffer(b.getvalue()[:len(b.getvalue()) - 2 * k], dtype=np.uint8)


def npy_positions(mlm_off, mlm_pos):
  """masked_lm_positions column: per row the np.save bytes of uint16[k]
  (header + 2k bytes), built vectorised.  mlm_off: int64[n+1] (from 0),
  mlm_pos: uint16[mlm_off[-1]].  Returns (int64 offsets, uint8 data)."""
  k = np.diff(mlm_off)
  uk, inv = np.unique(k, return_inverse=True)
  hdr = [_npy_header(int(v)) for v in uk]
  if len(k) and len({len(h) for h in hdr}) == 1 and len(hdr[0]) % 2 == 0:
    return _npy_positions_u16(k, inv, hdr, mlm_pos)
  hdr = dict(zip((int(v) for v in uk), hdr))
  hlen = np.array([len(hdr[int(v)]) for v in k], dtype=np.int64) if len(k) else np.zeros(0, np.int64)
  sizes = hlen + 2 * k
  off = np.zeros(len(k) + 1, dtype=np.int64)
  np.cumsum(sizes, out=off[1:])
  data = np.empty(int(off[-1]), dtype=np.uint8)
  for v, h in hdr.items():
    rows = np.nonzero(k == v)[0]
    data[(off[rows][:, None] + np.arange(len(h))[None, :]).ravel()] = np.tile(h, len(rows))
  # position bytes: row r's 2k bytes start at off[r] + hlen[r]
  if len(mlm_pos):
    rix = np.repeat(np.arange(len(k)), 2 * k)
    within = np.arange(int(2 * k.sum())) - np.repeat(2 * mlm_off[:-1], 2 * k)
    data[off[rix] + hlen[rix] + within] = np.ascontiguousarray(mlm_pos, dtype='<u2').view(np.uint8)
  return off, data


def _npy_positions_u16(k, inv, hdr, mlm_pos):
  """npy_positions when every row's header has one even length H (np.save
  pads its v1.0 header to 128 bytes for any 1-D uint16 shape): the column is
  a u16 stream whose header slots are H/2 values at each row start, filled
  by two boolean-mask assignments instead of index arrays per byte."""
  h2 = len(hdr[0]) // 2
  sizes = h2 + k  # u16 units
  off16 = np.zeros(len(k) + 1, dtype=np.int64)
  np.cumsum(sizes, out=off16[1:])
  data = np.empty(int(off16[-1]), dtype='<u2')
  is_hdr = np.zeros(int(off16[-1]) + 1, dtype=np.int8)
  is_hdr[off16[:-1]] += 1  # (starts distinct, ends distinct: each pass has no repeated index)
  is_hdr[off16[:-1] + h2] -= 1
  is_hdr = np.cumsum(is_hdr[:-1], dtype=np.int8).view(bool)
  table = np.stack([np.frombuffer(h.tobytes(), dtype='<u2') for h in hdr])
  data[is_hdr] = table[inv].ravel()
  data[~is_hdr] = np.ascontiguousarray(mlm_pos, dtype='<u2')
  return off16 * 2, data.view(np.uint8)


np_array = fixed_column  # Arrow array of a 1-D numpy array (bool, uint16, int32 or int64)


def str_array(strs):
  """Arrow string array of a list of str"""
  b = [s.encode('utf-8') for s in strs]
  off = np.zeros(len(b) + 1, dtype=np.int64)
  np.cumsum(np.fromiter(map(len, b), dtype=np.int64, count=len(b)), out=off[1:])
  return var_column(pa.string(), off, np.frombuffer(b''.join(b), dtype=np.uint8), 0, len(b))


def _worker_init():
  n = int(os.environ.get('LDDL_WORKER_NICE', '5'))  # (niced as the CLI's split workers)
  if n > 0:
    try:
      os.nice(n)
    except OSError:
      pass


def _warm(_):
  return os.getpid()


class ProcessEncoder:
  """Parquet encodes in a pool of host processes (encode_worker.encode).

  The per-file part of pyarrow's writer holds the GIL, so a thread pool
  serialises on small files (CodeBERT's, ~100 rows each); processes each
  have their own.  A batch's columns are copied once into a shared slot
  file under /dev/shm (device columns straight from the GPU, through the
  slot pinned with hipHostRegister when the runtime allows), then each task
  writes a run of the batch's files from it.  `slots` batches can be in
  flight; a slot is reused once its batch's files are written.  Create it
  before the process touches the GPU (its workers are forked); close() ends
  the workers and removes the slot files."""

  def __init__(self, workers=None, slots=3, context='fork'):
    import multiprocessing as mp
    self.workers = workers or encode_workers()
    self.ex = concurrent.futures.ProcessPoolExecutor(self.workers, mp_context=mp.get_context(context),
                                                     initializer=_worker_init)
    list(self.ex.map(_warm, range(self.workers)))  # start the workers now, not in the first batch
    d = None
    if os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK):
      st = os.statvfs('/dev/shm')
      if st.f_bavail * st.f_frsize >= (1 << 30) * slots:  # (a small /dev/shm would fault on the slot writes)
        d = '/dev/shm'
    import tempfile
    self.dir = tempfile.mkdtemp(prefix='lddl_enc_', dir=d)
    self.slots = [dict(path=os.path.join(self.dir, 'slot%d' % i), size=0, mm=None, t=None, pinned=False, futs=[])
                  for i in range(slots)]
    self.disk_dir = None  # (slots that outgrew /dev/shm: _grow)
    self.next = 0
    self.wait_s = 0.0  # waiting for a slot's previous batch to finish encoding
    self.copy_s = 0.0  # columns into the slots (device copies included)
    # the slot files are memory: removed at exit even when close() is never
    # reached (an exception on the caller's path)
    import shutil
    import weakref
    self._fin = weakref.finalize(self, shutil.rmtree, self.dir, True)

  def submit(self, fn, *a, **kw):  # (a plain task, as an executor)
    return self.ex.submit(fn, *a, **kw)

  def _unpin(self, sl):
    if sl['pinned']:
      torch.cuda.cudart().cudaHostUnregister(sl['t'].data_ptr())
      sl['pinned'] = False

  def _grow(self, sl, new):
    """The slot file at `new` bytes, its space reserved (posix_fallocate), so
    a full tmpfs is an OSError here and not a SIGBUS in the copy into the
    mapping (the /dev/shm check at construction sees neither the slots'
    growth nor the other ranks of the node).  A slot that no longer fits in
    /dev/shm moves to a directory on disk."""
    import errno
    import mmap
    for attempt in range(2):
      fd = os.open(sl['path'], os.O_RDWR | os.O_CREAT, 0o600)
      try:
        os.ftruncate(fd, new)
        try:
          os.posix_fallocate(fd, 0, new)
        except OSError as e:
          if e.errno not in (errno.ENOSPC, errno.EFBIG, errno.EDQUOT) or attempt:
            raise OSError(e.errno, 'parquet encoder slot of %d MB: no space in %s (%s)' % (
                new >> 20, os.path.dirname(sl['path']), e.strerror)) from e
          os.ftruncate(fd, 0)
          if self.disk_dir is None:
            import shutil
            import tempfile
            import weakref
            self.disk_dir = tempfile.mkdtemp(prefix='lddl_enc_')
            self._fin_disk = weakref.finalize(self, shutil.rmtree, self.disk_dir, True)
          os.close(fd)
          fd = -1
          os.remove(sl['path'])
          sl['path'] = os.path.join(self.disk_dir, os.path.basename(sl['path']))
          continue
        return mmap.mmap(fd, new)
      finally:
        if fd >= 0:
          os.close(fd)

  def _acquire(self, size):
    sl = self.slots[self.next]
    self.next = (self.next + 1) % len(self.slots)
    t0 = time.perf_counter()
    for f_ in sl['futs']:
      f_.result()
    self.wait_s += time.perf_counter() - t0
    sl['futs'] = []
    if sl['size'] < size:
      import mmap
      self._unpin(sl)
      sl['t'] = None
      if sl['mm'] is not None:
        sl['mm'].close()
      new = max(size, 2 * sl['size'], 64 << 20)
      new = (new + (1 << 21) - 1) & ~((1 << 21) - 1)
      sl['mm'] = self._grow(sl, new)
      sl['size'] = new
      sl['t'] = torch.frombuffer(sl['mm'], dtype=torch.uint8)
      if torch.cuda.is_initialized():
        try:
          sl['pinned'] = torch.cuda.cudart().cudaHostRegister(sl['t'].data_ptr(), new, 0) == 0
        except Exception:  # (not available: pageable copies)
          sl['pinned'] = False
    return sl

  def submit_batch(self, n, specs, sch, files, compression, dict_cols, stream=None):
    """specs: (name, kind, a, b) per schema column: 'str' / 'bin' with
    a = int64 offsets [n + 1] from 0 and b = bytes (device tensors or numpy),
    or 'bool' / 'u16' / 'i64' with a = numpy values [n]; files: (path, lo, hi)
    row ranges.  Returns the tasks' futures."""
    def nbytes(x):
      return x.numel() * x.element_size() if isinstance(x, torch.Tensor) else x.nbytes

    lay, pos = [], 0
    for name, kind, a, b in specs:
      p0 = (pos + 63) & ~63
      if kind in ('str', 'bin'):
        p1 = (p0 + nbytes(a) + 63) & ~63
        lay.append((name, kind, p0, p1))
        pos = p1 + nbytes(b)
      else:
        lay.append((name, kind, p0, 0))
        pos = p0 + nbytes(a)
    sl = self._acquire(max(pos, 64))
    t0 = time.perf_counter()
    dst = sl['t']
    dev = False
    st = None
    for (name, kind, a, b), (_, _, p0, p1) in zip(specs, lay):
      for x, at in ((a, p0), (b, p1)) if kind in ('str', 'bin') else ((a, p0),):
        k = nbytes(x)
        if k == 0:
          continue
        if isinstance(x, torch.Tensor):
          st = st or stream or torch.cuda.current_stream()
          with torch.cuda.stream(st):  # (the copies on the stream the columns were rendered on)
            dst[at:at + k].copy_(x.reshape(-1).view(torch.uint8), non_blocking=sl['pinned'])
          dev = True
        else:
          dst[at:at + k].numpy()[:] = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
    if dev:
      st.synchronize()
    self.copy_s += time.perf_counter() - t0
    # tasks of about equal rows, at least one file each, ~2 per worker
    ntask = max(1, min(len(files), 2 * self.workers))
    bounds = np.searchsorted(np.array([f_[2] for f_ in files]), np.linspace(0, n, ntask + 1)[1:-1], side='left')
    cuts = [0] + sorted(set(int(x) + 1 for x in bounds if 0 <= x < len(files) - 1)) + [len(files)]
    futs = [self.ex.submit(encode_worker.encode, sl['path'], sl['size'], n, lay, sch, files[a:b], compression,
                           dict_cols) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    sl['futs'] = list(futs)
    return futs

  def close(self):
    for sl in self.slots:
      for f_ in sl['futs']:
        try:
          f_.result()
        except Exception:
          pass
    t0 = time.perf_counter()
    self.ex.shutdown(wait=True)
    t1 = time.perf_counter()
    for sl in self.slots:
      self._unpin(sl)
      sl['t'] = None
      if sl['mm'] is not None:
        sl['mm'].close()
        sl['mm'] = None
    t2 = time.perf_counter()
    self._fin()
    if self.disk_dir is not None:
      self._fin_disk()
    self.close_s = (t1 - t0, t2 - t1, time.perf_counter() - t2)  # workers' exit, slot unpin / unmap, slot files


def _host_var(arr, r0, n):
  """rows [r0, r0 + n) of an Arrow string array as (int64 offsets from 0, bytes)"""
  data, off = var_buffers(arr.slice(r0, n))
  return off - off[0], data[int(off[0]):int(off[-1])]


FILE_NAMES = {'parquet': ('part.%d.parquet', 'part.%d.parquet_%d'), 'txt': ('%d.txt', '%d_%d.txt')}


class FilePlan:
  """The output files of one pack (or BART aggregate) call.  Rows are in
  file order, (partition, bin) major: file f = partition f // nbins, bin
  f % nbins = rows [file_start[f], file_start[f + 1]).  bin_count: rows per
  (partition, bin); unbinned, a partition is one file.  Only the first
  max_parts partitions are written: nfiles files, n_rows rows."""

  def __init__(self, bin_count, binned, max_parts=None, part_base=0):
    counts = np.asarray(bin_count, dtype=np.int64)
    if not binned:
      counts = counts.sum(axis=1, keepdims=True)
    self.binned, self.nbins, self.part_base = binned, counts.shape[1], part_base
    self.file_start = np.zeros(counts.size + 1, dtype=np.int64)
    np.cumsum(counts.ravel(), out=self.file_start[1:])
    self.nfiles = counts.size if max_parts is None else min(counts.size, max_parts * self.nbins)
    self.n_rows = int(self.file_start[self.nfiles])

  def batches(self, batch_rows):
    """(f, g, r0, r1): runs of whole files [f, g) = rows [r0, r1) of up to
    batch_rows rows (one file when it alone has more)"""
    fs, f = self.file_start, 0
    while f < self.nfiles:
      g = f + 1
      while g < self.nfiles and fs[g + 1] - fs[f] <= batch_rows:
        g += 1
      yield f, g, int(fs[f]), int(fs[g])
      f = g

  def files(self, f, g, out_dir, kind):
    """(path, lo, hi) of files [f, g), rows relative to file f's first;
    kind: the FILE_NAMES entry ('parquet' or 'txt')"""
    fs, out = self.file_start, []
    plain, per_bin = FILE_NAMES[kind]
    for fi in range(f, g):
      p, b = divmod(fi, self.nbins)
      name = per_bin % (self.part_base + p, b) if self.binned else plain % (self.part_base + p)
      out.append((os.path.join(out_dir, name), int(fs[fi] - fs[f]), int(fs[fi + 1] - fs[f])))
    return out


def pack_plan(res, bin_size, max_parts, part_base):
  """the FilePlan of a pipeline.PackResult"""
  n_part = res.bin_count.shape[0]
  return FilePlan(res.bin_count.cpu().numpy().reshape(n_part, res.nbins), bin_size is not None, max_parts, part_base)


@_on_stream
def mlm_positions(packer, res, r0, r1, n_rows, cache, stream=None, host=True):
  """masked_lm_positions of rows [r0, r1) as (offsets, bytes): render_npy,
  or where its header table does not apply npy_positions on the host copy of
  the call's n_rows rows (`cache`, a list, keeps it between batches)"""
  pos = render_npy(packer, res, r0, r1 - r0, stream, host=host)
  if pos is None:
    if not cache:
      moff = res.mlm_off[:n_rows + 1].cpu().numpy()
      cache.extend([moff, res.mlm_pos[:int(moff[-1])].cpu().numpy().view(np.uint16)])
    moff, mpos = cache
    m0 = int(moff[r0])
    pos = npy_positions(moff[r0:r1 + 1] - m0, mpos[m0:int(moff[r1])])
  return pos


class EncodeSink:
  """Where a writer's parquet encodes go: a thread pool of its own, whose
  files close() waits for, or the caller's executor (a ProcessEncoder or a
  thread pool), where close() hands the open futures to the caller's list.
  `host`: whether the batches' columns are wanted on the host (threads) or
  as device tensors (a ProcessEncoder copies them into its shared slot)."""

  @staticmethod
  def check(executor, pending):
    if executor is not None and pending is None:
      raise ValueError('executor needs pending: the list that takes the futures of the encodes')

  def __init__(self, executor, pending):
    self.check(executor, pending)
    self.own, self.pending = executor is None, pending
    self.proc = isinstance(executor, ProcessEncoder)
    self.host = not self.proc
    self.workers = executor.workers if self.proc else encode_workers()
    self.pool = concurrent.futures.ThreadPoolExecutor(self.workers) if self.own else executor
    self.futs = []

  def submit_batch(self, n, specs, sch, files, compression, dict_cols, stream=None):
    """The files of one batch, as ProcessEncoder.submit_batch takes them (with
    threads the specs' columns are host arrays, and a file is one task).
    Returns the seconds spent waiting for older files: threads hold at most
    4 * workers open futures, so that rendering does not run far ahead of the
    encodes (the parquet encoder releases the GIL: files encode in parallel
    on the host cores while the next batch renders on the GPU)."""
    if self.proc:
      self.futs.extend(self.pool.submit_batch(n, specs, sch, files, compression, dict_cols, stream))
      return 0.0
    cols = [spec[1:] for spec in specs]
    self.futs.extend(self.pool.submit(encode_worker.write_file, path, lo, hi, cols, sch, compression, dict_cols)
                     for path, lo, hi in files)
    t = time.perf_counter()
    while len(self.futs) > 4 * self.workers:
      self.futs.pop(0).result()
    return time.perf_counter() - t

  def close(self):
    if self.own:
      for fu in self.futs:
        fu.result()
      self.pool.shutdown()
    else:
      self.pending.extend(self.futs)


LAST_STATS = {}  # the last write_shards call's stage seconds (bench.py reports them)


@_on_stream
def write_shards(packer, res, out_dir, bin_size=None, codebert=False, masking=False, doc_ids=None,
                 part_base=0, compression='snappy', batch_rows=1 << 16, max_parts=None, stream=None,
                 executor=None, pending=None, nsp=True):
  """Write the rows of ``res`` (a pipeline.PackResult) as the reference's
  parquet files under out_dir.  nsp=False: ``res`` holds MLM-only rows
  (``Packer.pack(..., nsp=False)``); the files have the same names and hold
  A (the row's tokens) and num_tokens, no B, is_random_next or id.  Partition p of this pack call is file
  ``part.{part_base + p}.parquet`` (unbinned) or ``part.{..}.parquet_{b}``
  for every bin b (binned).  doc_ids: CodeBERT 'id' strings (list or Arrow array) per document of
  the packed corpus.  max_parts: only the first max_parts partitions.
  executor / pending: the parquet encodes go to the caller's thread pool and
  their futures to the caller's list (an executor without that list is a
  ValueError), and this call returns once the string
  columns are rendered and on the host (the device buffers are free again):
  the encodes run on while the caller's next chunk splits and packs.
  Rows are rendered in batches of whole files of about batch_rows rows, so
  the files of one batch encode while the next renders.
  stream: ``res`` need only be ready in stream order on `stream`: the renders
  and every read-back of its columns run on it.
  Returns the list of files (written once the futures are done)."""
  t_start = time.perf_counter()
  EncodeSink.check(executor, pending)
  _check_nsp(nsp, codebert, masking)
  kind = getattr(res, 'kind', 'bert')
  if (kind == 'mlm') == bool(nsp):
    raise ValueError('nsp=%s with a %r pack result' % (bool(nsp), kind))
  os.makedirs(out_dir, exist_ok=True)
  binned = bin_size is not None
  masking = masking and not codebert
  plan = pack_plan(res, bin_size, max_parts, part_base)
  assert plan.file_start[-1] == res.n_pairs, (plan.file_start[-1], res.n_pairs)
  sch = schema(codebert, masking, binned, nsp)
  # dictionary pages only where values repeat (flags, lengths, bins, the
  # CodeBERT id of a document's rows): the segment / label strings are unique
  # per row and the encoder would build and then discard a dictionary for them
  dict_cols = [n_ for n_ in sch.names if n_ not in DENSE_COLS]
  n_rows = plan.n_rows  # rows of the files written
  fixed = {'is_random_next': ('bool', (res.flags[:n_rows].cpu().numpy() & 1).astype(bool)),
           'num_tokens': ('u16', np.diff(res.tok_off[:n_rows + 1].cpu().numpy()).astype(np.uint16)),
           'bin_id': ('i64', res.bins[:n_rows].cpu().numpy().astype(np.int64))}
  if codebert:
    if doc_ids is None:
      raise ValueError('CodeBERT shards need doc_ids (the id column)')
    docs = np_array(row_docs(packer, res, n_rows, stream))
    ids_arr = doc_ids if isinstance(doc_ids, pa.Array) else str_array(doc_ids)
    ids_col = ids_arr.take(docs) if n_rows else str_array([])
  host_mlm = []  # mlm_positions' cache
  files = []
  sink = EncodeSink(executor, pending)
  st = {'setup_s': time.perf_counter() - t_start, 'render_s': 0.0, 'table_s': 0.0, 'backpressure_s': 0.0,
        'drain_s': 0.0, 'batches': 0, 'workers': sink.workers}
  seg0, seg1 = ('doc', 'code') if codebert else ('A', 'B')
  # render in batches of whole files (>= batch_rows rows, or one big file)
  for f, g, r0, r1 in plan.batches(batch_rows):
    n = r1 - r0
    flist = plan.files(f, g, out_dir, 'parquet')
    files.extend(f_[0] for f_ in flist)
    t0 = time.perf_counter()
    if nsp:
      var = dict(zip((seg0, seg1), seg_columns(packer, res, r0, n, codebert, stream, host=sink.host)))
    else:
      var = {'A': mlm_only_column(packer, res, r0, n, stream, host=sink.host)}
    if masking:
      var['masked_lm_labels'] = render(packer, res.mlm_label, res.mlm_off, r0, n, ROW, stream=stream, host=sink.host)
      var['masked_lm_positions'] = mlm_positions(packer, res, r0, r1, n_rows, host_mlm, stream, host=sink.host)
    if codebert:
      var['id'] = _host_var(ids_col, r0, n)
    specs = [(nm, 'bin' if nm == 'masked_lm_positions' else 'str') + tuple(var[nm]) if nm in var else
             (nm, fixed[nm][0], fixed[nm][1][r0:r1], None) for nm in sch.names]
    t1 = time.perf_counter()
    wait = sink.submit_batch(n, specs, sch, flist, compression, dict_cols, stream)
    t2 = time.perf_counter()
    st['render_s'] += t1 - t0
    st['table_s'] += t2 - t1 - wait
    st['backpressure_s'] += wait
    st['batches'] += 1
  t3 = time.perf_counter()
  sink.close()
  st['drain_s'] = time.perf_counter() - t3
  st['total_s'] = time.perf_counter() - t_start
  LAST_STATS.clear()
  LAST_STATS.update(st)
  return files


def encode_workers():
  """parquet encode threads: the host CPU share (hostinfo.cpu_share), or
  LDDL_ENCODE_WORKERS"""
  e = os.environ.get('LDDL_ENCODE_WORKERS')
  if e:
    return max(1, int(e))
  from .hostinfo import cpu_share
  return cpu_share()


@_on_stream
def write_txt(packer, res, out_dir, bin_size=None, codebert=False, masking=False, doc_ids=None, part_base=0,
              batch_rows=1 << 20, max_parts=None, stream=None, nsp=True):
  """The reference's txt sink (--output-format txt, pretrain.py:501-531,
  pretrain_codebert.py:540-559): one line per row,

    BERT      is_random_next: {b} - [CLS] {A} [SEP] {B} [SEP] - {num_tokens}
    masking   is_random_next: {b} - [CLS] {A} [SEP] {B} [SEP] - masked_lm_positions: {str(np.array)}
              - masked_lm_labels: {labels} - {num_tokens}
    CodeBERT  {id} [CLS] {doc} [SEP] {code} [SEP] - {num_tokens}

  joined by '\\n' with no final newline (dask's to_textfiles).  Files:
  {p}.txt per partition (to_textfiles' default name), or {p}_{b}.txt for
  every bin b (binning.py:439-476: the bin parsed back from the line's last
  field, rows in shuffled order within a bin == this packer's row order).
  Every file is created, empty ones included.  Returns the files.
  MLM-only rows (nsp=False) have no txt form: ValueError."""
  if not nsp:
    raise ValueError('write_txt: MLM-only rows (nsp=False) are written as parquet only')
  os.makedirs(out_dir, exist_ok=True)
  plan = pack_plan(res, bin_size, max_parts, part_base)
  n_rows = plan.n_rows
  num_tokens = np.diff(res.tok_off[:n_rows + 1].cpu().numpy())
  flags = res.flags[:n_rows].cpu().numpy()
  if codebert:
    if doc_ids is None:
      raise ValueError('CodeBERT txt output needs doc_ids (the id field)')
    if isinstance(doc_ids, pa.Array):
      doc_ids = doc_ids.to_pylist()
    docs = row_docs(packer, res, n_rows, stream)
  masking = masking and not codebert
  if masking:
    moff_all = res.mlm_off[:n_rows + 1].cpu().numpy()
    mpos_all = res.mlm_pos[:int(moff_all[-1])].cpu().numpy().view(np.uint16)
  files = []
  for f, g, r0, r1 in plan.batches(batch_rows):
    n = r1 - r0
    (o0, d0), (o1, d1) = seg_columns(packer, res, r0, n, codebert, stream)
    b0, b1 = d0.tobytes(), d1.tobytes()
    if masking:
      ol, dl = render(packer, res.mlm_label, res.mlm_off, r0, n, ROW, stream=stream)
      bl = dl.tobytes()
    for path, lo, hi in plan.files(f, g, out_dir, 'txt'):
      lines = []
      for i in range(lo, hi):
        r = r0 + i
        head = doc_ids[docs[r]] if codebert else 'is_random_next: {} -'.format(bool(flags[r] & 1))
        mlm = ''
        if masking:
          pos = np.array(mpos_all[moff_all[r] - moff_all[0]:moff_all[r + 1] - moff_all[0]], dtype=np.uint16)
          mlm = 'masked_lm_positions: {} - masked_lm_labels: {} - '.format(pos, bl[ol[i]:ol[i + 1]].decode())
        lines.append('{} [CLS] {} [SEP] {} [SEP] - {}{}'.format(head, b0[o0[i]:o0[i + 1]].decode(),
                                                               b1[o1[i]:o1[i + 1]].decode(), mlm, int(num_tokens[r])))
      with open(path, 'w', encoding='utf-8', newline='') as fh:
        fh.write('\n'.join(lines))
      files.append(path)
  return files
