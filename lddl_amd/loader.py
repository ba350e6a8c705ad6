"""Training-time collate of LDDL parquet rows on the GPU.

Drop-in for the collate the reference installs in
``get_bert_pretrain_data_loader`` (lddl/torch/bert.py:354-371
``_batch_preprocess``): ``_to_encoded_inputs`` (bert.py:69-153) turns a batch
of samples ``(A, B, is_random_next[, masked_lm_positions, masked_lm_labels])``
into padded int64 tensors, and ``_mask_tokens`` (bert.py:156-196) applies the
dynamic 80/10/10 masking when the shards carry no static masks.  Here both are
one HIP kernel (``lddl_collate_bert``, csrc/collate.hip): the batch's string
columns are staged in one pinned buffer, copied once, split / looked up /
padded / masked on the device, and the outputs stay in HBM for the model.

``BertCollate.load_rows`` / ``load_shards`` do the split and the vocabulary
lookup once per shard instead (``lddl_rows_from_strings``,
csrc/rows_from_strings.hip): the shard's rows become a ``PackResult`` with
spans on the GPU, and ``collate_rows`` / ``collate_rows_unpadded`` /
``RowBatches`` then serve files on disk as they serve a pack result.

``CodeCollate`` is the same surface for the CodeBERT preprocessor's rows (doc /
code / num_tokens, pretrain_codebert.py:425-433), for which the reference has
no loader at all: ``collate_rows`` / ``collate_rows_unpadded`` over a CodeBERT
pack result, ``load_rows`` / ``load_shards`` over CodeBERT shards.

``MlmCollate`` is that surface over the BERT vocabulary for MLM-only rows
(``Packer.pack(..., nsp=False)`` / ``preprocess --no-nsp``: ``[CLS] tokens
[SEP]``, shards of A / num_tokens): no pair, no next_sentence_labels.

Differences from the reference, by design:
* dynamic masking draws from a counter-based hash of (seed, batch counter, row,
  column), not torch's CPU generator: the same distribution (mask rate
  ``mlm_probability``, 80 % [MASK] / 10 % random / 10 % kept), not the same
  stream;
* outputs are CUDA tensors (the reference returns CPU tensors that the
  training loop moves with ``.to(device)``).
"""
import ctypes
import os
import re

import numpy as np
import torch

from . import _lib
from .tokenizer import Tokenizer, _stream

MODE_SPECIAL_MASK, MODE_STATIC, MODE_DYNAMIC = 0, 1, 2


def _column(values, encode):
  """list of str/bytes -> (uint8 bytes, int64 offsets)"""
  enc = [v.encode('utf-8') for v in values] if encode else [bytes(v) for v in values]
  off = np.zeros(len(enc) + 1, dtype=np.int64)
  if enc:
    np.cumsum([len(b) for b in enc], out=off[1:])
  return np.frombuffer(b''.join(enc), dtype=np.uint8), off


def _arrow_column(arr):
  """arrow_cols.var_buffers (pyarrow is imported with the first Arrow input)"""
  from .arrow_cols import var_buffers
  return var_buffers(arr)


def _merge_columns(parts):
  """[(bytes, offsets), ...] of consecutive row ranges -> one (bytes, offsets from 0)"""
  if len(parts) == 1:
    return parts[0]
  data = np.concatenate([d[int(o[0]):int(o[-1])] for d, o in parts])
  off, base = [np.zeros(1, np.int64)], 0
  for _, o in parts:
    off.append(o[1:] - o[0] + base)
    base += int(o[-1] - o[0])
  return data, np.concatenate(off)


def _sample_columns(batch, static):
  """the reference's samples -> ([A, B(, positions, labels)] as (bytes, offsets), is_random_next bytes)"""
  cols = [_column([s[0] for s in batch], True), _column([s[1] for s in batch], True)]
  if static:
    cols += [_column([s[3] for s in batch], False), _column([s[4] for s in batch], True)]
  return cols, np.fromiter((bool(s[2]) for s in batch), dtype=np.uint8, count=len(batch))


def _table_columns(table, static):
  """_sample_columns for a pyarrow RecordBatch / Table of the shard schema"""
  names = ['A', 'B'] + (['masked_lm_positions', 'masked_lm_labels'] if static else [])
  return ([_arrow_column(table.column(k)) for k in names],
          np.asarray(table.column('is_random_next').to_numpy(zero_copy_only=False), dtype=np.uint8))


def _code_shard_columns(table):
  """CodeCollate.load_rows' input -> ([doc, code] as (bytes, offsets), num_tokens uint16)"""
  table = list([table] if hasattr(table, 'schema') else table)
  if not table:
    raise ValueError('no rows')
  for t in table:
    names = t.schema.names if hasattr(t, 'schema') else ()
    if 'doc' not in names or 'code' not in names or 'num_tokens' not in names:
      raise ValueError('not a CodeBERT shard (columns %s): doc, code and num_tokens are needed; BertCollate loads '
                       'BERT shards' % (list(names),))
  parts = [[_arrow_column(t.column(k)) for k in ('doc', 'code')] for t in table]
  cols = [_merge_columns([c[k] for c in parts]) for k in range(2)]
  nt = [np.asarray(t.column('num_tokens').to_numpy(zero_copy_only=False)) for t in table]
  if any(len(x) and (x.min() < 0 or x.max() > 65535) for x in nt):
    raise ValueError('num_tokens outside uint16')
  return cols, np.concatenate(nt).astype(np.uint16)


def _mlm_shard_columns(table):
  """MlmCollate.load_rows' input -> ([empty doc, A] as (bytes, offsets), num_tokens uint16)"""
  table = list([table] if hasattr(table, 'schema') else table)
  if not table:
    raise ValueError('no rows')
  for t in table:
    names = t.schema.names if hasattr(t, 'schema') else ()
    if 'A' not in names or 'num_tokens' not in names or 'B' in names:
      raise ValueError('not an MLM-only shard (columns %s): A and num_tokens without B are needed; BertCollate loads '
                       'BERT shards, CodeCollate CodeBERT shards' % (list(names),))
  a = _merge_columns([_arrow_column(t.column('A')) for t in table])
  nt = [np.asarray(t.column('num_tokens').to_numpy(zero_copy_only=False)) for t in table]
  if any(len(x) and (x.min() < 0 or x.max() > 65535) for x in nt):
    raise ValueError('num_tokens outside uint16')
  nt = np.concatenate(nt).astype(np.uint16)
  return [(np.zeros(0, np.uint8), np.zeros(len(nt) + 1, np.int64)), a], nt


def _shard_columns(table):
  """load_rows' input -> ([A, B(, positions, labels)] as (bytes, offsets), is_random_next bytes, static)"""
  if hasattr(table, 'schema'):
    table = [table]
  table = list(table)
  if not table:
    raise ValueError('no rows')
  if not hasattr(table[0], 'schema'):  # the reference's samples
    static = len(table[0]) > 3
    if any(len(s) != (5 if static else 3) for s in table):
      raise ValueError('samples of 3 fields, or of 5 with static masks')
    return _sample_columns(table, static) + (static,)
  for t in table:
    if 'A' not in t.schema.names or 'B' not in t.schema.names:
      raise ValueError('not a BERT shard (columns %s): CodeBERT shards are loaded by CodeCollate, MLM-only shards '
                       '(A without B) by MlmCollate' % (t.schema.names,))
  static = 'masked_lm_positions' in table[0].schema.names
  for t in table:
    if ('masked_lm_positions' in t.schema.names) != static or (static and 'masked_lm_labels' not in t.schema.names):
      raise ValueError('shards with and without static masks')
  parts = [_table_columns(t, static) for t in table]
  cols = [_merge_columns([c[k] for c, _ in parts]) for k in range(4 if static else 2)]
  return cols, np.concatenate([rn for _, rn in parts]), static


def _check(rc):
  """_lib.check with LDDL_EINDEX (-7) as the IndexError the reference raises for a position out of range"""
  if rc == -7:
    raise IndexError(_lib.lib().lddl_last_error().decode())
  _lib.check(rc)


def _ptr(t):
  """a tensor's (None: NULL) or a device address's void pointer"""
  return ctypes.c_void_p(0 if t is None else t if isinstance(t, int) else t.data_ptr())


_SHARD_NAME = re.compile(r'^(?:(?:part\.|shard-)(\d+)(?=\.parquet)|[^/]*?)\.parquet(?:_(\d+))?$')


def shard_files(names):
  """The parquet files among ``names`` as [(name, partition, bin)] in
  (partition, bin) order.  A parquet file ends in ``.parquet`` (bin None) or
  ``.parquet_<b>`` (bin b, the convention of lddl/utils.py:54-75); other names
  are skipped.  The partition is the p of the preprocessor's
  ``part.<p>.parquet[_<b>]`` or the k of the load balancer's
  ``shard-<k>.parquet[_<b>]``; when some file is named otherwise, partitions
  are the ranks of the distinct stems in sorted order instead.  The bins found
  must be 0 .. nbins - 1 and a directory is binned or unbinned, not both."""
  out, stems = [], []
  for name in names:
    base = os.path.basename(name)
    m = _SHARD_NAME.match(base)
    if not m:
      continue
    out.append([name, None if m.group(1) is None else int(m.group(1)), None if m.group(2) is None else int(m.group(2))])
    stems.append(base[:base.rindex('.parquet')])
  if any(f[1] is None for f in out) or len({s.split('.')[0].split('-')[0] for s in stems}) > 1:
    rank = {s: i for i, s in enumerate(sorted(set(stems)))}
    for f, s in zip(out, stems):
      f[1] = rank[s]
  found = sorted(set(f[2] for f in out if f[2] is not None))
  if found != list(range(len(found))):
    raise ValueError('the bin suffixes %s are not 0 .. %d' % (found, len(found) - 1))
  if found and any(f[2] is None for f in out):
    raise ValueError('binned and unbinned files together')
  return sorted((tuple(f) for f in out), key=lambda f: (f[1], -1 if f[2] is None else f[2], f[0]))


def _check_rank(rank, world_size):
  rank, world_size = int(rank), int(world_size)
  if world_size < 1 or not 0 <= rank < world_size:
    raise ValueError('rank %d outside a world of %d' % (rank, world_size))
  return rank, world_size


def rank_shard_files(files, rank, world_size):
  """The entries of ``files`` (shard_files' output) that rank ``rank`` of
  ``world_size`` reads, in the same order: whole partitions dealt round-robin,
  the partition at position i of the sorted distinct partitions to rank
  i % world_size with all its bin files, as the reference's
  ``files[rank::world_size]`` (lddl/torch/datasets.py:167) deals balanced
  shards.  The partition count must be a multiple of world_size
  (datasets.py:143), so that every rank holds as many shards as any other."""
  rank, world_size = _check_rank(rank, world_size)
  parts = sorted({f[1] for f in files})
  if len(parts) % world_size:
    raise ValueError('%d partitions are not a multiple of world_size %d: balance to a multiple of it (--num-shards)'
                     % (len(parts), world_size))
  mine = set(parts[rank::world_size])
  return [f for f in files if f[1] in mine]


def rank_seed(base_seed, rank):
  """A ``base_seed`` for rank ``rank``'s collate: the dynamic draw is keyed by
  (seed, batch counter, batch row, column), so ranks that share a seed would
  mask the same positions of their batches.  The splitmix64 output function
  over base_seed + (rank + 1) * 0x9E3779B97F4A7C15, a 64-bit int."""
  m = (1 << 64) - 1
  z = (int(base_seed) + (int(rank) + 1) * 0x9E3779B97F4A7C15) & m
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
  return z ^ (z >> 31)


def load_shards(collate, path_or_paths, rank=None, world_size=None):
  """Every ``*.parquet`` / ``*.parquet_<b>`` file under a directory (or the
  files of a list) as one GPU row table: read with pyarrow in (partition, bin)
  order (shard_files), each row's bin from its file's suffix and its partition
  from ``part.<p>`` (the preprocessor's sink) or ``shard-<k>`` (the load
  balancer's output), then one ``collate.load_rows``.  The collate decides
  what is read: a BertCollate takes BERT shards (A / B / is_random_next and the
  static columns), a CodeCollate CodeBERT shards (doc / code / num_tokens; the
  id column is not loaded).  Shards of the other kind raise ValueError.

  rank / world_size (both or neither): only the files of rank_shard_files are
  read, so a rank of a data-parallel job holds its own partitions and no
  others.  The table keeps each row's original partition number in ``part``
  and the bin count of the whole directory."""
  import pyarrow.parquet as pq
  if (rank is None) != (world_size is None):
    raise ValueError('give rank and world_size together')
  if isinstance(path_or_paths, (str, bytes, os.PathLike)):
    path = os.fspath(path_or_paths)
    if os.path.isdir(path):
      names = [os.path.join(r, f) for r, _, fs in os.walk(path) for f in fs]
    else:
      names = [path]
  else:
    names = [os.fspath(x) for x in path_or_paths]
  files = shard_files(names)
  if not files:
    raise ValueError('no parquet files in %r' % (path_or_paths,))
  binned = files[0][2] is not None
  nbins = max(b for _, _, b in files) + 1 if binned else None
  if rank is not None:
    files = rank_shard_files(files, rank, world_size)
  tables, bins, part = [], [], []
  for name, pt, b in files:
    t = pq.read_table(name)
    if any(k not in t.schema.names for k in collate.SHARD_COLUMNS):
      raise ValueError('%s is not a %s shard (columns %s): %s' % (name, collate.SHARD_KIND, t.schema.names,
                                                                 collate.OTHER_SHARDS))
    if t.num_rows == 0:
      continue  # every bin is written, even when empty
    tables.append(t)
    bins.append(np.full(t.num_rows, b or 0, np.uint8))
    part.append(np.full(t.num_rows, pt, np.int64))
  if not tables:
    whose = '' if rank is None else ' for rank %d of %d' % (rank, world_size)
    raise ValueError('no rows in %r%s' % (path_or_paths, whose))
  return collate.load_rows(tables, np.concatenate(bins) if binned else None, np.concatenate(part), nbins)


def _span_args(span_mask):
  """``span_mask=`` of the collates -> (max_span, geo_p), or None when off"""
  if span_mask is None or span_mask is False:
    return None
  if span_mask is True:
    return 10, 0.2
  try:
    if isinstance(span_mask, dict):
      extra = set(span_mask) - {'max_span', 'geo_p'}
      if extra:
        raise ValueError('unknown keys %s' % sorted(extra))
      L, g = span_mask.get('max_span', 10), span_mask.get('geo_p', 0.2)
    else:
      L, g = span_mask
    if isinstance(L, bool) or int(L) != L or not 1 <= int(L) <= 16 or not 0.0 < float(g) <= 1.0:
      raise ValueError('max_span is an int in [1, 16], geo_p in (0, 1]')
  except (TypeError, ValueError) as e:
    raise ValueError('span_mask %r: None / False, True (max_span 10, geo_p 0.2), a (max_span, geo_p) pair or a dict '
                     'of the two (%s)' % (span_mask, e)) from None
  return int(L), float(g)


class _RowCollate:
  """What BertCollate and CodeCollate share: the constructor, the staging of
  string columns, the collate of row-table batches (padded and padding-free),
  the making of a row table and ``mask_tokens``.  CODE says which kind of row
  the C calls are for, KIND the PackResult.kind of the tables it loads."""
  CODE = False
  KIND = 'bert'
  VOCAB = _lib.VOCAB_BERT

  def __init__(self, vocab_file=None, device=None, sequence_length_alignment=8, ignore_index=-1,
               mlm_probability=0.15, base_seed=12345, tokenizer=None, whole_word_mask=False, compact_mlm=False,
               span_mask=None):
    """whole_word_mask: dynamic masking (mode 2 and ``mask_tokens``) selects
    words, not tokens: a piece and the ``##`` pieces after it are masked
    together (lddl_set_whole_word_mask; include/lddl_amd.h defines it).  The
    switch lives on the tokenizer's ctx and is set here, on or off: with
    ``tokenizer=`` a shared ctx, every collate over that ctx follows the one
    constructed last.

    span_mask: dynamic masking selects contiguous runs of whole words inside
    one segment (ALBERT's n-gram masking, SpanBERT's span masking): True for
    ``max_span=10, geo_p=0.2``, or a ``(max_span, geo_p)`` pair or dict; None
    or False: off (lddl_set_span_mask; include/lddl_amd.h defines it).  Span
    lengths follow SpanBERT's clipped geometric law, and spans start so often
    that a word is covered with ``mlm_probability``; the 80/10/10 replacement
    stays per token.  Set on the ctx as ``whole_word_mask`` is, on or off, with
    the same rule for a shared ctx; not to be combined with
    ``whole_word_mask=True`` (``max_span=1`` is whole-word masking).

    compact_mlm: every batch with ``labels`` (modes 1 and 2) also carries the
    compact targets of ``mlm_targets`` over those labels, as
    ``masked_lm_positions``, ``masked_lm_labels`` and ``masked_lm_offsets``:
    True for exact-size tensors, an int K for tensors of exactly K entries
    (a batch with more masked tokens raises).  ``ignore_index`` must then be
    negative.  Everything else in the batch, and the batch counter, are as
    without it."""
    assert isinstance(sequence_length_alignment, int) and sequence_length_alignment >= 1
    assert isinstance(mlm_probability, (int, float)) and 0 <= mlm_probability <= 1
    if not isinstance(compact_mlm, bool):
      if not isinstance(compact_mlm, int) or compact_mlm < 0:
        raise ValueError('compact_mlm %r: False, True or a capacity >= 0' % (compact_mlm,))
    if compact_mlm is not False and int(ignore_index) >= 0:  # (before the ctx is made: nothing here needs a GPU)
      raise ValueError('compact_mlm needs a negative ignore_index: %d could be a label' % int(ignore_index))
    self.span_mask = _span_args(span_mask)
    if self.span_mask and whole_word_mask:
      raise ValueError('span_mask and whole_word_mask=True: one selection at a time (spans are made of whole words)')
    self.compact_mlm = compact_mlm
    self.tok = tokenizer if tokenizer is not None else Tokenizer(vocab_file or self.VOCAB, device)
    self.whole_word_mask = bool(whole_word_mask)
    L = _lib.lib()
    if self.whole_word_mask or hasattr(L, 'lddl_set_whole_word_mask'):  # (an A/B library of an older revision lacks it)
      _lib.check(L.lddl_set_whole_word_mask(self.tok.handle, 1 if self.whole_word_mask else 0))
    if self.span_mask or hasattr(L, 'lddl_set_span_mask'):
      _lib.check(L.lddl_set_span_mask(self.tok.handle, *(self.span_mask or (0, 0.0))))
    self.device = self.tok.device
    self.sequence_length_alignment = sequence_length_alignment
    self.ignore_index = int(ignore_index)
    self.mlm_probability = float(mlm_probability)
    self.seed = int(base_seed) & ((1 << 64) - 1)
    self.counter = 0  # one per collated batch: the dynamic masks differ per batch

  # ---- staging ------------------------------------------------------------
  def _upload(self, cols, per_row):
    """One pinned host buffer holding every column and the per-row array
    (is_random_next bytes, or num_tokens) as 16-B aligned pieces, one H2D
    copy; returns device addresses of each piece."""
    pieces = []
    for data, off in cols:
      pieces.append(data)
      pieces.append(off.view(np.uint8))
    pieces.append(np.ascontiguousarray(per_row).view(np.uint8))
    starts, pos = [], 0
    for p in pieces:
      starts.append(pos)
      pos += (p.nbytes + 15) & ~15
    host = torch.empty(max(pos, 16), dtype=torch.uint8, pin_memory=True)
    hn = host.numpy()
    for p, s in zip(pieces, starts):
      hn[s:s + p.nbytes] = p
    dev = torch.empty_like(host, device=self.device)
    dev.copy_(host, non_blocking=True)
    base = dev.data_ptr()
    return dev, host, [base + s for s in starts]

  def _row_batch(self, who, res, rows, row0, n_rows, mode):
    """what collate_rows / collate_rows_unpadded (who) take -> (mode, rows, row0, n)"""
    if res.kind == 'mlm' and not self.CODE:
      raise ValueError('%s: MLM-only rows (nsp=False) have no pair and no NSP label: MlmCollate collates them' % who)
    if not res.spans:
      raise ValueError('%s needs a PackResult with spans (Packer.pack(..., spans=True))' % who)
    if mode is None:
      mode = MODE_STATIC if res.mlm_token is not None and not self.CODE else MODE_DYNAMIC
    if mode not in (MODE_SPECIAL_MASK, MODE_STATIC, MODE_DYNAMIC):
      raise ValueError('mode %r not in 0..2' % (mode,))
    if mode == MODE_STATIC and self.CODE:
      raise ValueError('CodeBERT rows have no static masks: mode 0 or 2')
    if mode == MODE_STATIC and res.mlm_token is None:
      raise ValueError('static mode needs a result packed with masking=True')
    if rows is not None:
      rows = torch.as_tensor(rows, dtype=torch.int64, device=self.device).contiguous().view(-1)
      n, row0 = rows.numel(), 0
    else:
      row0 = int(row0)
      n = res.n_pairs - row0 if n_rows is None else int(n_rows)
    if n <= 0:
      raise ValueError('empty batch')  # max() of an empty sequence in bert.py:94-95
    return mode, rows, row0, n

  def _collate(self, unpadded, res, rows, row0, n_rows, mode, fixed=None):
    """collate_rows (unpadded False), collate_rows_unpadded and
    collate_rows_fixed (unpadded True with fixed = (max_tokens, max_seqs,
    max_seqlen)) of both classes: the length call (lddl_collate[_code]_rows_seq_len
    / _cu_seqlens) and the outputs it sizes, or the outputs of the given
    capacities; the fill call, the batch counter and the dict."""
    who = 'collate_rows_fixed' if fixed else 'collate_rows_unpadded' if unpadded else 'collate_rows'
    mode, rows, row0, n = self._row_batch(who, res, rows, row0, n_rows, mode)
    L, st, p, h = _lib.lib(), _stream(), _ptr, self.tok.handle
    name = 'lddl_collate_code_rows' if self.CODE else 'lddl_collate_rows'
    lens = (p(res.len0), p(res.len1)) + ((p(res.flags),) if self.CODE else ())
    pick = (p(rows), row0, n, res.n_pairs)
    n_slots, end = n, ()
    if fixed:
      T, n_slots, S = (int(x) for x in fixed)
      if T < 1 or n_slots < 1 or S < 1:
        raise ValueError('%s: max_tokens %d, max_seqs %d, max_seqlen %d: each is 1 at least' % (who, T, n_slots, S))
      cu = torch.empty(n_slots + 1, dtype=torch.int32, device=self.device)
      status = torch.empty(4, dtype=torch.int32, device=self.device)
      counts = [ctypes.c_int64() for _ in range(3)]  # tokens, rows, sequences
      out = torch.empty((4, T), dtype=torch.int64, device=self.device)
      shape = (p(cu), T, n_slots, S)
      end = (p(status),) + tuple(ctypes.byref(x) for x in counts)
    elif unpadded:
      cu = torch.empty(n + 1, dtype=torch.int32, device=self.device)
      total, longest = ctypes.c_int64(), ctypes.c_int64()
      _check(getattr(L, name + '_cu_seqlens')(h, *lens, *pick, p(cu), ctypes.byref(total), ctypes.byref(longest), st))
      T = int(total.value)
      out = torch.empty((4, T), dtype=torch.int64, device=self.device)
      shape = (p(cu), T)
    else:
      seq = ctypes.c_int64()
      _check(getattr(L, name + '_seq_len')(h, *lens, *pick, self.sequence_length_alignment, ctypes.byref(seq), st))
      S = int(seq.value)
      out = torch.empty((4, n, S), dtype=torch.int64, device=self.device)
      shape = (S,)
    table = (p(res.ids), p(res.src0), p(res.src1), p(res.len0), p(res.len1), p(res.flags))
    draw = (mode, self.ignore_index, self.mlm_probability, self.seed, self.counter)
    outs = tuple(p(out[k]) for k in range(4))
    if self.CODE:
      nsl, mlm, tail = None, (), ()
    else:
      nsl = torch.empty(n_slots, dtype=torch.int64, device=self.device)
      mlm = (res.mlm_off, res.mlm_pos, res.mlm_label, res.mlm_token) if mode == MODE_STATIC else (None,) * 4
      mlm, tail = tuple(p(x) for x in mlm), (p(nsl),)
    call = getattr(L, name + ('_fixed' if fixed else '_unpadded' if unpadded else ''))
    rc = call(h, *table, *pick, *mlm, *shape, *draw, *outs, *tail, *end, st)
    if mode != MODE_SPECIAL_MASK:
      self.counter += 1
    _check(rc)
    batch = {'input_ids': out[0], 'token_type_ids': out[1], 'position_ids' if unpadded else 'attention_mask': out[2],
             'special_tokens_mask' if mode == MODE_SPECIAL_MASK else 'labels': out[3]}
    if nsl is not None:
      batch['next_sentence_labels'] = nsl
    if fixed:
      batch['cu_seqlens'], batch['max_seqlen'], batch['status'] = cu, S, status
      batch['num_tokens'], batch['num_rows'], batch['num_seqs'] = (int(x.value) for x in counts)
    elif unpadded:
      batch['cu_seqlens'], batch['max_seqlen'] = cu, int(longest.value)
    return self._with_targets(batch, cu if unpadded else None)

  def _load_table(self, cols, per_row, static, bins, part, nbins):
    """load_rows of both classes over staged columns: the length call, the
    table it sizes, the fill call and the PackResult.  per_row: is_random_next
    bytes, or (CodeCollate) num_tokens."""
    from .pipeline import PackResult
    n = len(per_row)
    if n == 0:
      raise ValueError('no rows')
    L, st, p, h = _lib.lib(), _stream(), _ptr, self.tok.handle
    dev, host, ptrs = self._upload(cols, per_row)
    if self.CODE:
      inp = [p(x) for x in ptrs[:4]] + [p(ptrs[-1])]
    else:
      inp = [p(x) for x in ptrs[:8]] if static else [p(x) for x in ptrs[:4]] + [p(None)] * 4

    def buf(m, dtype):
      return torch.empty(max(m, 1), dtype=dtype, device=self.device)
    len0, len1 = buf(n, torch.int16), buf(n, torch.int16)
    src0, src1 = buf(n, torch.int64), buf(n, torch.int64)
    tok_off = buf(n + 1, torch.int64)
    mlm_off = buf(n + 1, torch.int64) if static else None
    tot = (ctypes.c_int64 * 3)()
    spans = (p(len0), p(len1), p(src0), p(src1))
    try:
      if self.CODE:
        _check(L.lddl_code_rows_from_strings_len(h, *inp, n, *spans, p(tok_off), tot, st))
      else:
        _check(L.lddl_rows_from_strings_len(h, *inp, n, *spans, p(tok_off), p(mlm_off), tot, st))
    except Exception:
      torch.cuda.current_stream().synchronize()  # a call refused before its launch leaves the staging copy queued
      raise
    n_ids, n_masked, n_tokens = (int(tot[0]), 0, int(tot[1])) if self.CODE else (int(tot[0]), int(tot[1]), int(tot[2]))
    ids = torch.empty(n_ids + 16, dtype=torch.int16, device=self.device)  # 16 zeroed entries behind the last id
    ids[n_ids:].zero_()
    flags = buf(n, torch.uint8)
    mlm = [buf(n_masked, torch.int16) for _ in range(3)] if static else [None] * 3
    if self.CODE:
      _check(L.lddl_code_rows_from_strings(h, *inp, n, *spans, p(ids), n_ids, p(flags), st))
    else:
      _check(L.lddl_rows_from_strings(h, *inp, p(ptrs[-1]), n, *spans, p(mlm_off), p(ids), n_ids, p(flags), p(mlm[0]),
                                      p(mlm[1]), p(mlm[2]), n_masked, st))
    del dev, host  # the length call synchronised the stream behind the staging copy
    part_h = np.zeros(n, np.int64) if part is None else np.ascontiguousarray(part, dtype=np.int64).reshape(-1)
    bins_h = np.zeros(n, np.uint8) if bins is None else np.ascontiguousarray(bins, dtype=np.uint8).reshape(-1)
    if len(part_h) != n or len(bins_h) != n:
      raise ValueError('bins / part: one entry per row')
    if bins is None:
      nbins = 1
    elif nbins is None:
      nbins = int(bins_h.max()) + 1
    if int(bins_h.max()) >= nbins:
      raise ValueError('a bin id >= nbins %d' % nbins)
    n_part = int(part_h.max()) + 1
    bin_count = np.bincount(part_h * nbins + bins_h, minlength=n_part * nbins).reshape(n_part, nbins).astype(np.int64)
    h2d = lambda a: torch.from_numpy(a).to(self.device)  # noqa: E731
    res = PackResult(n, n_tokens, int(nbins), None, tok_off, len0, len1, flags, h2d(bins_h), h2d(part_h),
                     h2d(bin_count))
    res.ids, res.src0, res.src1 = ids, src0, src1
    res.cls_id, res.sep_id = self.tok.cls_id, self.tok.sep_id
    res.kind = self.KIND
    if static:
      res.n_masked = n_masked
      res.mlm_off, res.mlm_pos, res.mlm_label, res.mlm_token = mlm_off, mlm[0], mlm[1], mlm[2]
    return res

  def mask_tokens(self, inputs, special_tokens_mask, counter=None):
    """bert.py:156-196 on device tensors: masks ``inputs`` in place and
    returns (inputs, labels).  counter: the batch counter of the draws
    (default: the next one)."""
    assert inputs.dtype == torch.int64 and inputs.is_cuda and inputs.is_contiguous()
    sp = special_tokens_mask.to(device=self.device, dtype=torch.int64).contiguous()
    assert sp.shape == inputs.shape
    labels = torch.empty_like(inputs)
    n, S = inputs.shape
    if counter is None:
      counter = self.counter
      self.counter += 1
    _lib.check(_lib.lib().lddl_mask_tokens(self.tok.handle, ctypes.c_void_p(inputs.data_ptr()),
                                           ctypes.c_void_p(sp.data_ptr()), ctypes.c_void_p(labels.data_ptr()), n,
                                           S, self.mlm_probability, self.ignore_index, self.seed, counter,
                                           _stream()))
    return inputs, labels

  def mlm_targets(self, labels, cu_seqlens=None, capacity=None):
    """The masked positions of a batch and their labels, in order
    (lddl_mlm_targets; include/lddl_amd.h defines it): what a trainer gathers
    the hidden states at before the LM head.  labels: int64 CUDA, ``[n, S]``
    of a padded batch, or ``[T]`` with the int32 ``cu_seqlens`` ``[n + 1]`` of
    a padding-free one -- the ``labels`` of any collate here or of
    ``mask_tokens``.  Returns (positions, target_labels, offsets): the
    ascending flat indices into ``labels.view(-1)`` that lie in a row and
    differ from ``ignore_index``, the labels there (both int64), and int32
    ``[n + 1]`` offsets of each row's share, ``offsets[n]`` = their number M.
    capacity None: tensors of M entries (views of ``labels.numel()``
    allocated).  capacity K: tensors of exactly K entries, (0, ignore_index)
    behind the first M: fixed shapes, harmless to a loss that honours
    ``ignore_index``; M > K raises."""
    assert labels.dtype == torch.int64 and labels.is_cuda and labels.is_contiguous()
    if cu_seqlens is None:
      assert labels.dim() == 2
      n, S = labels.shape
    else:
      assert labels.dim() == 1 and cu_seqlens.dtype == torch.int32 and cu_seqlens.is_cuda and cu_seqlens.is_contiguous()
      n, S = cu_seqlens.numel() - 1, 0
    total = labels.numel()
    cap = total if capacity is None else int(capacity)
    pos = torch.empty(max(cap, 1), dtype=torch.int64, device=labels.device)
    lab = torch.empty(max(cap, 1), dtype=torch.int64, device=labels.device)
    off = torch.empty(max(n, 0) + 1, dtype=torch.int32, device=labels.device)
    count = ctypes.c_int64()
    _check(_lib.lib().lddl_mlm_targets(self.tok.handle, _ptr(labels), n, S, _ptr(cu_seqlens), total, self.ignore_index,
                                       cap, _ptr(pos), _ptr(lab), _ptr(off), ctypes.byref(count), _stream()))
    m = int(count.value) if capacity is None else cap
    return pos[:m], lab[:m], off

  def _with_targets(self, batch, cu_seqlens=None):
    """the batch of a collate, with the compact targets of its labels when compact_mlm asks for them"""
    if self.compact_mlm is not False and 'labels' in batch:
      capacity = None if self.compact_mlm is True else self.compact_mlm
      pos, lab, off = self.mlm_targets(batch['labels'], cu_seqlens, capacity)
      batch['masked_lm_positions'], batch['masked_lm_labels'], batch['masked_lm_offsets'] = pos, lab, off
    return batch


class BertCollate(_RowCollate):
  """``collate(batch) -> dict`` with the keys of bert.py:129-152 plus
  ``labels`` (masked): input_ids, token_type_ids, attention_mask, labels,
  next_sentence_labels -- int64 tensors on the GPU.  With ``compact_mlm``
  also masked_lm_positions, masked_lm_labels and masked_lm_offsets
  (``mlm_targets`` over those labels), here and in every ``collate_rows*``.

  batch: a list of samples as the reference's DataLoader hands to its
  collate_fn (tuples of 3 or 5 fields), or a pyarrow RecordBatch / Table of
  the shard schema (zero-copy columns; ``collate_arrow``)."""
  SHARD_COLUMNS, SHARD_KIND = ('A', 'B'), 'BERT'
  OTHER_SHARDS = 'CodeBERT shards are loaded by CodeCollate, MLM-only shards (A without B) by MlmCollate'

  def _run(self, cols, is_random_next, static, mode=None):
    """lddl_collate_seq_len + lddl_collate_bert over staged columns.  mode None:
    static or dynamic masking, and the batch counter advances; mode 0 (the
    special_tokens_mask in place of labels) leaves it."""
    L = _lib.lib()
    n = len(is_random_next)
    if n == 0:
      raise ValueError('empty batch')  # max() of an empty sequence in bert.py:94-95
    dev, host, ptrs = self._upload(cols, is_random_next)
    st = _stream()
    ab = [_ptr(x) for x in ptrs[:4]]
    seq = ctypes.c_int64()
    _check(L.lddl_collate_seq_len(self.tok.handle, *ab, n, self.sequence_length_alignment, ctypes.byref(seq), st))
    S = int(seq.value)
    out = torch.empty((4, n, S), dtype=torch.int64, device=self.device)
    nsl = torch.empty(n, dtype=torch.int64, device=self.device)
    advance = mode is None
    if advance:
      mode = MODE_STATIC if static else MODE_DYNAMIC
    masks = [_ptr(x) for x in ptrs[4:8]] if mode == MODE_STATIC else [_ptr(None)] * 4
    rc = L.lddl_collate_bert(self.tok.handle, *ab, _ptr(ptrs[-1]), *masks, n, S, mode, self.ignore_index,
                             self.mlm_probability, self.seed, self.counter, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                             _ptr(out[3]), _ptr(nsl), st)
    if advance:
      self.counter += 1
    _check(rc)
    del dev, host  # the stream was synchronised by the call
    return self._with_targets({'input_ids': out[0], 'token_type_ids': out[1], 'attention_mask': out[2],
                               'next_sentence_labels': nsl,
                               'special_tokens_mask' if mode == MODE_SPECIAL_MASK else 'labels': out[3]})

  # ---- entry points ---------------------------------------------------------
  def __call__(self, batch):
    if hasattr(batch, 'schema'):
      return self.collate_arrow(batch)
    static = len(batch[0]) > 3
    if static:
      assert len(batch[0]) == 5
    return self._run(*_sample_columns(batch, static), static)

  def collate_arrow(self, table):
    """A pyarrow RecordBatch/Table with the shard schema (pretrain.py:457-471)."""
    static = 'masked_lm_positions' in table.schema.names
    if static:
      assert 'masked_lm_labels' in table.schema.names
    return self._run(*_table_columns(table, static), static)

  def collate_rows(self, res, rows=None, row0=0, n_rows=None, mode=None):
    """A batch straight from a pack result on the GPU (lddl_collate_rows):
    the rows ``rows`` (an int64 CUDA tensor, or anything torch.as_tensor
    takes; any order, repeats allowed) of ``res``, a PackResult with spans
    (``Packer.pack(..., spans=True)``) -- or rows [row0, row0 + n_rows)
    (default: all from row0 on).  Returns the dict of ``__call__`` (mode 0:
    'special_tokens_mask' in place of 'labels', as ``to_encoded_inputs``) and
    advances the batch counter as ``__call__`` does.  mode defaults to static
    when the result carries static masks, else dynamic.  Nothing is staged on
    the host: the kernel reads the packer's own buffers.  ``res`` must have
    been packed with this collate's vocab, on its device; a CodeBERT result
    (rows without the [SEP] after segment 0) is refused by the C call."""
    return self._collate(False, res, rows, row0, n_rows, mode)

  def collate_rows_unpadded(self, res, rows=None, row0=0, n_rows=None, mode=None):
    """The batch of ``collate_rows`` without its padding
    (lddl_collate_rows_cu_seqlens + lddl_collate_rows_unpadded), for a model
    with variable-length attention: the rows concatenated into one stream of
    T tokens, row r at [cu_seqlens[r], cu_seqlens[r + 1]).  Arguments and mode
    defaults as ``collate_rows``.  Returns input_ids, token_type_ids,
    position_ids and labels (mode 0: special_tokens_mask) as int64 [T],
    next_sentence_labels as int64 [n], cu_seqlens as int32 [n + 1] and
    max_seqlen as a Python int; there is no attention_mask.  The reference
    has no such output: it is ``collate_rows`` at the same seed and counter
    with the pad columns dropped, bit for bit.  The batch counter advances as
    in ``collate_rows``.  ``sequence_length_alignment`` has no effect here:
    nothing is padded."""
    return self._collate(True, res, rows, row0, n_rows, mode)

  def collate_rows_fixed(self, res, rows=None, row0=0, n_rows=None, mode=None, *, max_tokens, max_seqs, max_seqlen):
    """The batch of ``collate_rows_unpadded`` in tensors whose shapes do not
    depend on the batch (lddl_collate_rows_fixed: offsets and fill in one call,
    one launch, one synchronise), for a step that is captured or compiled
    once: input_ids, token_type_ids, position_ids and labels (mode 0:
    special_tokens_mask) as int64 [max_tokens], cu_seqlens as int32
    [max_seqs + 1], next_sentence_labels as int64 [max_seqs], and max_seqlen,
    the argument.  With n rows of ``total`` tokens, [0, total),
    cu_seqlens[0..n] and next_sentence_labels[0..n) are
    ``collate_rows_unpadded`` at the same seed and counter, bit for bit.  The
    slack [total, max_tokens) is cut into p = ceil(slack / max_seqlen) pad
    sequences in slots n .. n + p - 1, so that every token lies in a sequence:
    input_ids 0, token_type_ids 0, position_ids restarting at 0 in each,
    labels ignore_index (special_tokens_mask 1).  The remaining slots are
    empty, cu_seqlens = max_tokens; next_sentence_labels is ignore_index from
    slot n on.  Also returned: num_tokens (total), num_rows (n) and num_seqs
    (n + p) as Python ints, and ``status``, an int32 [4] device tensor
    {total, n, n + p, max_seqlen} for a trainer that reads them without the
    host.  More than max_tokens tokens, a row longer than max_seqlen, or
    n + p > max_seqs raise; ``fixed_seq_cap`` gives a max_seqs that the
    batches of ``RowBatches(res, max_tokens=, max_rows=)`` never exceed.  The
    batch counter advances as in ``collate_rows_unpadded``; with
    ``compact_mlm`` the targets are those of the real rows (pad sequences
    have none) and masked_lm_offsets is [max_seqs + 1]: ``compact_mlm=K``
    makes every tensor of the step fixed-shape."""
    return self._collate(True, res, rows, row0, n_rows, mode, (max_tokens, max_seqs, max_seqlen))

  def load_rows(self, table, bins=None, part=None, nbins=None):
    """The rows of a shard as a GPU row table, once (lddl_rows_from_strings_len
    + lddl_rows_from_strings): the decode-and-lookup half of the reference's
    loader (bert.py:42-60, :83-89, :109-124) done per shard instead of per
    batch.  Returns a ``pipeline.PackResult`` with spans, so ``collate_rows``,
    ``collate_rows_unpadded``, ``RowBatches``, ``rows()`` and
    ``host_tokens()`` serve files on disk as they serve a pack result.

    table: a pyarrow Table / RecordBatch of the shard schema (string or
    large_string columns), a list of such tables, or a list of the reference's
    3- or 5-tuples.  Shards with masked_lm_positions / masked_lm_labels give a
    result with static masks.  bins / part: the bin and the partition of every
    row (default zeros); without bins the result is unbinned (nbins 1), with
    them nbins defaults to max(bins) + 1.  The columns are staged in one pinned
    buffer and copied once; the staging is released when the call returns.
    Fields that only a pack has stay None: tokens, ntok, ids_off, pack."""
    cols, rn, static = _shard_columns(table)
    return self._load_table(cols, rn, static, bins, part, nbins)

  # ---- the reference's two steps, separately ----------------------------------
  def to_encoded_inputs(self, batch):
    """bert.py:69-153 as is: with static masks 'labels', else
    'special_tokens_mask' (dynamic masking left to mask_tokens)."""
    if len(batch[0]) > 3:
      return self(batch)
    return self._run(*_sample_columns(batch, False), False, mode=MODE_SPECIAL_MASK)


class CodeCollate(_RowCollate):
  """The loader of CodeBERT rows (pretrain_codebert.py:425-433: doc, code,
  num_tokens), which the reference lacks: same constructor as BertCollate (the
  CodeBERT vocabulary by default), batches from a CodeBERT pack result or from
  CodeBERT shards.  A row shows ``[CLS] doc [SEP] code [SEP]`` with
  token_type_ids 1 on code and its [SEP], or, when its document has no
  docstring (flags bit 1 clear), ``[CLS] code [SEP]`` with token_type_ids 0:
  what a BERT tokenizer gives for a pair and for a single sequence.  There is
  no next_sentence_labels and no static masking; mode defaults to dynamic and
  draws as BertCollate does, keyed by (seed, batch counter, row, column)."""
  CODE = True
  KIND = 'codebert'
  VOCAB = _lib.VOCAB_CODEBERT
  SHARD_COLUMNS, SHARD_KIND = ('doc', 'code', 'num_tokens'), 'CodeBERT'
  OTHER_SHARDS = 'BERT shards are loaded by BertCollate'

  def collate_rows(self, res, rows=None, row0=0, n_rows=None, mode=None):
    """A padded batch of CodeBERT rows (lddl_collate_code_rows), picked as in
    ``BertCollate.collate_rows``: input_ids, token_type_ids, attention_mask and
    labels (mode 0: special_tokens_mask, 1 on [CLS], each [SEP] and the
    padding) as int64 [n, S].  mode 2 (the default) is mode 0 followed by
    ``mask_tokens`` at the same seed and counter, bit for bit, and advances
    the batch counter.  On rows that have the first [SEP] the four tensors are
    those of ``BertCollate.collate_rows``."""
    return self._collate(False, res, rows, row0, n_rows, mode)

  def collate_rows_unpadded(self, res, rows=None, row0=0, n_rows=None, mode=None):
    """``collate_rows`` at the same seed and counter with the pad columns
    dropped, bit for bit (lddl_collate_code_rows_cu_seqlens +
    lddl_collate_code_rows_unpadded): input_ids, token_type_ids, position_ids
    and labels (mode 0: special_tokens_mask) as int64 [T], cu_seqlens as int32
    [n + 1] and max_seqlen as a Python int."""
    return self._collate(True, res, rows, row0, n_rows, mode)

  def collate_rows_fixed(self, res, rows=None, row0=0, n_rows=None, mode=None, *, max_tokens, max_seqs, max_seqlen):
    """``collate_rows_unpadded`` in tensors of fixed shape
    (lddl_collate_code_rows_fixed), as ``BertCollate.collate_rows_fixed``
    without next_sentence_labels: the real rows first, bit for bit, then the
    slack as pad sequences of at most max_seqlen tokens, cu_seqlens as int32
    [max_seqs + 1], num_tokens / num_rows / num_seqs and ``status``."""
    return self._collate(True, res, rows, row0, n_rows, mode, (max_tokens, max_seqs, max_seqlen))

  def load_rows(self, table, bins=None, part=None, nbins=None):
    """The rows of a CodeBERT shard as a GPU row table, once
    (lddl_code_rows_from_strings_len + lddl_code_rows_from_strings): a
    ``pipeline.PackResult`` with spans, as ``BertCollate.load_rows`` returns.
    table: a pyarrow Table / RecordBatch with doc, code (string or
    large_string) and num_tokens columns, or a list of such tables; the id
    column is not loaded.  A row's num_tokens says whether a [SEP] follows its
    doc segment (doc + code + 3 tokens) or not (code + 2, with an empty doc);
    any other value is refused.  bins / part / nbins as there."""
    cols, nt = _code_shard_columns(table)
    return self._load_table(cols, nt, False, bins, part, nbins)


class MlmCollate(CodeCollate):
  """The loader of MLM-only rows (``Packer.pack(..., nsp=False)``,
  ``preprocess --no-nsp``): consecutive sentences of one document as
  ``[CLS] tokens [SEP]``, for recipes that train without NSP.  CodeCollate's
  surface over the BERT vocabulary: ``collate_rows`` /
  ``collate_rows_unpadded`` / ``collate_rows_fixed`` over an MLM-only pack
  result, ``load_rows`` /
  ``load_shards`` over MLM-only shards (A, num_tokens), ``whole_word_mask``,
  ``span_mask`` and ``compact_mlm`` as on the other classes.  Batches hold input_ids,
  token_type_ids (all 0), attention_mask (unpadded: position_ids, cu_seqlens,
  max_seqlen) and labels (mode 0: special_tokens_mask); there is no
  next_sentence_labels.  Such a row is a CodeBERT row without docstring, so
  the calls are CodeCollate's (lddl_collate_code_rows*,
  lddl_code_rows_from_strings*)."""
  KIND = 'mlm'
  VOCAB = _lib.VOCAB_BERT
  SHARD_COLUMNS, SHARD_KIND = ('A', 'num_tokens'), 'MLM-only'
  OTHER_SHARDS = 'BERT shards are loaded by BertCollate, CodeBERT shards by CodeCollate'

  def load_rows(self, table, bins=None, part=None, nbins=None):
    """The rows of an MLM-only shard as a GPU row table, once: a pyarrow
    Table / RecordBatch with A (string or large_string) and num_tokens
    columns and no B, or a list of such tables.  A goes to the code segment
    beside an empty doc column; num_tokens must be len(A.split()) + 2.
    bins / part / nbins as ``BertCollate.load_rows``."""
    cols, nt = _mlm_shard_columns(table)
    res = self._load_table(cols, nt, False, bins, part, nbins)
    if bool(res.flags[:res.n_pairs].any()):  # (len + 3: the C call reads a [SEP] after the empty doc segment)
      raise ValueError('an MLM-only row whose num_tokens is not len(A.split()) + 2')
    return res


def plan_row_batches(bins, batch_size, seed=12345, epoch=0, drop_last=False, n_rows=None):
  """The batches of one epoch over binned rows, on the host: a list of int64
  index arrays.  bins: the bin id of every row (None: n_rows rows of one bin).
  Each bin's rows are permuted and cut into batches of batch_size (a bin's
  last short batch is kept unless drop_last; an empty bin gives none), then
  the batch list is permuted; every draw comes from one generator seeded by
  (seed, epoch).  A batch never mixes bins, so its padded length tracks its
  bin (the point of binning, lddl/torch/bert.py's per-bin data loaders)."""
  batch_size = int(batch_size)
  if batch_size < 1:
    raise ValueError('batch_size %d < 1' % batch_size)
  if bins is None:
    bins = np.zeros(int(n_rows), dtype=np.int64)
  bins = np.asarray(bins).reshape(-1)
  rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & ((1 << 64) - 1), int(epoch)])))
  order = np.argsort(bins, kind='stable').astype(np.int64)
  counts = np.bincount(bins.astype(np.int64)) if bins.size else np.zeros(0, np.int64)
  batches, lo = [], 0
  for c in counts:  # ascending bin id; empty bins add nothing
    rows = order[lo:lo + c][rng.permutation(int(c))]
    lo += c
    full = (int(c) // batch_size) * batch_size
    batches.extend(rows[i:i + batch_size] for i in range(0, full, batch_size))
    if full < c and not drop_last:
      batches.append(rows[full:])
  return [batches[i] for i in rng.permutation(len(batches))]


def plan_token_batches(lengths, max_tokens, max_rows=None, seed=12345, epoch=0):
  """The batches of one epoch for a padding-free collate, on the host: a list
  of int64 index arrays.  lengths: the tokens of every row (len0 + len1 + 3; a CodeBERT
  row without docstring has one fewer).
  All rows are permuted by a generator seeded by (seed, epoch), built as in
  plan_row_batches, and the permutation is cut in order: a batch is closed
  when the next row would take it over max_tokens tokens or max_rows rows.
  With no padding a bin means nothing, and what a step holds constant is its
  tokens.  Every row appears once and no batch is empty; a row longer than
  max_tokens raises ValueError."""
  max_tokens = int(max_tokens)
  if max_tokens < 1:
    raise ValueError('max_tokens %d < 1' % max_tokens)
  if max_rows is not None:
    max_rows = int(max_rows)
    if max_rows < 1:
      raise ValueError('max_rows %d < 1' % max_rows)
  lengths = np.asarray(lengths).reshape(-1).astype(np.int64)
  if lengths.size and int(lengths.max()) > max_tokens:
    raise ValueError('row %d has %d tokens, max_tokens %d' % (int(lengths.argmax()), int(lengths.max()), max_tokens))
  rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(seed) & ((1 << 64) - 1), int(epoch)])))
  order = rng.permutation(lengths.size).astype(np.int64)
  # token t of the permuted stream starts its row at csum; a batch that starts at row i ends in front of the first
  # row whose end passes csum[i] + max_tokens
  csum = np.concatenate([np.zeros(1, np.int64), np.cumsum(lengths[order])])
  batches, i, n = [], 0, int(lengths.size)
  while i < n:
    j = int(np.searchsorted(csum, csum[i] + max_tokens, side='right')) - 1
    if max_rows is not None:
      j = min(j, i + max_rows)
    batches.append(order[i:j])
    i = j
  return batches


def _dp_generators(seed, epoch, rank):
  """(world generator, rank generator) of the data-parallel planners: the
  first is seeded by (seed, epoch) as in plan_row_batches and is the same on
  every rank, the second is its SeedSequence child with spawn key (rank,)."""
  entropy = [int(seed) & ((1 << 64) - 1), int(epoch)]
  seqs = (np.random.SeedSequence(entropy), np.random.SeedSequence(entropy, spawn_key=(int(rank),)))
  return tuple(np.random.Generator(np.random.PCG64(s)) for s in seqs)


def plan_row_batches_dp(bins, counts, rank, batch_size, seed=12345, epoch=0, drop_last=False, n_rows=None):
  """plan_row_batches for rank ``rank`` of a data-parallel job: every rank
  gets the same number of batches, and at every step all ranks' batches come
  from the same bin and have the same length, so padded lengths agree and no
  rank runs out first (what the reference gets from one world generator,
  lddl/torch/dataloader.py:32-91, and from equal shards, datasets.py:143-152).
  Returns this rank's batches, int64 index arrays into its own rows.

  bins: the bin id of each of this rank's rows (None: n_rows rows of bin 0).
  counts: int64 [world_size, nbins], the rows every rank holds per bin; row
  ``rank`` must be the counts of ``bins``.  Bin b serves n_b = min over ranks
  of counts[:, b] rows on every rank, in n_b // batch_size batches with
  drop_last, else ceil(n_b / batch_size), the short one last.  The list of
  steps (bin ids) is permuted by a generator seeded by (seed, epoch) alone;
  this rank's rows inside each bin are permuted by one seeded by (seed, epoch,
  rank), and a rank that holds more than n_b rows leaves the tail of that
  permutation out for this epoch: the reference loses the surplus of its
  larger files the same way (datasets.py:147-152), here it is drawn afresh
  every epoch.  The k-th step of a bin takes that bin's k-th batch."""
  batch_size = int(batch_size)
  if batch_size < 1:
    raise ValueError('batch_size %d < 1' % batch_size)
  counts = np.asarray(counts, dtype=np.int64)
  if counts.ndim != 2:
    raise ValueError('counts: [world_size, nbins]')
  rank, _ = _check_rank(rank, counts.shape[0])
  nbins = counts.shape[1]
  if bins is None:
    bins = np.zeros(int(n_rows), dtype=np.int64)
  bins = np.asarray(bins).reshape(-1).astype(np.int64)
  if bins.size and int(bins.max()) >= nbins:
    raise ValueError('a bin id >= the %d bins of counts' % nbins)
  if not np.array_equal(np.bincount(bins, minlength=nbins), counts[rank]):
    raise ValueError('counts[%d] is not the bin count of this rank\'s rows' % rank)
  world_rng, rank_rng = _dp_generators(seed, epoch, rank)
  used = counts.min(axis=0)
  order = np.argsort(bins, kind='stable')
  lo = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts[rank])])
  per_bin, steps = [], []
  for b in range(nbins):  # ascending bin id: every rank draws in the same order
    c, n = int(counts[rank, b]), int(used[b])
    rows = order[lo[b]:lo[b] + c][rank_rng.permutation(c)][:n]
    full = (n // batch_size) * batch_size
    cut = [rows[i:i + batch_size] for i in range(0, full, batch_size)]
    if full < n and not drop_last:
      cut.append(rows[full:])
    per_bin.append(cut)
    steps += [b] * len(cut)
  step_bins = np.asarray(steps, dtype=np.int64)[world_rng.permutation(len(steps))]
  taken = [0] * nbins
  batches = []
  for b in step_bins.tolist():
    batches.append(per_bin[b][taken[b]])
    taken[b] += 1
  return batches


def plan_token_batches_dp(lengths, rank, max_tokens, max_rows=None, seed=12345, epoch=0, steps=None):
  """plan_token_batches for rank ``rank`` of a data-parallel job: this rank's
  rows are permuted by a generator seeded by (seed, epoch, rank), built as in
  plan_row_batches_dp, and plan_token_batches cuts that order.  steps: the
  batches of this epoch, the minimum over ranks of their own plans' lengths
  (RowBatches agrees on it); the plan is cut to its first ``steps`` batches
  and the rows behind them sit this epoch out.  None keeps the whole plan;
  more steps than the plan has raise ValueError."""
  lengths = np.asarray(lengths).reshape(-1).astype(np.int64)
  _, rank_rng = _dp_generators(seed, epoch, rank)
  perm = rank_rng.permutation(lengths.size).astype(np.int64)
  plan = [perm[b] for b in plan_token_batches(lengths[perm], max_tokens, max_rows, seed, epoch)]
  if steps is not None:
    steps = int(steps)
    if not 0 <= steps <= len(plan):
      raise ValueError('steps %d, but rank %d has %d batches' % (steps, int(rank), len(plan)))
    plan = plan[:steps]
  return plan


def fixed_seq_cap(max_tokens, max_rows, max_seqlen):
  """The ``max_seqs`` of ``collate_rows_fixed`` that no batch of
  ``RowBatches(res, max_tokens=max_tokens, max_rows=max_rows)`` can exceed:
  max_rows + ceil(max_tokens / max_seqlen).  A fixed batch takes n slots for
  its rows and p = ceil((max_tokens - total) / max_seqlen) for the pad
  sequences of its slack; the plan gives n <= max_rows, and total >= 0 gives
  p <= ceil(max_tokens / max_seqlen), whatever the batch holds: the short last
  batch of an epoch, which is mostly slack, is covered as well."""
  max_tokens, max_rows, max_seqlen = int(max_tokens), int(max_rows), int(max_seqlen)
  if max_tokens < 1 or max_rows < 1 or max_seqlen < 1:
    raise ValueError('max_tokens %d, max_rows %d, max_seqlen %d: each is 1 at least' % (max_tokens, max_rows, max_seqlen))
  return max_rows + -(-max_tokens // max_seqlen)


class RowBatches:
  """Iterable of int64 row-index tensors (on the result's device), one per
  batch, over a PackResult: ``for idx in RowBatches(res, 256): batch =
  collate.collate_rows(res, idx)``.  The plan is plan_row_batches over a host
  copy of res.bins (an unbinned result is one bin); set_epoch(e) reshuffles.

  With ``max_tokens`` in place of ``batch_size`` (exactly one of the two) the
  batches are for ``collate_rows_unpadded``: plan_token_batches over a host
  copy of len0 + len1 + 2 + ((flags >> 1) & 1), at most max_tokens tokens (and max_rows rows) each;
  bins are ignored and drop_last has no meaning.  For ``collate_rows_fixed``
  give max_rows too: ``fixed_seq_cap(max_tokens, max_rows, max_seqlen)`` is then its max_seqs.

  ``start_step=k`` (here or in ``set_epoch``) resumes in the middle of an
  epoch: iteration skips the first k batches of the plan and ``len()`` still
  reports the whole epoch.  With ``collate.counter = k`` beside it the dynamic
  masks are those of the uninterrupted job.

  With ``rank`` / ``world_size`` (``res`` being that rank's table,
  ``load_shards(..., rank=, world_size=)``) the plans are plan_row_batches_dp
  and plan_token_batches_dp: every rank iterates the same number of batches,
  and the binned ones share their bin and length at every step.  What the
  ranks must agree on comes from ``group`` (None: the default process group):
  the per-bin row counts of every rank, one all_gather_into_tensor of [nbins]
  int64 in the constructor, or the number of token batches, one
  all_reduce(MIN) of one int per epoch's plan.  ``counts`` ([world_size,
  nbins]) or ``steps`` given explicitly take their place, so that one process
  can stand in for every rank; a world of more than one rank with neither and
  no process group raises.  world_size defaults to the group's size.  A
  rank's plan of an epoch is kept until seed or epoch change, so ``len()`` and
  the loop cost one collective together."""

  def __init__(self, res, batch_size=None, seed=12345, epoch=0, drop_last=False, max_tokens=None, max_rows=None,
               rank=None, world_size=None, group=None, counts=None, steps=None, start_step=0):
    if (batch_size is None) == (max_tokens is None):
      raise ValueError('give exactly one of batch_size and max_tokens')
    if max_rows is not None and max_tokens is None:
      raise ValueError('max_rows goes with max_tokens')
    if rank is None and any(x is not None for x in (world_size, group, counts, steps)):
      raise ValueError('world_size, group, counts and steps go with rank')
    if counts is not None and max_tokens is not None:
      raise ValueError('counts goes with batch_size: a token plan agrees on steps')
    if steps is not None and max_tokens is None:
      raise ValueError('steps goes with max_tokens: a binned plan agrees on counts')
    self.rank = self.world_size = self.group = self.counts = self.steps = None
    self._planned = None
    self.start_step = self._start(start_step)
    self.seed, self.epoch, self.drop_last = seed, epoch, drop_last
    self.batch_size = int(batch_size) if batch_size is not None else None
    self.max_tokens = int(max_tokens) if max_tokens is not None else None
    self.max_rows = max_rows
    self.device = res.len0.device
    self.n_rows = res.n_pairs
    self.bins = self.lengths = None
    if self.max_tokens is not None:
      n = res.n_pairs
      l0 = res.len0[:n].cpu().numpy().view(np.uint16).astype(np.int64)  # int16 views of uint16
      l1 = res.len1[:n].cpu().numpy().view(np.uint16).astype(np.int64)
      fl = res.flags[:n].cpu().numpy().astype(np.int64)
      self.lengths = l0 + l1 + 2 + ((fl >> 1) & 1)  # bit 1: the [SEP] after segment 0 (every BERT row has it)
    elif res.nbins > 1:
      self.bins = res.bins[:res.n_pairs].cpu().numpy()
    if rank is not None:
      self._join(res, rank, world_size, group, counts, steps)

  @staticmethod
  def _start(start_step):
    start_step = int(start_step)
    if start_step < 0:
      raise ValueError('start_step %d < 0' % start_step)
    return start_step

  def _collective(self, what):
    """torch.distributed and the device its collectives over self.group take (the GPU under nccl = RCCL)"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
      raise ValueError('rank %d of %d with no process group: init_process_group first, or give %s' %
                       (self.rank, self.world_size, what))
    return dist, self.device if dist.get_backend(self.group) == 'nccl' else torch.device('cpu')

  def _join(self, res, rank, world_size, group, counts, steps):
    """the constructor's data-parallel half: rank and world, and the per-bin counts of every rank for a binned plan"""
    self.group = group
    if world_size is None:
      import torch.distributed as dist
      if not (dist.is_available() and dist.is_initialized()):
        raise ValueError('rank without world_size and no process group to take it from')
      world_size = dist.get_world_size(group)
    self.rank, self.world_size = _check_rank(rank, world_size)
    if self.max_tokens is not None:
      self.steps = None if steps is None else int(steps)
      if self.steps is None and self.world_size > 1:
        self._collective('steps')  # (refuse here, not in the first epoch)
      return
    nbins = int(res.nbins)
    mine = np.bincount(self.bins, minlength=nbins) if self.bins is not None else np.array([self.n_rows])
    mine = mine.astype(np.int64)
    if counts is not None:
      counts = np.array(counts, dtype=np.int64)
      if counts.shape != (self.world_size, nbins):
        raise ValueError('counts of shape %s, not [world_size %d, nbins %d]' % (counts.shape, self.world_size, nbins))
      if not np.array_equal(counts[self.rank], mine):
        raise ValueError('counts[%d] is not the bin count of this rank\'s rows' % self.rank)
    elif self.world_size == 1:
      counts = mine[None]
    else:
      dist, dev = self._collective('counts')
      if dist.get_world_size(group) != self.world_size:
        raise ValueError('world_size %d, but the group has %d ranks' % (self.world_size, dist.get_world_size(group)))
      out = torch.empty(self.world_size * nbins, dtype=torch.int64, device=dev)
      dist.all_gather_into_tensor(out, torch.from_numpy(mine).to(dev), group=group)
      counts = out.cpu().numpy().reshape(self.world_size, nbins)
    self.counts = counts

  def set_epoch(self, epoch, start_step=0):
    self.epoch = epoch
    self.start_step = self._start(start_step)

  def _fewest(self, local):
    """the token batches of this epoch: the fewest any rank has"""
    dist, dev = self._collective('steps')
    n = torch.tensor([local], dtype=torch.int64, device=dev)
    dist.all_reduce(n, op=dist.ReduceOp.MIN, group=self.group)
    return int(n.item())

  def plan(self):
    if self.rank is not None:
      key = (self.seed, self.epoch, self.drop_last, self.batch_size, self.max_tokens, self.max_rows, self.steps)
      if self._planned is None or self._planned[0] != key:
        if self.max_tokens is not None:
          plan = plan_token_batches_dp(self.lengths, self.rank, self.max_tokens, self.max_rows, self.seed, self.epoch,
                                       steps=self.steps)
          if self.steps is None and self.world_size > 1:
            plan = plan[:self._fewest(len(plan))]
        else:
          plan = plan_row_batches_dp(self.bins, self.counts, self.rank, self.batch_size, self.seed, self.epoch,
                                     self.drop_last, n_rows=self.n_rows)
        self._planned = (key, plan)
      return list(self._planned[1])
    if self.max_tokens is not None:
      return plan_token_batches(self.lengths, self.max_tokens, self.max_rows, self.seed, self.epoch)
    return plan_row_batches(self.bins, self.batch_size, self.seed, self.epoch, self.drop_last, n_rows=self.n_rows)

  def __len__(self):
    return len(self.plan())

  def __iter__(self):
    plan = self.plan()[self.start_step:]
    if not plan:
      return
    flat = torch.from_numpy(np.concatenate(plan)).to(self.device)  # the indices only: one copy per epoch
    lo = 0
    for b in plan:
      yield flat[lo:lo + len(b)]
      lo += len(b)
