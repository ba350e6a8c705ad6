"""lddl_render_strings (its four segment modes), lddl_render_masked and
lddl_row_docs (lddl_amd/csrc/render.hip, capi_render.hip, capi_pack.hip) on hand-made row tables.

Every parquet string column goes through render_len_kernel (bytes per row),
the offset scan and render_bytes_kernel; the other tests reach them only
through write_shards over the rows a packer happens to produce.  Here the
inputs are numpy tables and the reference is Python inside this file:

  row r    = b' '.join(vocab[t] for t in segment(r))
  offsets  = the running sum of len(row), from 0

compared exactly (offsets, byte count, bytes).  vocab is the vocabulary file's
lines (Tokenizer.ids_to_tokens); only ids below the vocabulary size occur.

  a  SEG0 / SEG1 / ROW / SPAN over one table whose segments have 0, 1, 2, 63,
     64, 65, 127, 128, 129, 510 and 511 tokens (the 64-token chunk edges of
     the wave loop), spans at odd offsets of a dense id buffer that ends with
     the last span; CodeBERT rows with and without the [SEP] after segment 0
  b  row ranges: offsets restart at 0, n_rows = 0
  c  the size query, LDDL_ECAPACITY one byte short, and a guard of 0xAA past
     the last byte (no joining space after a row's last token), every third
     row rendered alone
  d  more rows than one pass of the grid (and than one block of the scan)
  e  the 'widths' vocabulary: entries of 0..255 bytes, multi-byte endings
  f  static masking: hand-made positions at the chunk edges and segment ends,
     70 and 130 positions in a row, replacements longer / shorter / equal /
     empty, a row range that starts inside the table
  g  a render call as the first call of a new ctx
  h  lddl_row_docs against oracle/pack_oracle.py over documents with empty
     sentences, empty documents and empty partitions
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import synth_vocab as sv
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

SEG0, SEG1, ROW, SPAN = 0, 1, 2, 3
ECAPACITY = -6
LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 510)
MODES = ('seg0', 'seg1', 'row', 'span0', 'span1')
GUARD = 64


# ---- the reference ------------------------------------------------------------
def reference(vocab, segs):
  """(offsets int64[n + 1], bytes) of the string column whose rows are segs"""
  rows = [b' '.join(vocab[t] for t in seg) for seg in segs]
  off = np.zeros(len(rows) + 1, dtype=np.int64)
  off[1:] = np.cumsum(np.fromiter(map(len, rows), dtype=np.int64, count=len(rows)))
  return off, b''.join(rows)


def check(got, vocab, segs):
  off, data = got
  eoff, ebytes = reference(vocab, segs)
  off, data = np.asarray(off), np.asarray(data)
  assert off.dtype == np.int64 and off.shape == eoff.shape, (off.dtype, off.shape, eoff.shape)
  bad = np.nonzero(off != eoff)[0]
  assert bad.size == 0, 'offset %d: %d, expected %d (row %d has %d tokens)' % (
      bad[0], off[bad[0]], eoff[bad[0]], bad[0] - 1, len(segs[max(bad[0] - 1, 0)]))
  assert data.dtype == np.uint8 and data.size == len(ebytes), (data.size, len(ebytes))
  got_b = data.tobytes()
  if got_b != ebytes:
    at = int(np.nonzero(np.frombuffer(got_b, np.uint8) != np.frombuffer(ebytes, np.uint8))[0][0])
    r = int(np.searchsorted(eoff, at, side='right')) - 1
    raise AssertionError('byte %d (row %d, %d tokens, byte %d of its %d): got %r, expected %r' % (
        at, r, len(segs[r]), at - eoff[r], eoff[r + 1] - eoff[r], got_b[at:at + 24], ebytes[at:at + 24]))


# ---- device tables ------------------------------------------------------------
def u16(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def i64(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def u8(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def pair_table(A, B, sep0, rn, cls, sep, fill):
  """rows [CLS] A [SEP]? B [SEP] (the [SEP] after A where sep0) as
  lddl_materialize lays them out (tokens, tok_off, len0, len1, flags) and as
  lddl_row_spans does (src0 / src1 over dense ids): every span starts at an
  odd offset, other ids lie between the spans, the last span ends the buffer"""
  t = types.SimpleNamespace(A=A, B=B, n=len(A))
  t.rows = [[cls] + a + ([sep] if s else []) + b + [sep] for a, b, s in zip(A, B, sep0)]
  t.len0, t.len1 = u16([len(a) for a in A]), u16([len(b) for b in B])
  t.flags = u8([(2 if s else 0) | (1 if r else 0) for s, r in zip(sep0, rn)])
  t.tokens = u16([x for r in t.rows for x in r])
  t.tok_off = i64(np.concatenate([[0], np.cumsum([len(r) for r in t.rows])]))
  dense, src = [], ([], [])
  for a, b in zip(A, B):
    for k, seg in enumerate((a, b)):
      while len(dense) % 2 == 0:
        dense.append(fill())
      src[k].append(len(dense))
      dense += seg
  assert all(x % 2 for x in src[0] + src[1]) and B[-1] and src[1][-1] + len(B[-1]) == len(dense)
  t.ids, t.src0, t.src1 = u16(dense), i64(src[0]), i64(src[1])
  return t


def segs_of(t, mode):
  return {'seg0': t.A, 'span0': t.A, 'seg1': t.B, 'span1': t.B, 'row': t.rows}[mode]


def render_mode(pk, t, mode, row0, n, codebert=False):
  from lddl_amd import writer
  if mode == 'span0':
    return writer.render(pk, t.ids, t.src0, row0, n, SPAN, len0=t.len0)
  if mode == 'span1':
    return writer.render(pk, t.ids, t.src1, row0, n, SPAN, len0=t.len1)
  if mode == 'row':
    return writer.render(pk, t.tokens, t.tok_off, row0, n, ROW)
  # (no flags without codebert: the [SEP] after segment 0 is unconditional there)
  return writer.render(pk, t.tokens, t.tok_off, row0, n, SEG0 if mode == 'seg0' else SEG1, len0=t.len0, len1=t.len1,
                       flags=t.flags if codebert else None, codebert=codebert)


@functools.lru_cache(maxsize=None)
def packer(name):
  from lddl_amd import pipeline
  return pipeline.Packer({'bert': _lib.VOCAB_BERT, 'codebert': _lib.VOCAB_CODEBERT}.get(name) or sv.vocab_path(name), 0)


def vocab_of(pk):
  return [t.encode('utf-8') for t in pk.tok.ids_to_tokens]


def draw(rng, n, hi):
  return [int(x) for x in rng.integers(0, hi, n)]


@functools.lru_cache(maxsize=None)
def bert_table():
  """every (len(A), len(B)) of LENS x LENS in a fixed shuffled order, then the 1024-token row (510, 511)"""
  tok = packer('bert').tok
  rng = np.random.default_rng(11)
  V = tok.vocab_size
  shapes = [(a, b) for a in LENS for b in LENS]
  shapes = [shapes[i] for i in rng.permutation(len(shapes))] + [(510, 511)]
  A = [draw(rng, a, V) for a, _ in shapes]
  B = [draw(rng, b, V) for _, b in shapes]
  t = pair_table(A, B, [True] * len(A), [bool(x) for x in rng.integers(0, 2, len(A))], tok.cls_id, tok.sep_id,
                 lambda: int(rng.integers(0, V)))
  assert len(t.rows[-1]) == 1024
  return t


@functools.lru_cache(maxsize=None)
def codebert_table():
  """[CLS] doc [SEP] code [SEP] (flags bit 1) next to [CLS] code [SEP] (bit 1 clear, len0 = 0); bit 0 is noise"""
  tok = packer('codebert').tok
  rng = np.random.default_rng(12)
  V = tok.vocab_size
  shapes = [(a, b, True) for a in LENS for b in (1, 2, 64, 65, 129)] + [(0, b, False) for b in LENS[1:]] * 2
  shapes = [shapes[i] for i in rng.permutation(len(shapes))] + [(0, 511, False), (510, 511, True)]
  A = [draw(rng, a, V) for a, _, _ in shapes]
  B = [draw(rng, b, V) for _, b, _ in shapes]
  return pair_table(A, B, [s for _, _, s in shapes], [bool(x) for x in rng.integers(0, 2, len(A))], tok.cls_id,
                    tok.sep_id, lambda: int(rng.integers(0, V)))


# ---- a. the four segment modes --------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_segment_modes(gpu, mode):
  pk, t = packer('bert'), bert_table()
  check(render_mode(pk, t, mode, 0, t.n), vocab_of(pk), segs_of(t, mode))


@pytest.mark.parametrize('mode', MODES)
def test_segment_modes_codebert(gpu, mode):
  pk, t = packer('codebert'), codebert_table()
  fl = t.flags.cpu().numpy()
  l0 = t.len0.cpu().numpy()
  assert ((fl & 2) == 0).sum() >= 10 and (l0[(fl & 2) == 0] == 0).all() and ((fl & 2) != 0).sum() >= 10
  assert set(fl.tolist()) == {0, 1, 2, 3}  # (is_random_next set on rows of either kind: only bit 1 may move segment 1)
  check(render_mode(pk, t, mode, 0, t.n, codebert=True), vocab_of(pk), segs_of(t, mode))


# ---- b. row ranges ----------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_row_ranges(gpu, mode):
  pk, t = packer('bert'), bert_table()
  vocab, segs = vocab_of(pk), segs_of(t, mode)
  for row0, n in ((0, t.n), (1, 1), (5, 3), (t.n - 1, 1), (7, 0), (t.n, 0)):
    off, data = render_mode(pk, t, mode, row0, n)
    assert off[0] == 0, (row0, n)
    check((off, data), vocab, segs[row0:row0 + n])
    if n == 0:
      assert off.tolist() == [0] and data.size == 0


# ---- c. the two-phase contract -----------------------------------------------------
def raw_render(pk, t, mode, row0, n, out, cap, codebert=False):
  """one lddl_render_strings (mode: MODES) or lddl_render_masked (mode 'masked0' / 'masked1') call:
  (return code, *out_nbytes, the offsets on the host)"""
  from lddl_amd.tokenizer import _ptr, _stream
  L = _lib.lib()
  off = torch.full((n + 1,), -7, dtype=torch.int64, device='cuda')
  nb = ctypes.c_int64(-7)
  tail = (_ptr(off), _ptr(out), cap, ctypes.byref(nb), _stream())
  if mode.startswith('masked'):
    s = int(mode[-1])
    rc = L.lddl_render_masked(pk.tok.handle, _ptr(t.ids), _ptr((t.src0, t.src1)[s]), _ptr((t.len0, t.len1)[s]),
                              _ptr(t.len0), s, _ptr(t.mlm_off), _ptr(t.mlm_pos), _ptr(t.mlm_token), row0, n, *tail)
  else:
    tokens, row_off, l0 = {'span0': (t.ids, t.src0, t.len0), 'span1': (t.ids, t.src1, t.len1)}.get(
        mode, (t.tokens, t.tok_off, t.len0))
    seg = {'seg0': SEG0, 'seg1': SEG1, 'row': ROW, 'span0': SPAN, 'span1': SPAN}[mode]
    rc = L.lddl_render_strings(pk.tok.handle, _ptr(tokens), _ptr(row_off), _ptr(l0), _ptr(t.len1),
                               _ptr(t.flags if codebert else None), row0, n, seg, 1 if codebert else 0, *tail)
  torch.cuda.synchronize()
  return rc, nb.value, off.cpu().numpy()


def two_phase(pk, t, mode, row0, n, vocab, segs):
  eoff, ebytes = reference(vocab, segs[row0:row0 + n])
  rc, nb, off = raw_render(pk, t, mode, row0, n, None, 0)  # the size query
  assert (rc, nb) == (0, len(ebytes)) and np.array_equal(off, eoff), (mode, row0, n, rc, nb)
  buf = torch.full((nb + GUARD,), 0xAA, dtype=torch.uint8, device='cuda')
  if nb > 0:  # one byte short: refused, nothing written, the count still reported
    rc, nb1, _ = raw_render(pk, t, mode, row0, n, buf, nb - 1)
    assert (rc, nb1) == (ECAPACITY, nb), (mode, row0, n, rc, nb1)
    assert b'out_cap %d' % (nb - 1) in _lib.lib().lddl_last_error()
    assert bool((buf == 0xAA).all()), (mode, row0, n)
  rc, nb2, off = raw_render(pk, t, mode, row0, n, buf, nb)  # the next call on the ctx, at the exact capacity
  assert (rc, nb2) == (0, nb) and np.array_equal(off, eoff), (mode, row0, n, rc, nb2)
  got = buf.cpu().numpy()
  check((off, got[:nb]), vocab, segs[row0:row0 + n])
  assert (got[nb:] == 0xAA).all(), (mode, row0, n, got[nb:].tolist())  # (a space after the last token lands here)


@pytest.mark.parametrize('mode', MODES)
def test_two_phase_and_guard_bytes(gpu, mode):
  """every third row alone: rows whose last token sits at each place of a 64-token chunk are the last row"""
  pk, t = packer('bert'), bert_table()
  vocab, segs = vocab_of(pk), segs_of(t, mode)
  for row0, n in [(0, t.n), (3, 9)] + [(r, 1) for r in range(0, t.n, 3)] + [(t.n - 1, 1)]:
    two_phase(pk, t, mode, row0, n, vocab, segs)


# ---- d. more rows than one pass of the grid ------------------------------------------
def rows_table(rows):
  """rows back to back (RENDER_ROW over tok_off; RENDER_SPAN over tok_off[:-1] and the lengths)"""
  t = types.SimpleNamespace(rows=rows, n=len(rows))
  lens = np.fromiter(map(len, rows), dtype=np.int64, count=len(rows))
  t.tokens = u16(np.fromiter((x for r in rows for x in r), dtype=np.int64, count=int(lens.sum())))
  t.tok_off = i64(np.concatenate([[0], np.cumsum(lens)]))
  t.lens = u16(lens)
  return t


def check_rows(pk, rows, row0=0, n=None):
  from lddl_amd import writer
  t = rows_table(rows)
  n = t.n - row0 if n is None else n
  vocab = vocab_of(pk)
  check(writer.render(pk, t.tokens, t.tok_off, row0, n, ROW), vocab, rows[row0:row0 + n])
  check(writer.render(pk, t.tokens, t.tok_off, row0, n, SPAN, len0=t.lens), vocab, rows[row0:row0 + n])
  return t


def test_more_rows_than_one_pass_of_the_grid(gpu):
  """the grid is capped at 32 blocks of 4 waves per CU: 5 rows are some wave's second; the offsets cross
  the scan's 4096-row blocks; masked positions on rows of both passes"""
  from lddl_amd import writer
  pk = packer('bert')
  n = torch.cuda.get_device_properties(0).multi_processor_count * 128 + 5
  assert n > 2 * 4096
  rng = np.random.default_rng(13)
  V = pk.tok.vocab_size
  lens = rng.integers(1, 4, n)
  flat = rng.integers(0, V, int(lens.sum()))
  rows = [r.tolist() for r in np.split(flat, np.cumsum(lens)[:-1])]
  t = check_rows(pk, rows)
  # the rows as A segments ([CLS] at position 0): one masked position on every 1000th row, at 4095 / 4096 and on the last 5
  hit = sorted(set(range(0, n, 1000)) | {4095, 4096} | set(range(n - 5, n)))
  cnt = np.zeros(n, np.int64)
  cnt[hit] = 1
  pos = [1 + int(rng.integers(0, lens[r])) for r in hit]
  new = draw(rng, len(hit), V)
  exp = [list(r) for r in rows]
  for r, p, x in zip(hit, pos, new):
    exp[r][p - 1] = x
  res = types.SimpleNamespace(ids=t.tokens, src0=t.tok_off, len0=t.lens, src1=None, len1=None,
                              mlm_off=i64(np.concatenate([[0], np.cumsum(cnt)])), mlm_pos=u16(pos), mlm_token=u16(new))
  check(writer.render_masked(pk, res, 0, n, 0), vocab_of(pk), exp)


# ---- e. string widths ------------------------------------------------------------------
def test_widths_vocabulary_is_what_the_issue_asks(gpu):
  v = packer('widths').tok.ids_to_tokens
  b = [t.encode() for t in v]
  assert v[:5] == sv.SPECIALS and v[sv.WIDTHS_EMPTY] == '' and v.count('') == 1 and len(set(v)) == len(v)
  assert [len(b[sv.widths_id(k)]) for k in range(256)] == list(range(256))
  assert all(x.isascii() for x in v[:sv.widths_id(255) + 1])
  cont = [x for x in b if x.startswith(b'##')]
  assert [len(x) for x in cont] == [255]
  tails = {len(x[-1].encode()) for x in v if x and not x.isascii()}
  assert tails == {2, 3, 4} and max(map(len, b)) == 255


@pytest.mark.parametrize('name', ['widths', 'specials', 'utf8'])
def test_every_id_once(gpu, name):
  pk = packer(name)
  V = pk.tok.vocab_size
  assert V == sv.vocab_size(name)
  ids = list(range(V))
  check_rows(pk, [ids[i:i + 64] for i in range(0, V, 64)] + [ids[i:i + 65] for i in range(0, V, 65)])


def test_empty_entry_and_longest_rows(gpu):
  pk = packer('widths')
  E, a, b, big = sv.WIDTHS_EMPTY, sv.widths_id(3), sv.widths_id(7), sv.widths_id(255)
  vocab = vocab_of(pk)
  rows = [[E], [a, b], [E, a, b], [a, E, b], [a, b, E], [E, E], [], [E] * 64, [a] * 63 + [E], [a] * 64 + [E],
          [E] + [a] * 64, [E, E, E], [big] * 1024, [E]]
  off, data = reference(vocab, rows)
  assert (off[1], data[off[5]:off[6]], data[off[4]:off[5]]) == (0, b' ', vocab[a] + b' ' + vocab[b] + b' ')
  assert off[13] - off[12] == 1024 * 255 + 1023 and off[14] == off[13]
  check_rows(pk, rows)
  check_rows(pk, rows, 12, 2)  # the longest row, then a row of no bytes as the last


# ---- f. static masking -------------------------------------------------------------------
def seg_edges(n):
  return sorted({k for k in (0, 62, 63, 64, 65, 127, 128, n - 1) if 0 <= k < n})


@functools.lru_cache(maxsize=None)
def masked_table():
  """widths-vocabulary rows with hand-made masked positions.  Per row: (len(A), len(B), what), what =
  'none', 'edges' (tokens 0, 62, 63, 64, 65, 127, 128 and the last of both segments), 'all', a count of
  random positions, 'A' / 'B' (the edges of one segment only, every replacement the empty entry)"""
  spec = [(1, 1, 'all'), (64, 65, 'none'), (64, 65, 'edges'), (65, 64, 'edges'), (129, 129, 'none'),
          (129, 129, 'edges'), (129, 129, 70), (1, 129, 'none'), (129, 129, 130), (64, 65, 'all'), (129, 1, 'A'),
          (1, 129, 'B'), (65, 65, 'none'), (129, 129, 'all'), (510, 511, 'edges')]
  rng = np.random.default_rng(14)
  V = sv.vocab_size('widths')
  E, longest, shortest = sv.WIDTHS_EMPTY, sv.widths_id(255), sv.widths_id(1)
  pool = [i for i, w in enumerate(sv._build('widths')[0]) if 1 < len(w.encode()) < 255]  # 2..254 bytes each
  assert len(pool) >= 256 and max(pool) < V
  pick = lambda n: [pool[int(i)] for i in rng.integers(0, len(pool), n)]  # noqa: E731
  A = [pick(a) for a, _, _ in spec]
  B = [pick(b) for _, b, _ in spec]
  t = pair_table(A, B, [True] * len(spec), [False] * len(spec), 2, 3, lambda: pick(1)[0])
  t.spec = spec
  moff, mpos, mtok, t.kinds = [0], [], [], set()
  t.MA, t.MB = [list(a) for a in A], [list(b) for b in B]
  for r, (la, lb, what) in enumerate(spec):
    ea, eb = [1 + k for k in seg_edges(la)], [la + 2 + k for k in seg_edges(lb)]
    legit = list(range(1, la + 1)) + list(range(la + 2, la + lb + 2))
    pos = {'none': [], 'edges': ea + eb, 'all': legit, 'A': ea, 'B': eb}.get(what)
    if pos is None:
      pos = sorted(int(x) for x in rng.choice(legit, what, replace=False))
    row = t.rows[r]
    for j, p in enumerate(pos):
      kind = 'empty' if what in ('A', 'B') else ('longer', 'shorter', 'equal', 'empty', 'mask')[(j + r) % 5]
      new = {'longer': longest, 'shorter': shortest, 'equal': row[p], 'empty': E, 'mask': 4}[kind]
      k = p - 1 if p <= la else p - la - 2
      where = 'first' if k == 0 else 'last' if k == (la if p <= la else lb) - 1 else 'in'
      t.kinds.add((kind, 'A' if p <= la else 'B', where))
      (t.MA[r] if p <= la else t.MB[r])[k] = new
      mpos.append(p)
      mtok.append(new)
    moff.append(len(mpos))
  t.mlm_off, t.mlm_pos, t.mlm_token = i64(moff), u16(mpos), u16(mtok)
  t.counts = np.diff(moff).tolist()
  return t


def test_masked_table_covers_the_cases(gpu):
  t = masked_table()
  vocab = vocab_of(packer('widths'))
  assert set(t.counts) >= {0, 2, 70, 129, 130, 258} and t.counts[1] == t.counts[4] == 0 < t.counts[2]
  for seg in 'AB':
    assert {k for k, s, _ in t.kinds if s == seg} == {'longer', 'shorter', 'equal', 'empty', 'mask'}
    assert {w for _, s, w in t.kinds if s == seg} == {'first', 'last', 'in'}
    assert {('empty', seg, 'first'), ('empty', seg, 'last')} <= t.kinds
  # longer / shorter are strict: every original has 2..254 bytes
  assert all(1 < len(vocab[x]) < 255 for seg in t.A + t.B for x in seg)
  assert sorted({len(a) for a in t.A} | {len(b) for b in t.B}) == [1, 64, 65, 129, 510, 511]


@pytest.mark.parametrize('seg', [0, 1])
def test_render_masked(gpu, seg):
  from lddl_amd import writer
  pk, t = packer('widths'), masked_table()
  vocab, exp = vocab_of(pk), (t.MA, t.MB)[seg]
  assert exp != (t.A, t.B)[seg]
  for row0, n in ((0, t.n), (3, 4), (1, 1), (t.n - 1, 1), (5, 0), (8, 3)):
    off, data = writer.render_masked(pk, t, row0, n, seg)
    assert off[0] == 0
    check((off, data), vocab, exp[row0:row0 + n])
  # without positions the same call renders the plain spans
  plain = types.SimpleNamespace(**{**vars(t), 'mlm_off': i64(np.zeros(t.n + 1))})
  check(writer.render_masked(pk, plain, 0, t.n, seg), vocab, (t.A, t.B)[seg])


@pytest.mark.parametrize('seg', [0, 1])
def test_render_masked_two_phase_and_guard_bytes(gpu, seg):
  pk, t = packer('widths'), masked_table()
  vocab, exp = vocab_of(pk), (t.MA, t.MB)[seg]
  for row0, n in [(0, t.n), (2, 5)] + [(r, 1) for r in range(t.n)]:
    two_phase(pk, t, 'masked%d' % seg, row0, n, vocab, exp)


# ---- g. a new ctx ---------------------------------------------------------------------------
def test_render_is_the_first_call_of_a_new_ctx(gpu):
  """lddl_render_strings / lddl_render_masked read the byte total back through the ctx's pinned words,
  which lddl_create allocates: no pack, bin or collate call need have run (capi.hip, capi_render.hip;
  the other readers of those words: test_capi_first_call_gpu.py)"""
  from lddl_amd import pipeline, writer
  t = masked_table()
  path = sv.vocab_path('widths')
  pk = pipeline.Packer(path, 0)
  check(writer.render(pk, t.tokens, t.tok_off, 0, t.n, ROW), vocab_of(pk), t.rows)
  check(writer.render(pk, t.tokens, t.tok_off, 2, 3, SEG1, len0=t.len0, len1=t.len1), vocab_of(pk), t.B[2:5])
  pk2 = pipeline.Packer(path, 0)
  check(writer.render_masked(pk2, t, 0, t.n, 1), vocab_of(pk2), t.MB)
  check(writer.render_masked(pk2, t, 0, t.n, 0), vocab_of(pk2), t.MA)


# ---- h. lddl_row_docs ---------------------------------------------------------------------------
SEQ, BIN, DUP, SEED = 64, 16, 2, 31
PDO = [0, 0, 1, 30, 30, 55, 81, 81]  # empty partitions at both ends and inside, a one-document partition


def row_docs_corpus(codebert):
  """81 documents of sentences (BERT) or segments (CodeBERT: + the leading docstring segments per
  document) with empty ones at the start, in the middle, at the end and in runs, whole empty documents
  (at partition edges too) and documents without code"""
  rng = np.random.default_rng(15 + codebert)
  sent = lambda lo=1, hi=30: [int(x) for x in rng.integers(1000, 2000, int(rng.integers(lo, hi)))]  # noqa: E731
  docs, ndoc = [], []
  for d in range(81):
    k = d % 9
    nd = 0
    if d in (1, 29, 54, 55, 80) or k == 8:  # whole empty documents; 1, 29 / 55, 80: first and last of a partition
      doc = [[] for _ in range(1 + d % 3)]
    elif k == 0:
      doc = [sent() for _ in range(1 + d % 7)]
    elif k == 1:
      doc = [[], sent(), sent()]
    elif k == 2:
      doc = [sent(), [], sent(), [], [], [], sent()]
    elif k == 3:
      doc = [sent(), sent(), []]
    elif k == 4:
      doc = [[], [], sent(), [], sent(20, 60), [], []]
    elif k == 5:
      doc = [sent(1, 4)]
    elif k == 6:
      doc = [[], [], [], sent()] + [sent(1, 12) for _ in range(9)] + [[]]
    else:
      doc = [sent(), [], []] + [sent(10, 40) for _ in range(4)]
    if codebert:  # leading docstring segments: none, some, some of them or all of them empty
      nd = (0, 1, 2, 3, len(doc))[d % 5] if any(doc) else d % 2
      nd = min(nd, len(doc))
      if d % 10 == 3:
        doc = doc[:nd] + [[] for _ in doc[nd:]]  # no code: the document is dropped
    docs.append(doc)
    ndoc.append(nd)
  return docs, ndoc


def expected_row_docs(docs, ndoc, codebert, binned):
  """per row in output order: (document, A / doc tokens, B / code tokens) from the oracle's pairs;
  filtered document indices map back through the kept documents of the partition"""
  from oracle import pack_oracle as po
  out = []
  for p in range(len(PDO) - 1):
    kept, D, nd = [], [], []
    for d in range(PDO[p], PDO[p + 1]):
      if codebert:
        ds, cs = [s for s in docs[d][:ndoc[d]] if s], [s for s in docs[d][ndoc[d]:] if s]
        if cs:
          kept.append(d)
          D.append(ds + cs)
          nd.append(len(ds))
      elif any(docs[d]):
        kept.append(d)
        D.append([s for s in docs[d] if s])
    rows = []
    if codebert:
      for doc_s, code_s, dw, cw in po.partition_pairs(D, SEED + p, lambda X, di, r: po.codebert_pairs(X, nd, di, SEQ, 0.1, r), DUP):
        dt = [x for (d, s) in doc_s for x in D[d][s]][dw[0]:dw[1]]
        ct = [x for (d, s) in code_s for x in D[d][s]][cw[0]:cw[1]]
        own = doc_s[0][0] if dt else code_s[0][0]  # the document of the row's first non-empty segment
        assert own == code_s[0][0]
        rows.append((kept[own], dt, ct, len(dt) + len(ct) + (3 if nd[code_s[0][0]] else 2)))
    else:
      for pr in po.partition_pairs(D, SEED + p, lambda X, di, r: po.bert_pairs(X, di, SEQ, 0.1, r), DUP):
        a, b, _ = po.pair_tokens(D, pr)
        rows.append((kept[pr[0][0][0]], a, b, len(a) + len(b) + 3))
    order = po.binned_order([r[3] for r in rows], BIN, SEQ // BIN)[0] if binned else range(len(rows))
    out += [rows[i][:3] for i in order]
  return out


@pytest.mark.parametrize('binned', [False, True])
@pytest.mark.parametrize('codebert', [False, True])
def test_row_docs_vs_oracle(gpu, codebert, binned):
  from lddl_amd import writer
  from test_pack_gpu import shards_from_docs
  docs, ndoc = row_docs_corpus(codebert)
  exp = expected_row_docs(docs, ndoc, codebert, binned)
  assert len(exp) > 100
  if codebert:  # rows with and without a doc segment
    assert any(not e[1] for e in exp) and any(e[1] for e in exp)
  else:  # B from another document than the row's own occurs (is_random_next), so A decides
    assert len({e[0] for e in exp}) > 40
  pk = packer('codebert' if codebert else 'bert')
  sh, ids, ntok = shards_from_docs(docs, ndoc if codebert else None, part_doc_off=PDO)
  res = pk.pack(sh, ids, ntok, target_seq_length=SEQ, duplicate_factor=DUP, seed=SEED, bin_size=BIN if binned else None,
                codebert=codebert)
  assert [(r[1], r[2]) for r in res.rows()] == [(e[1], e[2]) for e in exp]  # the oracle's rows in this order
  got = writer.row_docs(pk, res)
  assert got.dtype == np.int64 and got.tolist() == [e[0] for e in exp]
  # the same through a pack result of its own, after the ctx has packed something else
  from lddl_amd.pipeline import PackHandle
  other = PackHandle(pk.tok)
  res2 = pk.pack(sh, ids, ntok, target_seq_length=SEQ, duplicate_factor=DUP, seed=SEED, bin_size=BIN if binned else None,
                 codebert=codebert, into=other)
  pk.pack(sh, ids, ntok, target_seq_length=SEQ, duplicate_factor=1, seed=SEED + 1, codebert=codebert)
  assert writer.row_docs(pk, res2).tolist() == [e[0] for e in exp]
  other.close()
