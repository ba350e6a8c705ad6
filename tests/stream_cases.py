"""Delayed-producer harness: does a GPU entry point keep to the stream it is given?

The C API promises that work is enqueued on `stream`, and every Python wrapper
takes ``stream=`` or uses the current torch stream.  On the default (legacy
NULL) stream a misrouted launch, memset, copy or read-back is still ordered by
accident, and on an idle side stream with long-finished inputs it still sees
finished inputs.  Here the inputs are NOT finished when the call is issued:

1. the call runs on the default stream with input A, then with input B, fully
   synchronised: the two baselines (the other test modules pin such results to
   the oracle).  They must differ, or the case has no teeth.  B runs last, so a
   recycled caching-allocator block holds B's answer rather than A's;
2. the call's input tensors are filled with B and the device is synchronised;
3. on a fresh ``torch.cuda.Stream()`` s a delay is enqueued (``torch.cuda._sleep``,
   calibrated once to 20-100 ms) and behind it ``inp.copy_(A)`` for every
   staged input;
4. the producer must still be pending (``not s.query()``) when the call is
   issued on s -- ``stream=s`` where the wrapper takes one, with the current
   stream left at the default so that the wrapper's own torch operations are
   exercised, else ``with torch.cuda.stream(s)`` -- and, for calls documented
   as not synchronising, still pending when the call has returned;
5. the outputs are read as a user would (the wrapper's own read-back, or
   after ``s.synchronize()``) and must equal baseline(A): byte for byte for
   device buffers, ``==`` for host values.  Everything is integer work.

What this proves: anything the call enqueues or reads on a stream other than
s before its first synchronisation sees B (or a half-copied mixture) and gives
a different answer, deterministically; so does any read-back that is not
ordered behind s.  What it does not prove: work misrouted after the call has
synchronised s itself (the producer has drained by then) is not caught.

A failing case must give a wrong answer, never a GPU fault, and a misrouted
kernel may run while the copy is half done.  So only arrays for which EVERY
element-wise mixture of A's and B's values is a valid input are staged;
offsets (sent_off, doc_sent_off, part_doc_off, tok_off, src0 / src1, mlm_off,
cu_seqlens, string column offsets) are the same in A and B, in place from the
start and never staged.  ROLES holds, per kind of staged array, how B is made
from A and the rule the pair must meet; check_pair asserts it, on a machine
without a GPU over numpy stand-ins (tests/test_stream_cases_host.py) and on the
GPU over the arrays that are staged, before they are.
"""
import dataclasses
import pickle

import numpy as np

# arrays no case may stage: a stale or half-copied offset can point anywhere
OFFSETS = frozenset(['sent_off', 'doc_sent_off', 'part_doc_off', 'doc_nseg_doc', 'tok_off', 'ids_off', 'src0', 'src1',
                     'len0', 'len1', 'mlm_off', 'cu_seqlens', 'a_off', 'b_off', 'pos_off', 'lab_off', 'rec_off',
                     'chunk_sent0', 'chunk_nsent', 'chunk_off', 'doc_chunk_off', 'rows', 'special_tokens_mask'])


def _is_lower(a):
  return (a >= 97) & (a <= 122)


def _is_upper(a):
  return (a >= 65) & (a <= 90)


def rot_text(a):
  """ASCII letters rotated by one inside their case: every byte keeps its UTF-8
  role, every space, digit and punctuation mark its place; other words, so other tokens"""
  a = np.asarray(a, dtype=np.uint8)
  b = a.copy()
  lo, up = _is_lower(a), _is_upper(a)
  b[lo] = (a[lo] - 97 + 1) % 26 + 97
  b[up] = (a[up] - 65 + 1) % 26 + 65
  return b


def join_words(a):
  """every third space becomes '_': the same bytes per sentence, fewer words (lddl_bart_count's input)"""
  a = np.asarray(a, dtype=np.uint8)
  b = a.copy()
  sp = np.flatnonzero(a == 32)
  b[sp[::3]] = 95
  return b


def bump_ids(a, vocab, special=()):
  """ids in [1000, vocab - 1) move up by one: still in the vocabulary, [CLS] / [SEP] / [MASK] / [PAD] where they were"""
  a = np.asarray(a)
  move = (a >= 1000) & (a < vocab - 1)
  for s in special:
    move &= (a != s) & (a + 1 != s)
  return np.where(move, a + 1, a).astype(a.dtype)


def lower_lengths(a):
  """every third length of 2 or more drops by one: B <= A element-wise and no length that was >= 1 falls below 1"""
  a = np.asarray(a)
  b = a.copy()
  idx = np.flatnonzero(a >= 2)[::3]
  b[idx] -= 1
  return b


def flip_bit0(a):
  """is_random_next (flags bit 0) flipped on every other row; bit 1 (the row's layout) untouched"""
  a = np.asarray(a)
  b = a.copy()
  b[::2] ^= 1
  return b


def _check_text(a, b, m):
  same = a == b
  assert np.all(same | (_is_lower(a) & _is_lower(b)) | (_is_upper(a) & _is_upper(b))), 'a byte changed its role'
  assert np.array_equal(a == 32, b == 32), 'a space moved'


def _check_join(a, b, m):
  assert np.all((a == b) | ((a == 32) & (b == 95))), 'only a space may become an underscore'


def _check_ids(a, b, m):
  v = m['vocab']
  assert a.min() >= 0 and b.min() >= 0 and a.max() < v and b.max() < v, 'an id outside the vocabulary'
  for s in m.get('special', ()):
    assert np.array_equal(a == s, b == s), 'a special token moved'


def _check_lengths(a, b, m):
  assert np.all(b <= a), 'B lengths must be <= A lengths: a mixture then describes sub-ranges of A'
  assert np.all(b >= np.minimum(a, 1)), 'a length fell below the minimum'


def _check_flags(a, b, m):
  assert np.all((a ^ b) & 0xFE == 0), 'only bit 0 may differ'


def _check_range(a, b, m):
  lo, hi = m['range']
  assert min(a.min(), b.min()) >= lo and max(a.max(), b.max()) < hi, 'a value outside [%d, %d)' % (lo, hi)


def _check_any(a, b, m):
  pass


# role -> (B from A, the rule every mixture relies on, why mixtures are in bounds)
ROLES = {
    'text': (lambda a, m: rot_text(a), _check_text, 'valid UTF-8 of the same layout whichever bytes have arrived'),
    'words': (lambda a, m: join_words(a), _check_join, 'ASCII for ASCII: valid UTF-8, the offsets are untouched'),
    'ids': (lambda a, m: bump_ids(a, m['vocab'], m.get('special', ())), _check_ids, 'every id is a vocabulary id'),
    'lengths': (lambda a, m: lower_lengths(a), _check_lengths, 'B <= A: sub-ranges of the ranges tok_off (A\'s) gives'),
    'flags': (lambda a, m: flip_bit0(a), _check_flags, 'bit 0 is a label, not a layout'),
    'num_tokens': (lambda a, m: a[::-1].copy(), _check_range, 'any in-range length bins validly'),
    'values': (lambda a, m: np.roll(a, 1), _check_any, 'copied through as values, never used as an index'),
    'u16': (lambda a, m: (a + 1).astype(a.dtype), _check_any, 'serialised as values, never used as an index'),
}


def make_b(role, a, meta):
  return ROLES[role][0](np.asarray(a), meta)


def check_pair(name, role, a, b, meta):
  """the rule of section 2, mechanically, for one staged array"""
  assert name not in OFFSETS, '%s is an offset array: never staged' % name
  a, b = np.asarray(a), np.asarray(b)
  assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
  assert a.size and not np.array_equal(a, b), '%s: A == B' % name
  ROLES[role][1](a, b, meta)


@dataclasses.dataclass(frozen=True)
class Case:
  """One call under test.  staged: ((array name, role), ...), the inputs that go
  through the delayed copy (device tensors), or for `host` cases the host
  inputs that differ between A and B (the wrapper stages them itself and the
  delay sits ahead of its own copies).  nosync: the call is documented as not
  synchronising, so the producer must still be pending when it returns."""
  id: str
  kind: str
  staged: tuple
  p: dict = dataclasses.field(default_factory=dict)
  nosync: bool = False
  host: bool = False

  def __hash__(self):
    return hash(self.id)


# ---- the delay ---------------------------------------------------------------
def _elapsed_ms(torch, enqueue):
  s = torch.cuda.Stream()
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  with torch.cuda.stream(s):
    e0.record(s)
    enqueue()
    e1.record(s)
  s.synchronize()
  return e0.elapsed_time(e1)


def calibrate(target_ms=60.0, lo=20.0, hi=100.0):
  """-> (enqueue, measured ms): enqueue() queues a delay of about target_ms on
  the current stream.  torch.cuda._sleep with a cycle count measured by two
  events on an idle stream; where that does not land in [lo, hi] ms, a chain
  of matrix products over a private tensor, sized the same way."""
  import torch
  torch.cuda.synchronize()
  if hasattr(torch.cuda, '_sleep'):
    cycles = 1_000_000
    _elapsed_ms(torch, lambda: torch.cuda._sleep(cycles))  # (first launch)
    ms = _elapsed_ms(torch, lambda: torch.cuda._sleep(cycles))
    while ms < 5.0 and cycles < 1 << 40:
      cycles *= 8
      ms = _elapsed_ms(torch, lambda: torch.cuda._sleep(cycles))
    if ms > 0:
      cycles = max(1, int(cycles * target_ms / ms))
      enqueue = lambda: torch.cuda._sleep(cycles)  # noqa: E731
      ms = _elapsed_ms(torch, enqueue)
      if lo <= ms <= hi:
        return enqueue, ms
  x = torch.randn(2048, 2048, device='cuda')
  y = torch.empty_like(x)

  def chain(n):
    for _ in range(n):
      torch.mm(x, x, out=y)
  _elapsed_ms(torch, lambda: chain(4))
  per = _elapsed_ms(torch, lambda: chain(64)) / 64
  n = max(1, int(target_ms / per))
  ms = _elapsed_ms(torch, lambda: chain(n))
  assert lo <= ms <= hi, 'no delay of %g-%g ms could be calibrated (got %.1f ms)' % (lo, hi, ms)
  return (lambda: chain(n)), ms


# ---- the run -------------------------------------------------------------------
def snapshot(out):
  """outputs -> {name: comparable host value}: device tensors and numpy arrays as (dtype, shape, bytes)"""
  import torch
  snap = {}
  for k, v in out.items():
    if callable(v):  # (a part whose extent is itself a result: taken once the work is done)
      v = v()
    if isinstance(v, torch.Tensor):
      v = v.cpu().numpy()
    if isinstance(v, np.ndarray):
      v = (str(v.dtype), v.shape, v.tobytes())
    snap[k] = v
  return snap


def parquet_bytes(path):
  """a parquet file as comparable bytes: its columns' values (the container's metadata may name the writer)"""
  import pyarrow.parquet as pq
  t = pq.read_table(path)
  return pickle.dumps((t.schema.names, [c.to_pylist() for c in t.columns]))


def run_delayed(case, staged, call, delay, meta):
  """staged: [(name, role, live device tensor, A as numpy)]; call(stream, which)
  -> {name: output}, which = 'A' / 'B' for host cases (else the staged tensors
  hold the input).  Returns the three snapshots."""
  import torch
  dev = []
  for name, role, t, a in staged:
    b = make_b(role, a, meta)
    check_pair(name, role, a, b, meta)
    assert not case.host
    a, b = (x.view(np.int16) if x.dtype == np.uint16 else x for x in (np.ascontiguousarray(a), b))  # (torch holds u16 as i16)
    da, db = (torch.from_numpy(np.ascontiguousarray(x)).to(t.device).view(t.dtype).reshape(t.shape) for x in (a, b))
    dev.append((t, da, db))

  def fill(k):
    for t, da, db in dev:
      t.copy_((da, db)[k])
    torch.cuda.synchronize()

  try:
    fill(0)
    base_a = snapshot(call(None, 'A'))
    torch.cuda.synchronize()
    fill(1)
    base_b = snapshot(call(None, 'B'))  # (last: its buffers are what the allocator hands out next)
    torch.cuda.synchronize()
    assert base_a.keys() == base_b.keys()
    assert any(base_a[k] != base_b[k] for k in base_a), 'baseline(A) == baseline(B): the case has no teeth'
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
      delay()
      for t, da, db in dev:
        t.copy_(da, non_blocking=True)
    assert not s.query(), 'the producer finished before the call was issued: nothing was tested'
    out = call(s, 'A')
    if case.nosync:
      assert not s.query(), 'the producer finished inside a call that does not synchronise: nothing was tested'
    s.synchronize()
    got = snapshot(out)
    torch.cuda.synchronize()
  finally:
    if dev:
      fill(0)
  return base_a, base_b, got


def assert_same(case, base_a, base_b, got):
  assert got.keys() == base_a.keys()
  bad = [k for k in base_a if got[k] != base_a[k]]
  assert not bad, '%s on a side stream behind a pending producer: %s differ from the default-stream result%s' % (
      case.id, bad, '; equal to B\'s: ' + str([k for k in bad if got[k] == base_b[k]]))


# ---- the cases -------------------------------------------------------------------
# Shapes: the smallest that launch more than one workgroup and cross a chunk
# boundary: ~250 KB of synthetic Wikipedia in 3 partitions (one empty), 300
# code documents, sequence length 128, bins of 32, duplicate_factor 2, batches of 24 rows.
PACK_KINDS = ('bert', 'masked', 'codebert', 'mlm', 'sop')
_PACK = (('ntok', 'lengths'), ('ids', 'ids'))  # lengths: sub-ranges of A's ranges; ids: vocabulary ids


def _cases():
  c = []
  # text: rotated letters are valid UTF-8 of the same layout, out_ids holds nbytes + 16 ids: no total can pass it
  c += [Case('tokenize[split]', 'tokenize', (('text', 'text'),), dict(algo=5), nosync=True),
        Case('tokenize[serial]', 'tokenize', (('text', 'text'),), dict(algo=0), nosync=True),
        Case('tokenize[fallback]', 'tokenize', (('text', 'text'),), dict(algo=5, dense=True), nosync=True),
        Case('tokenize[packer]', 'tokenize', (('text', 'text'),), dict(algo=5, packer=True))]
  # ntok: B <= A over A's tok_off, so every mixture names sub-ranges of A's sentences; ids: vocabulary ids
  for kind in PACK_KINDS:
    for spans in (False, True):
      c.append(Case('pack[%s-%s]' % (kind, 'spans' if spans else 'rows'), 'pack', _PACK, dict(kind=kind, spans=spans)))
  # tok_off=None: the scan of any mixture of ntok ends at or below A's total, inside the ids buffer
  c += [Case('pack[bert-rows-tok_off_none]', 'pack', (('ntok', 'lengths'),), dict(kind='bert', spans=False, scan=True)),
        Case('pack[bert-spans-tok_off_none]', 'pack', (('ntok', 'lengths'),), dict(kind='bert', spans=True, scan=True)),
        Case('pack[bert-spans-into]', 'pack', _PACK, dict(kind='bert', spans=True, into=True))]
  # the post-pack calls alone (ctypes: no wrapper calls them apart from pack): vocabulary ids, the pack's own spans
  c += [Case('post_pack[rows]', 'post_pack', (('ids', 'ids'),), dict(spans=False), nosync=True),
        Case('post_pack[spans]', 'post_pack', (('ids', 'ids'),), dict(spans=True), nosync=True)]
  # num_tokens: any length in [1, bin_size * nbins] has a bin
  c.append(Case('bin_rows', 'bin', (('num_tokens', 'num_tokens'),)))
  # row_docs reads the pack result alone: A and B are two pack results, nothing is staged
  c.append(Case('row_docs', 'row_docs', (), host=True))
  # render: ids / labels / shown tokens are vocabulary ids rendered as text; positions are serialised as values
  for host in (True, False):
    h = 'host' if host else 'device'
    c += [Case('render[span-%s]' % h, 'render', (('ids', 'ids'),), dict(what='span', host=host)),
          Case('render[labels-%s]' % h, 'render', (('mlm_label', 'ids'),), dict(what='labels', host=host)),
          Case('render_masked[%s]' % h, 'render', (('ids', 'ids'), ('mlm_token', 'ids')), dict(what='masked', host=host)),
          Case('render_npy[%s]' % h, 'render', (('mlm_pos_values', 'u16'),), dict(what='npy', host=host))]
  # the writers end to end: vocabulary ids and the is_random_next bit; offsets, lengths and positions stay
  w = (('ids', 'ids'), ('flags', 'flags'), ('mlm_label', 'ids'), ('mlm_token', 'ids'))
  c += [Case('write_shards[bert]', 'write', w, dict(sink='parquet')),
        Case('write_txt[bert]', 'write', w, dict(sink='txt')),
        Case('write_shards[codebert]', 'write', (('ids', 'ids'),), dict(sink='parquet', code=True))]
  # BART: '_' for ' ' changes the word counts and no offset; the render copies bytes between checked offsets
  c.append(Case('bart_aggregate', 'bart', (('text', 'words'),), dict(what='aggregate')))
  c += [Case('bart_render[%s]' % ('host' if h_ else 'device'), 'bart', (('text', 'text'),), dict(what='render', host=h_))
        for h_ in (True, False)]
  # the splitter stages its own records: nothing device-side, the delay sits ahead of its H2D copies
  c.append(Case('split_device', 'split', (('records', 'text'),), host=True))
  # collate from a row table: res.ids (and the static labels / shown tokens) are vocabulary ids; the spans stay
  for cls, modes in (('bert', (0, 1, 2)), ('code', (0, 2)), ('mlm', (0, 2))):
    for route in ('padded', 'unpadded', 'fixed'):
      for mode in modes:
        st = (('ids', 'ids'),) + ((('mlm_label', 'ids'), ('mlm_token', 'ids')) if mode == 1 else ())
        c.append(Case('collate_rows[%s-%s-%d]' % (cls, route, mode), 'collate', st, dict(cls=cls, route=route, mode=mode)))
  c += [Case('collate_rows[bert-padded-wwm]', 'collate', (('ids', 'ids'),), dict(cls='bert', route='padded', mode=2, wwm=True)),
        Case('collate_rows[bert-unpadded-span]', 'collate', (('ids', 'ids'),),
             dict(cls='bert', route='unpadded', mode=2, span=True))]
  # string routes stage their own columns (rotated letters: same offsets, same token counts)
  c += [Case('load_rows[bert]', 'strings', (('samples', 'text'),), dict(what='load', static=False), host=True),
        Case('load_rows[bert-static]', 'strings', (('samples', 'text'),), dict(what='load', static=True), host=True),
        Case('load_rows[code]', 'strings', (('samples', 'text'),), dict(what='load_code'), host=True),
        Case('collate_call[dynamic]', 'strings', (('samples', 'text'),), dict(what='call', static=False), host=True),
        Case('collate_call[static]', 'strings', (('samples', 'text'),), dict(what='call', static=True), host=True),
        Case('collate_call[special-mask]', 'strings', (('samples', 'text'),), dict(what='encoded'), host=True),
        Case('collate_arrow', 'strings', (('samples', 'text'),), dict(what='arrow'), host=True)]
  # ids pass through as values; labels are compared with ignore_index and copied, capacity = every token
  c += [Case('mask_tokens', 'mask_tokens', (('inputs', 'ids'),)),
        Case('mlm_targets[padded]', 'mlm_targets', (('labels', 'values'),), dict(cu=False)),
        Case('mlm_targets[cu_seqlens]', 'mlm_targets', (('labels', 'values'),), dict(cu=True))]
  return c


CASES = _cases()
VOCAB_SIZES = {'bert': 30522, 'codebert': 52000}


def host_stand_in(name, vocab, rng):
  """a numpy array of the kind the GPU module stages under `name`, made without a GPU"""
  if name in ('text', 'records', 'samples'):
    from lddl_amd import synth
    c = synth.make_wiki(20_000, seed=int(rng.integers(1 << 30)))
    return np.ascontiguousarray(c.data[:c.nbytes])
  if name in ('ids', 'mlm_label', 'mlm_token', 'inputs'):
    a = rng.integers(0, vocab, 5000)
    a[::17] = rng.integers(0, 1000, len(a[::17]))  # (the special and unused ids)
    return a.astype(np.int64 if name == 'inputs' else np.uint16)
  if name == 'ntok':
    return rng.integers(0, 60, 3000).astype(np.int32)
  if name == 'flags':
    return rng.integers(2, 4, 3000).astype(np.uint8)
  if name == 'num_tokens':
    return rng.integers(1, 129, 3000).astype(np.int64)
  if name == 'mlm_pos_values':
    return rng.integers(0, 128, 3000).astype(np.uint16)
  if name == 'labels':
    a = rng.integers(0, vocab, 3000).astype(np.int64)
    a[rng.random(3000) < 0.85] = -1
    return a
  raise KeyError(name)


def meta_for(case, vocab_sizes=VOCAB_SIZES, special=(0, 100, 101, 102, 103)):
  code = case.p.get('kind') == 'codebert' or case.p.get('cls') == 'code' or case.p.get('code') \
      or case.p.get('what') == 'load_code'
  return {'vocab': vocab_sizes['codebert' if code else 'bert'], 'special': tuple(special), 'range': (1, 129)}
