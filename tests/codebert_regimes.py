"""The regimes of the CodeBERT packer (lddl_amd/csrc/pack_wave.hip,
pack_codebert_wave_kernel: pretrain_codebert.py:343-442 restated with wave
prefix sums, 64 coins per truncation round, a carried segment and two error
exits), as hand-made corpora that reach them and a host-side trace of the
oracle's walk.  Host only: nothing here touches a GPU.

Per document visit the kernel chooses
  * the docstring: none (no kept docstring line), the first line untruncated
    (the short-sequence draw), or a scan that flushes at line i (the code
    segment count - 1, the reference's quirk, or the first total > max_doc)
    or never flushes (an empty docstring in a row that still has its [SEP]),
  * code chunks [cs, i] from find_over, 64 segments per window, with the
    overflowing segment carried into the next chunk (stay) or lost at the end,
  * per truncation ceil(E / 64) rounds of coins, cut short where the MT19937
    state ends (312 random() calls per 624-word state) and one serial coin
    where a round starts at the twist,
  * to keep a chunk (the first, or >= 16 tokens) or to drop it,
  * IndexError (the code limit is negative) or AssertionError (it is zero).
trace() / classify() restate those formulas over the documents' lengths and
check them against what oracle/pack_oracle.py codebert_pairs drew and returned.
"""
import functools
import random

from oracle import pack_oracle as po

CORPUS_SEED = 3  # the filler documents
DUP = 2
# partition p packs after random.seed(PACK_SEED + p).  At ssp 0.1 the seed
# decides which visits take the first docstring line untruncated: pinned so
# that a visit of a long first line does and a visit of the unflushed
# docstring does not (searched on the host; test_codebert_regimes_host.py
# fails for a seed that misses one)
PACK_SEED = 11
PACK_SEEDS = {(128, 0.1): 11, (512, 0.1): 11}
N_PART = 5
DRAWS_PER_STATE = 312  # random() = 2 of MT19937's 624 words

# (seq, ssp) of the main corpus; (seq, ssp, exception) of the error corpora.
# 5 is the smallest target_seq_length lddl_pack_codebert accepts; there
# max_num = 2 and a 3-token docstring leaves the code -1 tokens
CONFIGS = [(128, 0.0), (128, 0.1), (128, 1.0), (512, 0.0), (512, 0.1), (512, 1.0)]
ERROR_CONFIGS = [(128, 1.0, 'AssertionError'), (128, 1.0, 'IndexError'), (512, 1.0, 'AssertionError'),
                 (512, 1.0, 'IndexError'), (8, 0.0, 'AssertionError'), (5, 0.0, 'IndexError')]


def max_doc(seq):
  return 64 if seq >= 512 else 32  # pack_wave.hip: max_seq >= 512 ? 64 : 32


def bin_size(seq):
  return max(1, seq // 4)


class _Ids:
  """token ids 1000, 1001, ...: every token of a corpus its own id (mod
  48000), so that a window of a row names its place in the document"""

  def __init__(self):
    self.n = 0

  def __call__(self, n):
    out = [1000 + (self.n + k) % 48000 for k in range(n)]
    self.n += n
    return out


def _build(spec):
  """[(docstring line lengths, code segment lengths[, doc_nseg_doc])] -> (docs, ndoc)"""
  ids = _Ids()
  docs, ndoc = [], []
  for d in spec:
    dl, cl = d[0], d[1]
    docs.append([ids(n) for n in list(dl) + list(cl)])
    ndoc.append(d[2] if len(d) > 2 else len(dl))
  return docs, ndoc


def _filler(rnd, n, seq):
  """ordinary documents: 0-3 docstring lines (the first at most 40 tokens) and
  1-8 code segments, some of them empty"""
  out = []
  for _ in range(n):
    dl = [rnd.choice([0, 2, 7, 11, 25, 40])] + [rnd.choice([0, 3, 9, 30, 70]) for _ in range(rnd.randint(0, 2))]
    dl = dl[:rnd.randint(0, 3)]
    cl = [rnd.choice([0, 1, 4, 12, 16, 33, 90, seq]) for _ in range(rnd.randint(1, 8))]
    if not any(cl):
      cl[-1] = 6
    out.append((dl, cl))
  return out


@functools.lru_cache(maxsize=None)
def corpus(seq):
  """-> (docs, ndoc, part_doc_off): documents as lists of segments (id lists,
  empty ones included), doc_nseg_doc per document, N_PART partitions.
  M3 / M2 = the token budget of a row with / without a docstring."""
  M3, M2, MD = seq - 3, seq - 2, max_doc(seq)
  rnd = random.Random(CORPUS_SEED + seq)
  few = 1 if seq < 512 else 6
  # -- partition 0: one or a few documents per docstring regime, and filler
  p0 = [
      ([5, 6], [4, 9, 3, 8, 20]),              # unflushed: stop index 4 lies past 2 lines, 11 <= MD
      ([5, 6], [0, 4, 9, 0, 3, 8, 20, 0]),     # the same with empty code segments: the stop counts kept ones
      ([MD - 1, 1], [40, 50, 60]),             # unflushed at exactly MD
      ([5, 6, 7], [30, 40]),                   # flushed by the stop index 1: two lines
      ([5, 6, 7], [30]),                       # by the stop index 0: one line
      ([MD - 1, 2, 3], [9] * 6),               # total > MD at line 1: the first line alone
      ([MD + 1, 2], [9] * 6),                  # first line > MD alone: kept and cut by 1
      ([MD + 64], [17] * 9),                   # docstring truncation of 64 coins
      ([MD + 65, 3], [17] * 9),                # of 65
      ([1] * 64 + [3, 2, 2], [3] * 66),        # the flush index 64 (seq >= 512): second window of the line scan
      ([1] * 70, [2] * 80),                    # 70 lines, never above 70 tokens
      ([M3 - 20], [7] * 9),                    # short-sequence draw: a first line > MD, 20 tokens left for code
      ([M3 - 20, 4], [0, 7, 7, 0, 30, 7]),
      ([M3 - 1, 9], [5, 0, 6, 40]),            # one token left for code: later chunks of 1 token dropped
      ([M3 - 16], [16, 16, 15, 16]),           # exactly 16 left
      ([0, 0], [8, 9]),                        # only empty docstring lines: a row without a docstring
      ([0, 6, 0, 7, 0], [0, 8, 0, 9, 0]),      # empty segments at the start, middle and end
      ([6, 7], []),                            # docstring only: vanishes
      ([6, 7], [0, 0]),                        # docstring and empty code: vanishes
      ([], [], 0),                             # no segments at all
      ([4], [5, 6], 7),                        # doc_nseg_doc past its 3 segments: all docstring, vanishes
      ([4, 5], [31] * 5, 2),
  ] + _filler(rnd, 10, seq)
  # -- partition 1 is empty
  # -- partition 2: no docstrings up to the twist.  Draw 0 is the first visit's
  # short-sequence draw and 310 coins follow; draw 311 is the second visit's,
  # so its truncation starts at draw 312 = the first draw of the second state
  p2 = [
      ([], [M2 + 310]),
      ([], [M2 + 64]),                         # E == 64, starting at the twist
      ([], [M2 + 65]),                         # E == 65: a round of 64 and a round of 1
      ([], [M2 - 10, 30]),                     # lost tail: the last segment overflows, stays, is never emitted
      ([], [M2 + 1, 15]),                      # later chunk of 15: dropped
      ([], [M2 + 1, 16]),                      # later chunk of 16: kept
      ([], [M2 - 3, 10, 5]),                   # carried 10 + 5 = 15: dropped
      ([], [M2 - 3, 10, 6]),                   # carried 10 + 6 = 16: kept
      ([], [7]),                               # first chunk under 16: kept
      ([], [15]),
      ([], [M2 + 1, 5, M2 + 1, 15, 0, 16]),    # dropped chunks between kept ones
      ([], [M2 + 129]),                        # E > 128
  ] + _filler(rnd, 6, seq)
  # -- partition 3: 300 coins, then a truncation of 65 from draw 302: the round
  # is cut to the 10 coins left, one serial coin at the twist, 54 more
  p3 = [
      ([], [M2 + 300]),
      ([], [M2 + 65]),
      ([], [M2 - 20, 30] + [few] * 100),       # a chunk of > 64 segments from k0 = 2 with a carried base
      ([], [few] * 150 + [M2]),                # > 64 segments from k0 = 0
      ([9], [M3 - 30, 25] + [few] * 90),       # the same beside a docstring
      ([], [M2 + 64]),
      ([3, 4], [M2, M2 + 70, 2, M2 + 200]),
  ] + _filler(rnd, 6, seq)
  # -- partition 4: more than 64 kept documents (the document scan's second window)
  p4 = []
  for k in range(72):
    p4.append(([k % 5] * (k % 3), [1 + k % 19, k % 4] if k % 7 else [0, 3 + k % 30, 0]))
  p4[10] = ([5], [])  # vanishes among them
  parts = [p0, [], p2, p3, p4]
  assert len(parts) == N_PART
  docs, ndoc = _build([d for p in parts for d in p])
  pdo = [0]
  for p in parts:
    pdo.append(pdo[-1] + len(p))
  return docs, ndoc, pdo


def _error_corpus(bad, seq):
  """three partitions; the failing document in the middle of the second"""
  rnd = random.Random(CORPUS_SEED)
  # (at a small seq, ordinary documents of 1-token segments: a docstring leaves them seq - 4 tokens)
  small = lambda n: [([1], [1, 1]) if seq < 16 else d for d in _filler(rnd, n, seq)]  # noqa: E731
  parts = [small(4), small(3) + [bad] + small(3), small(4)]
  docs, ndoc = _build([d for p in parts for d in p])
  return docs, ndoc, [0, 4, 11, 15]


def corpus_assert(seq):
  """the code limit is exactly 0: every code token is cut, AssertionError.
  seq >= 128 (ssp 1.0): a first docstring line of seq - 3 tokens taken whole;
  small seq (ssp 0.0): the scanned docstring fills seq - 3 <= 32 tokens"""
  return _error_corpus(([seq - 3], [9, 9]) if seq >= 128 else ([seq - 3], [1]), seq)


def corpus_index(seq):
  """the code limit is -1: _truncate_seq deletes from an empty list, IndexError"""
  return _error_corpus(([seq - 2], [9, 9]) if seq >= 128 else ([seq - 2], [1]), seq)


def error_corpus(seq, exc):
  return corpus_assert(seq) if exc == 'AssertionError' else corpus_index(seq)


def partition_docs(docs, ndoc, pdo, p):
  """partition p's kept documents as the oracle takes them: empty segments
  dropped, documents without a code segment dropped (:143-161) -> (D, nd)"""
  D, nd = [], []
  for d in range(pdo[p], pdo[p + 1]):
    ds = [x for x in docs[d][:ndoc[d]] if x]
    cs = [x for x in docs[d][ndoc[d]:] if x]
    if cs:
      D.append(ds + cs)
      nd.append(len(ds))
  return D, nd


class CountingRandom(random.Random):
  """random.Random that counts its random() calls and keeps the last value"""

  def __init__(self, seed):
    super().__init__(seed)
    self.n = 0
    self.last = None

  def random(self):
    self.n += 1
    self.last = super().random()
    return self.last

  def getrandbits(self, k):
    # (stated so that shuffle keeps drawing bits: a subclass that overrides
    # random() alone makes random.Random build its integers from random())
    return super().getrandbits(k)


def walk(dl, cl, seq, short):
  """The kernel's per-visit decisions from the segment lengths alone
  (pack_wave.hip: the docstring part and the chunk loop).  dl / cl: kept
  docstring line / code segment lengths; short: the short-sequence draw fell
  below short_seq_prob.  -> dict(flush, dn, Ed, doc_len, chunks, error)"""
  nd, nc = len(dl), len(cl)
  max_num = seq - (3 if nd else 2)
  MD = max_doc(seq)
  flush, dn, dsum, Ed = None, 0, 0, 0
  if nd and short:
    dn, dsum = 1, dl[0]
  elif nd:
    cur = 0
    for i in range(nd):
      cur += dl[i]
      if i == nc - 1 or cur > MD:
        flush = i
        dn = i if (cur > MD and i > 0) else i + 1
        dsum = sum(dl[:dn])
        Ed = max(0, dsum - MD)
        break
  doc_len = dsum - Ed
  lim = max_num - doc_len
  out = dict(nd=nd, nc=nc, short=bool(nd and short), flush=flush, dn=dn, Ed=Ed, doc_len=doc_len, lim=lim, chunks=[],
             error=None, lost_tail=False)
  cs = k0 = carried = nout = 0
  while k0 < nc:
    cur = doc_len + carried
    for i in range(k0, nc):
      cur += cl[i]
      if i == nc - 1 or cur > max_num:
        break
    cn = i - cs + 1
    stay = cur > max_num and cn > 1
    tot = cur - doc_len
    if lim < 0:
      out['error'] = 'IndexError'
      out['chunks'].append(dict(cs=cs, k0=k0, i=i, cn=cn, stay=stay, E=tot, n=0, kept=False, carried=carried))
      return out
    E = max(0, tot - lim)
    n = tot - E
    if n < 1:
      out['error'] = 'AssertionError'
      out['chunks'].append(dict(cs=cs, k0=k0, i=i, cn=cn, stay=stay, E=E, n=0, kept=False, carried=carried))
      return out
    kept = nout == 0 or n >= 16
    nout += kept
    out['chunks'].append(dict(cs=cs, k0=k0, i=i, cn=cn, stay=stay, E=E, n=n, kept=kept, carried=carried))
    cs, carried = (i, cl[i]) if stay else (i + 1, 0)
    k0 = i + 1
    out['lost_tail'] = stay and k0 == nc
  return out


def trace(docs, ndoc, pdo, seq, ssp, dup, seed):
  """Walks po.partition_pairs / po.codebert_pairs with a CountingRandom.  ->
  (visits, rows): per partition the list of visit dicts (walk()'s, plus 'draw':
  the partition's random() count when the visit begins, and 'at' on the
  docstring truncation and on every chunk: the count when that truncation
  begins), and the partition's oracle pairs after the shuffle.  Every visit
  is checked against the oracle: the draws it took and the rows it returned."""
  visits, rows = [], []
  for p in range(len(pdo) - 1):
    D, nd = partition_docs(docs, ndoc, pdo, p)
    rnd = CountingRandom(seed + p)
    pv, pairs = [], []
    for _ in range(dup):
      for di in range(len(D)):
        n0 = rnd.n
        got = po.codebert_pairs(D, nd, di, seq, ssp, rnd)
        pv.append((di, n0, rnd.n, got))
        pairs.extend(got)
    rnd.shuffle(pairs)
    # the same stream again, read by index: a visit's first draw decides its docstring path
    val = random.Random(seed + p)
    stream = [val.random() for _ in range(rnd.n)]
    out = []
    for di, n0, n1, got in pv:
      w = walk([len(s) for s in D[di][:nd[di]]], [len(s) for s in D[di][nd[di]:]], seq, stream[n0] < ssp)
      assert w['error'] is None
      w['di'], w['draw'] = di, n0
      at = n0 + 1
      w['at'] = at
      at += w['Ed']
      for c in w['chunks']:
        c['at'] = at
        at += c['E']
      assert at == n1, ('draws', p, di, at, n1)
      kept = [c for c in w['chunks'] if c['kept']]
      assert len(kept) == len(got), ('rows', p, di)
      for c, (doc_s, code_s, dw, cw) in zip(kept, got):
        assert [s for (_, s) in doc_s] == list(range(w['dn'])) and dw[1] - dw[0] == w['doc_len']
        assert [s for (_, s) in code_s] == list(range(nd[di] + c['cs'], nd[di] + c['i'] + 1))
        assert cw[1] - cw[0] == c['n']
      out.append(w)
    visits.append(out)
    rows.append((D, nd, pairs))
  return visits, rows


def rounds(at, E):
  """trunc_seq_wave's rounds for E coins from draw `at`: list of
  ('serial', 1) | ('wave', n) | ('cut', n) -- cut: fewer than min(E, 64)
  because the state ends"""
  out = []
  while E > 0:
    avail = (DRAWS_PER_STATE - at % DRAWS_PER_STATE) % DRAWS_PER_STATE
    if avail == 0:
      out.append(('serial', 1))
      n = 1
    else:
      n = min(E, 64, avail)
      out.append(('cut' if n < min(E, 64) else 'wave', n))
    at += n
    E -= n
  return out


def classify(visits, seq):
  """visits: trace()'s -> the set of regimes reached, as tuples
    ('doc', 'none' | 'short' | 'short_long' | 'unflushed' | 'stop' | 'over_first' | 'over_drop')
    ('flush_window', w)            the docstring scan flushed at line i, w = i // 64
    ('empty_doc_row',)             a kept row of flags 2 and an empty docstring
    ('lim', lim)                   for lim <= 20
    ('stay',) ('lost_tail',) ('single_over',)   single_over: a one-segment chunk above max_num, not the last
    ('drop', n) ('keep_later', n) ('keep_first', n)   for n <= 16
    ('windows', k0 % 64 != 0, carried > 0)      a chunk scan that crossed a 64-segment window
    ('E', kind, E) for E in (1, 64, 65); ('E>128', kind)   kind: 'doc' | 'code'
    ('cut', kind) ('start_at_twist', kind)
    ('docs>64',)"""
  out = set()
  for part in visits:
    if len({w['di'] for w in part}) > 64:
      out.add(('docs>64',))
    for w in part:
      if not w['nd']:
        out.add(('doc', 'none'))
      elif w['short']:
        out.add(('doc', 'short_long' if w['doc_len'] > max_doc(seq) else 'short'))
      elif w['flush'] is None:
        out.add(('doc', 'unflushed'))
        if any(c['kept'] for c in w['chunks']):
          out.add(('empty_doc_row',))
      else:
        out.add(('flush_window', w['flush'] // 64))
        out.add(('doc', 'stop' if w['dn'] == w['flush'] + 1 and w['Ed'] == 0 and w['flush'] == w['nc'] - 1 else
                 'over_first' if w['dn'] == w['flush'] + 1 else 'over_drop'))
      if w['lim'] <= 20:
        out.add(('lim', w['lim']))
      truncs = [('doc', w['at'], w['Ed'])] + [('code', c['at'], c['E']) for c in w['chunks']]
      for kind, at, E in truncs:
        if E in (1, 64, 65):
          out.add(('E', kind, E))
        if E > 128:
          out.add(('E>128', kind))
        rr = rounds(at, E)
        if any(r[0] == 'cut' for r in rr):
          out.add(('cut', kind))
        if rr and rr[0][0] == 'serial':
          out.add(('start_at_twist', kind))
      for q, c in enumerate(w['chunks']):
        if c['stay']:
          out.add(('stay',))
        if c['cn'] == 1 and c['E'] > 0 and c['i'] < w['nc'] - 1 and c['carried'] == 0:
          out.add(('single_over',))
        if c['n'] <= 16:
          first = not any(x['kept'] for x in w['chunks'][:q])
          out.add(('keep_first' if first else 'keep_later' if c['kept'] else 'drop', c['n']))
        if (c['i'] - c['k0']) // 64 > 0:
          out.add(('windows', c['k0'] % 64 != 0, c['carried'] > 0))
      if w['lost_tail']:
        out.add(('lost_tail',))
  return out


def required(seq, ssp):
  """the regimes configuration (seq, ssp) must reach, from the formulas alone:
  what never depends on a draw everywhere; the scanned docstring where the
  short-sequence draw can fail (ssp < 1); the first line taken whole where it
  can succeed (ssp > 0); the flush index >= 64 only where max_doc = 64"""
  req = {('doc', 'none'), ('stay',), ('lost_tail',), ('single_over',), ('drop', 15), ('keep_later', 16),
         ('keep_first', 7), ('keep_first', 15), ('windows', True, True), ('windows', False, False),
         ('E', 'code', 1), ('E', 'code', 64), ('E', 'code', 65), ('E>128', 'code'), ('cut', 'code'),
         ('start_at_twist', 'code'), ('docs>64',)}
  if ssp < 1.0:
    req |= {('doc', 'unflushed'), ('empty_doc_row',), ('doc', 'stop'), ('doc', 'over_first'), ('doc', 'over_drop'),
            ('flush_window', 0), ('E', 'doc', 1), ('E', 'doc', 64), ('E', 'doc', 65)}
    if seq >= 512:
      req |= {('flush_window', 1), ('E>128', 'doc')}
  if ssp > 0.0:
    req |= {('doc', 'short'), ('doc', 'short_long')}
  if ssp >= 1.0:  # every first line taken whole: the code limits 1, 16 and 20, chunks of one token dropped
    req |= {('lim', 1), ('lim', 16), ('lim', 20), ('drop', 1)}
  return req


@functools.lru_cache(maxsize=None)
def oracle_rows(seq, ssp, seed=None, dup=DUP):
  """-> (visits, rows, counts): trace()'s visits of corpus(seq), the oracle's
  rows (partition, docstring ids, code ids, num_tokens, has_docstring) in the
  binned output order, and the per-partition bin counts.  Computed once per
  configuration and shared; not modified."""
  docs, ndoc, pdo = corpus(seq)
  seed = PACK_SEEDS.get((seq, ssp), PACK_SEED) if seed is None else seed
  visits, parts = trace(docs, ndoc, pdo, seq, ssp, dup, seed)
  return (visits,) + binned_rows(parts, seq)


def binned_rows(parts, seq):
  """trace()'s per-partition (D, nd, pairs) -> (rows, counts) in the binned output order"""
  bs = bin_size(seq)
  nbins = seq // bs
  rows, counts = [], []
  for p, (D, nd, pairs) in enumerate(parts):
    exp = []
    for (doc_s, code_s, dw, cw) in pairs:
      dt = [t for (d, s) in doc_s for t in D[d][s]][dw[0]:dw[1]]
      ct = [t for (d, s) in code_s for t in D[d][s]][cw[0]:cw[1]]
      has = nd[code_s[0][0]] > 0
      exp.append((p, dt, ct, len(dt) + len(ct) + (3 if has else 2), has))
    order, cnt = po.binned_order([e[3] for e in exp], bs, nbins)
    rows += [exp[i] for i in order]
    counts.append(cnt)
  return rows, counts


def golden_rows(case):
  """a case of tests/golden/pack_codebert_regimes.json.gz (the reference's
  rows per partition in the shuffled order) -> (rows, counts) as oracle_rows
  gives them; a row has a docstring when it counts 3 special tokens"""
  bs = bin_size(case['seq'])
  rows, counts = [], []
  for p, part in enumerate(case['parts']):
    exp = [(p, dt, ct, n, n - len(dt) - len(ct) == 3) for dt, ct, n in part]
    order, cnt = po.binned_order([e[3] for e in exp], bs, case['seq'] // bs)
    rows += [exp[i] for i in order]
    counts.append(cnt)
  return rows, counts


def row_tokens(row, cls_id, sep_id):
  """the layout of a CodeBERT row: [CLS] doc [SEP] code [SEP] with a
  docstring (empty or not), else [CLS] code [SEP]"""
  _, dt, ct, n, has = row
  tok = [cls_id] + (dt + [sep_id] if has else []) + ct + [sep_id]
  assert len(tok) == n
  return tok
