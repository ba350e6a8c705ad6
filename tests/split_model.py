"""A byte-level restatement of the sentence split as the GPU kernels
(lddl_amd/csrc/split.hip) compute it -- the position-local rule over UTF-8
bytes and splitnative.props_table() -- and the record families the split
tests share.  Not a test module.

A record is buf[r0, r1).  Mode 0: the id is [r0, i), i the first whitespace
code point (or r1), the body starts at b0, one code point after i (or r1);
mode 1: b0 = r0.  Position p in (b0, r1) is a break when
  1. p starts a non-whitespace code point and the code point before it is
     whitespace;
  2. left of that whitespace run (back to w) lie closers ["')\\]]* and before
     them a run of [.!?], maximal to the left and starting at ms >= b0;
  3. the code point at p is upper case, a digit or one of " ' ( [;
  4. if buf[ms] == '.', the last whitespace-delimited word before ms
     (bounded by b0), lowered and stripped of ( " ' [, is neither in _ABBREV
     nor one alphabetic code point.
The sentences of a record start at the body's first non-whitespace byte and at
its breaks; each ends at the w of the next break, the last one at the body's
end stripped of whitespace.
"""
import numpy as np

from lddl_amd import preprocess, splitnative, synth

P_SPACE, P_UPPER, P_DIGIT, P_ALPHA1 = 1, 2, 4, 8
PIECE = 4096
_ABBREV = frozenset(a.encode() for a in preprocess._ABBREV)
_PUNCT, _CLOSE, _STRIP, _OPEN = b'.!?', b'"\')]', b'("\'[', frozenset(b'"\'([')


class InvalidUtf8(Exception):
  def __init__(self, bad):
    super().__init__('records %r are not strict UTF-8' % (bad,))
    self.bad = bad


def _need(b):
  return 1 if 0xC2 <= b <= 0xDF else 2 if 0xE0 <= b <= 0xEF else 3 if 0xF0 <= b <= 0xF4 else 0


def dec(s, i, n):
  """strict UTF-8 decode at s[i], no byte at or past n read: (code point or -1, length)"""
  b = s[i]
  if b < 0x80:
    return b, 1
  k = _need(b)
  if k == 0 or i + k >= n:
    return -1, 1
  c = b & (0x3F >> k)
  for j in range(1, k + 1):
    x = s[i + j]
    if x & 0xC0 != 0x80:
      return -1, 1
    c = (c << 6) | (x & 0x3F)
  if c < (0x80, 0x800, 0x10000)[k - 1] or c > 0x10FFFF or 0xD800 <= c <= 0xDFFF:
    return -1, 1
  return c, k + 1


def _space_at(s, i, n, tab):
  c, ln = dec(s, i, n)
  return c >= 0 and bool(tab[c] & P_SPACE), ln


def _back(s, i, lo):
  i -= 1
  k = 0
  while k < 3 and i > lo and s[i] & 0xC0 == 0x80:
    i -= 1
    k += 1
  return i


def _rec_of(rec_off, n_rec, p):
  """the record holding byte p: the last one starting at or before p"""
  return min(int(np.searchsorted(rec_off, p, side='right')) - 1, n_rec - 1)


def invalid_records(buf, rec_off):
  """the records that are not strict UTF-8, ascending, found the kernels' way:
  the buffer checked as a whole (a sequence belongs to its lead byte, a
  continuation byte to a lead at most three bytes back) plus "no record
  starts on a continuation byte", which also condemns the record holding the
  lead"""
  s = bytes(buf)
  a = np.frombuffer(s, np.uint8)
  n, n_rec = len(a), len(rec_off) - 1
  bad = set()
  for p in np.flatnonzero(a >= 0x80).tolist():
    b = int(a[p])
    if b & 0xC0 == 0x80:
      cov = False
      for j in range(1, 4):
        if p - j < 0:
          break
        x = int(a[p - j])
        if x & 0xC0 == 0x80:
          continue
        cov = _need(x) >= j
        break
      if not cov:
        bad.add(_rec_of(rec_off, n_rec, p))
    elif dec(s, p, n)[0] < 0:
      bad.add(_rec_of(rec_off, n_rec, p))
  for r in range(n_rec):
    r0, r1 = int(rec_off[r]), int(rec_off[r + 1])
    if r0 < r1 and a[r0] & 0xC0 == 0x80:
      bad.add(r)
      for j in range(1, 4):
        if r0 - j < 0:
          break
        x = int(a[r0 - j])
        if x & 0xC0 == 0x80:
          continue
        if _need(x) >= j:
          bad.add(_rec_of(rec_off, n_rec, r0 - j))
        break
  return sorted(bad)


def _no_break_word(s, a, e, tab):
  while a < e and s[a] in _STRIP:
    a += 1
  while e > a and s[e - 1] in _STRIP:
    e -= 1
  if a >= e:
    return False
  c0, ln = dec(s, a, e)
  if c0 >= 0 and a + ln == e:
    return bool(tab[c0] & P_ALPHA1)
  w = bytearray()
  i = a
  while i < e:
    c, ln = dec(s, i, e)
    if c < 0 or len(w) >= 7:
      return False
    if c < 0x80:
      w.append(c + 32 if 65 <= c <= 90 else c)
    elif c == 0x212A:
      w.append(ord('k'))
    else:
      return False
    i += ln
  return bytes(w) in _ABBREV


def _is_break(s, p, b0, tab):
  """p (in its record, body start b0) starts a new sentence: w, else None"""
  w = p
  while w > b0:
    q = _back(s, w, b0)
    if not _space_at(s, q, w, tab)[0]:
      break
    w = q
  if w == p:
    return None
  j = w
  while j > b0 and s[j - 1] in _CLOSE:
    j -= 1
  ms = j
  while ms > b0 and s[ms - 1] in _PUNCT:
    ms -= 1
  if ms == j:
    return None
  if s[ms] == 0x2E:
    e = ms
    while e > b0:
      q = _back(s, e, b0)
      if not _space_at(s, q, e, tab)[0]:
        break
      e = q
    a = e
    while a > b0:
      q = _back(s, a, b0)
      if _space_at(s, q, a, tab)[0]:
        break
      a = q
    if _no_break_word(s, a, e, tab):
      return None
  return w


def split_model(buf, rec_off, mode, tab=None):
  """-> (data bytes, sent_off, doc_sent_off, id_end) as lddl_split_len /
  lddl_split give them; raises InvalidUtf8 with the bad records"""
  tab = splitnative.props_table() if tab is None else tab
  s = bytes(buf)
  a = np.frombuffer(s, np.uint8)
  rec_off = np.asarray(rec_off, np.int64)
  n_rec = len(rec_off) - 1
  bad = invalid_records(s, rec_off)
  if bad:
    raise InvalidUtf8(bad)
  b0s, fss, ends, id_end = [], [], [], []
  for r in range(n_rec):
    r0, r1 = int(rec_off[r]), int(rec_off[r + 1])
    i, ln = r0, 0
    if mode == 0:
      while i < r1:
        sp, ln = _space_at(s, i, r1, tab)
        if sp:
          break
        i += ln
    id_end.append(i)
    b0 = i + ln if mode == 0 and i < r1 else i
    fs = b0
    while fs < r1:
      sp, ln = _space_at(s, fs, r1, tab)
      if not sp:
        break
      fs += ln
    e = r1
    while e > fs:
      q = _back(s, e, fs)
      if not _space_at(s, q, e, tab)[0]:
        break
      e = q
    b0s.append(b0)
    fss.append(fs if fs < r1 else -1)
    ends.append(e)
  # candidates: a byte that starts a code point allowed by rule 3, behind a byte that can end whitespace
  brk = [[] for _ in range(n_rec)]
  if len(a) > 1:
    asc = np.arange(128)
    start_ok = np.zeros(256, bool)
    start_ok[:128] = (tab[:128] & (P_UPPER | P_DIGIT)) != 0
    start_ok[[ord(c) for c in '"\'([']] = True
    start_ok[0xC0:] = True
    prev_ok = np.zeros(256, bool)
    prev_ok[:128] = (tab[asc] & P_SPACE) != 0
    prev_ok[128:] = True
    cand = np.flatnonzero(start_ok[a[1:]] & prev_ok[a[:-1]]) + 1
    recs = np.minimum(np.searchsorted(rec_off, cand, side='right') - 1, n_rec - 1)
    for p, r in zip(cand.tolist(), recs.tolist()):
      if p <= b0s[r]:
        continue
      c, _ = dec(s, p, int(rec_off[r + 1]))
      if c < 0 or not (tab[c] & (P_UPPER | P_DIGIT) or c in _OPEN):
        continue
      w = _is_break(s, p, b0s[r], tab)
      if w is not None:
        brk[r].append((p, w))
  out, sent_off, dso = [], [0], [0]
  for r in range(n_rec):
    if fss[r] >= 0:
      starts = [fss[r]] + [p for p, _ in brk[r]]
      stops = [w for _, w in brk[r]] + [ends[r]]
      for x, y in zip(starts, stops):
        out.append(s[x:y])
        sent_off.append(sent_off[-1] + y - x)
    dso.append(len(sent_off) - 1)
  return b''.join(out), np.asarray(sent_off, np.int64), np.asarray(dso, np.int64), np.asarray(id_end, np.int64)


def join(raws):
  """records as bytes -> (buffer, rec_off)"""
  rec_off = np.zeros(len(raws) + 1, np.int64)
  np.cumsum([len(r) for r in raws], out=rec_off[1:])
  return b''.join(raws), rec_off


def reference(records, whole_line):
  """preprocess.split_records with the rule splitter -> (data bytes, sent_off,
  doc_sent_off, ids)"""
  c, ids = preprocess.split_records(records, False, preprocess._rule_split, whole_line)
  return bytes(c.data[:c.nbytes]), np.asarray(c.sent_off, np.int64), np.asarray(c.doc_sent_off, np.int64), ids


def model_ids(raws, id_end, rec_off):
  buf = b''.join(raws)
  return [buf[int(rec_off[r]):int(id_end[r])].decode('utf-8') for r in range(len(raws))]


# ------------------------------------------------------------- families --
ATOMS = ['Mr.', 'mr.', 'Dr.', 'U.S.', 'u.k.', 'e.g.', 'i.e.', 'etc.', 'U.K.', 'Ko.', 'A.', 'b.', 'İ.',
         'É.', 'Σ.', 'x.', 'Hello', 'world', 'The', 'the', '42', '٣', 'End.', 'Why?', 'Wow!', '?!',
         '...', '."', ".'", '.)', '.]', '("Hi', "'quoted'", '[x]', '(y)', ' ', ' ', '　', ' ',
         '\u0085', '\x1c', '\t', '\n', '  ', 'café', 'Ångström', '日本', '\U0001F600', 'ABC.',
         '.', '!', '?', 'Ⅲ', '½', '²', 'K.', '((mr.', '"Dr.']


def adversarial(seed, n):
  rng = np.random.default_rng(seed)
  out = []
  for i in range(n):
    parts = []
    for _ in range(int(rng.integers(0, 40))):
      parts.append(ATOMS[int(rng.integers(0, len(ATOMS)))])
      parts.append([' ', '', ' ', '  ', ' '][int(rng.integers(0, 5))])
    sep = [' ', '\t', ' ', ' ', '　'][int(rng.integers(0, 5))]
    rid = ['doc%d' % i, 'dé%d' % i, '', 'x'][int(rng.integers(0, 4))]
    out.append(rid + sep + ''.join(parts) if rng.random() < 0.95 else rid)
  return out


def random_code_points(seed, n):
  """records of code points drawn near the rules' decisions"""
  rng = np.random.default_rng(seed)
  special = [ord(x) for x in '.!?"\')]([ '] + [c for c in range(0x3100) if chr(c).isspace()] + [0x212A, 0x130]
  recs = []
  for _ in range(n):
    cps = []
    for _ in range(int(rng.integers(0, 120))):
      u = rng.random()
      if u < 0.45:
        cps.append(special[int(rng.integers(0, len(special)))])
      elif u < 0.8:
        cps.append(int(rng.integers(65, 123)))
      else:
        c = int(rng.integers(0, 0x110000))
        cps.append(c if not 0xD800 <= c <= 0xDFFF else 0x41)
    recs.append(''.join(map(chr, cps)))
  return recs


EDGE = ['', ' ', 'id', 'id ', 'id  two', 'id A. B. C.', 'id Mr. Smith went. He left.', 'id K. Bob. x.',
        'id End. Next one.', 'id 3.14 is pi. 2 is two.', 'id "Quote." Next.', 'id a.b.c. D', 'id x. İs',
        'id One!  Two?\tThree.\n"Four." (Five.) [Six.] \'Seven.\'', 'id . A', 'id .A . B', 'id ... ... A']


def wiki(nbytes, seed=4):
  docs = synth.make_wiki(nbytes, seed=seed).documents()
  return ['wiki-%d %s' % (i, ' '.join(d)) for i, d in enumerate(docs)]


# (body, the structure sits at the body's start): each is shifted through the 64-byte steps and a piece boundary
STRUCTURES = [
    ('He met Mr. Smith today. Then left', False), ('In the U.S. Army now. Yes', False),
    ('See e.g. Figure two. Done', False), ('It is approx. Five of them', False),
    ('Temp K. Next one', False), ('Name É. Next', False), ('Name İ. Next', False),
    ('Name Σ. Next', False), ('What?!")] 　Next one', False), ('End.\u0085Next.\u0085\u0085Again', False),
    ('Wow' + '!' * 70 + ' Next', False), ('Wow' + '?!.' * 67 + ' Next', False),
    ('End.' + ')' * 70 + ' Next', False), ('End.' + '")]\'' * 50 + ' Next', False),
    ('End.' + ' ' * 70 + 'Next', False), ('End.' + '  \t' * 67 + 'Next', False),
    ('(' * 70 + 'mr. Smith', False), ('(["' * 67 + 'cat. Next', False), ('(' * 200 + 'U.S. Next', False),
    ('. Next one', True), ('?") Next', True), ('The end.   ', False), ('The end. 　\u0085', False),
]
SHIFTS = list(range(0, 131)) + list(range(4090, 4101))


def shift_sweep():
  """records: every structure behind 0..130 and 4090..4100 filler bytes, each case's record starting on a
  piece boundary (a filler record before it pads the buffer up to one)"""
  out, pos = [], 0
  for body, at_b0 in STRUCTURES:
    for k in SHIFTS:
      rec = 'a' * (k + 3) + ' ' + body if at_b0 else 'id ' + 'a' * k + ' ' + body
      pad = -pos % PIECE
      if pad:
        out.append('p ' + 'p' * (pad - 2) if pad >= 2 else 'p')
      out.append(rec)
      pos += pad + len(rec.encode('utf-8'))
  return out


def book(nbytes, seed=9):
  """one record of about nbytes: a whole book"""
  return 'book-1 ' + ' '.join(r.split(' ', 1)[1] for r in wiki(nbytes, seed))


def degenerate(book_bytes):
  """record lists: lengths 0 / 1 / 63 / 64 / 65, id only, id + one whitespace, all-whitespace body, a
  multi-byte id separator, no record, runs of empty records, one very long record"""
  text = 'id ' + 'A b. C d! "E" f? ' * 8
  return [[], [''], [''] * 65, ['a'], ['.'], [' '], [text[:63]], [text[:64]], [text[:65]], ['idonly'], ['id '],
          ['id\t'], ['id   \t 　 \n'], ['id　Body one. Two.'], ['id  Body one. Two.'],
          [''] * 65 + ['id A. B.'] + [''] * 65 + ['x', '', 'id C. D. '],
          [book(book_bytes)]]


INVALID = [b'id bad \xff byte. A', b'id overlong \xc0\x80. A', b'id overlong \xe0\x80\x80. A',
           b'id overlong \xf0\x80\x80\x80. A', b'id surrogate \xed\xa0\x80. A', b'id high \xf4\x90\x80\x80. A',
           b'id five \xf8\x88\x80\x80\x80. A', b'id stray \x80 here. A', b'id stray after \xc3\xa9\xa9. A',
           b'id short \xe2\x82. A', b'id trunc \xe2\x82', b'\xc3', b'i\xcc d']
