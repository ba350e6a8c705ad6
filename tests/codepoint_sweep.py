"""Every Unicode scalar value as tokenizer input: the corpora of the code-point
sweep and the digests its golden file keeps.  No GPU, no pytest; shared by
tools/gen_golden_codepoints.py (HF tokenizers -> tests/golden/tok_codepoints.npz),
tests/test_codepoints_host.py (the oracle) and
tests/test_tokenize_codepoints_gpu.py (both GPU paths).

A family is one corpus, (data, sent_off) through synth.corpus_from_sentences:

  alone      chr(c)                    inner    'a' + chr(c) + 'b'
  spaced     'a ' + chr(c) + ' b'      doubled  chr(c) * 2
  after_e    'e' + chr(c)              upper    'A' + chr(c) + 'A'
  run40      40 consecutive code points joined with nothing (dense windows)
  run40sp    the same joined with ' '
  markpairs  every ordered pair (x, y) of one mark per non-zero combining
             class: 'a'+x+y+'b' and 'e'+x+y+x (canonical reordering)
  len100     WordPiece's 100-character rule after normalisation: chr(c) * k
             for k in LEN100_REPS and 'x'*k + chr(c) + 'y'*(99-k) for k in
             LEN100_AT, c every 7th code point that normalisation changes
  markwords  the marks that survive normalisation with a non-zero combining
             class (the tokenizer strips Mn by its own, older category table:
             83 code points stay, 57 vocabulary entries of codebert hold one),
             so that their canonical order decides the ids: for every ordered
             pair (x, y) of them x+y, 'a'+x+y+'b', x+U+0301+y (a stripped mark
             between) and 'e'+x+y+' '+y+x; every triple x+y+z of the lowest
             of each class; MARKWORDS_EXTRA

unicodedata only chooses inputs (select()); the golden file stores the
selections, so a test's corpora do not depend on its Python's Unicode version,
and never supplies an expected value.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
from lddl_amd import synth  # noqa: E402

# every scalar value: U+0000..U+10FFFF without the surrogates
CPS = np.concatenate([np.arange(0, 0xD800), np.arange(0xE000, 0x110000)]).astype(np.int32)
assert len(CPS) == 1_112_064

BLOCK = 512  # sentences per digest block
RUN = 40
LEN100_REPS = (33, 34, 50, 51, 99, 100, 101)
LEN100_AT = (0, 98, 99)
# a word the adversarial test met: classes 230, 216, 230, the middle one moves to the front
MARKWORDS_EXTRA = ['\u08d9\U0001d16e\u08d4', 'b \u08d9\U0001d16e\u08d4', '\u08d9\U0001d16e\u08d4 b']

PER_CP = {'alone': ('', '', 1), 'inner': ('a', 'b', 1), 'spaced': ('a ', ' b', 1), 'doubled': ('', '', 2),
          'after_e': ('e', '', 1), 'upper': ('A', 'A', 1)}
FAMILIES = ['alone', 'inner', 'spaced', 'doubled', 'after_e', 'upper', 'run40', 'run40sp', 'markpairs', 'len100',
            'markwords']
# what the golden file holds per vocabulary
GOLDEN_FAMILIES = {'bert': FAMILIES, 'codebert': ['alone', 'spaced', 'run40sp', 'markpairs', 'len100', 'markwords']}
GOLDEN_FILE = 'tok_codepoints.npz'


def select(normalize):
  """{'marks', 'len100', 'kept'}: the code points of markpairs, len100 and
  markwords, chosen with this Python's unicodedata (the generator's; the tests
  read the golden's) and, for 'kept', normalize(str) -> str, the reference
  normalizer: the code points of a non-zero combining class that it keeps"""
  import unicodedata
  first = {}
  changed = []
  for c in CPS.tolist():
    ch = chr(c)
    k = unicodedata.combining(ch)
    if k and k not in first:
      first[k] = c
    if len(unicodedata.normalize('NFD', ch)) != 1 or unicodedata.category(ch) in ('Mn', 'Cc', 'Cf'):
      changed.append(c)
  kept = [c for c in CPS.tolist() if unicodedata.combining(chr(c)) and normalize('a' + chr(c)) != 'a']
  return {'marks': np.array([first[k] for k in sorted(first)], np.int32), 'len100': np.array(changed[::7], np.int32),
          'kept': np.array(kept, np.int32), 'kept_class': np.array([unicodedata.combining(chr(c)) for c in kept], np.int32)}


def _kept_reps(sel):
  """the lowest kept mark of each combining class, by class"""
  first = {}
  for c, k in zip(sel['kept'].tolist(), sel['kept_class'].tolist()):
    first.setdefault(k, c)
  return [first[k] for k in sorted(first)]


_MARKWORDS = {}


def _markwords(sel):
  """[(sentence, its code points under test), ...] (built once per selection)"""
  kept = sel['kept'].tolist()
  if tuple(kept) in _MARKWORDS:
    return _MARKWORDS[tuple(kept)]
  out = []
  for x in kept:
    for y in kept:
      a, b = chr(x), chr(y)
      out += [(s, [x, y]) for s in (a + b, 'a' + a + b + 'b', a + '\u0301' + b, 'e' + a + b + ' ' + b + a)]
  reps = _kept_reps(sel)
  out += [(chr(x) + chr(y) + chr(z), [x, y, z]) for x in reps for y in reps for z in reps]
  out += [(s, [0x8D9, 0x1D16E, 0x8D4]) for s in MARKWORDS_EXTRA]
  _MARKWORDS[tuple(kept)] = out
  return out


def sentences(family, sel=None):
  """the family's sentences, in corpus order"""
  if family in PER_CP:
    pre, post, rep = PER_CP[family]
    return [pre + chr(c) * rep + post for c in CPS.tolist()]
  if family in ('run40', 'run40sp'):
    chars = [chr(c) for c in CPS.tolist()]
    sep = ' ' if family == 'run40sp' else ''
    return [sep.join(chars[i:i + RUN]) for i in range(0, len(chars), RUN)]
  if family == 'markpairs':
    marks = [chr(c) for c in sel['marks'].tolist()]
    return [s for x in marks for y in marks for s in ('a' + x + y + 'b', 'e' + x + y + x)]
  if family == 'len100':
    out = []
    for c in sel['len100'].tolist():
      ch = chr(c)
      out += [ch * k for k in LEN100_REPS]
      out += ['x' * k + ch + 'y' * (99 - k) for k in LEN100_AT]
    return out
  if family == 'markwords':
    return [s for s, _ in _markwords(sel)]
  raise KeyError(family)


def sentence_cps(family, sel, i):
  """the code points under test in sentence i of the family"""
  if family in PER_CP:
    return [int(CPS[i])]
  if family in ('run40', 'run40sp'):
    return CPS[i * RUN:(i + 1) * RUN].tolist()
  if family == 'markpairs':
    n = len(sel['marks'])
    return [int(sel['marks'][(i // 2) // n]), int(sel['marks'][(i // 2) % n])]
  if family == 'len100':
    return [int(sel['len100'][i // (len(LEN100_REPS) + len(LEN100_AT))])]
  if family == 'markwords':
    return _markwords(sel)[i][1]
  raise KeyError(family)


def n_sentences(family, sel=None):
  if family in PER_CP:
    return len(CPS)
  if family in ('run40', 'run40sp'):
    return (len(CPS) + RUN - 1) // RUN
  if family == 'markpairs':
    return 2 * len(sel['marks']) ** 2
  if family == 'markwords':
    return 4 * len(sel['kept']) ** 2 + len(_kept_reps(sel)) ** 3 + len(MARKWORDS_EXTRA)
  return len(sel['len100']) * (len(LEN100_REPS) + len(LEN100_AT))


def block_range(family, sel, b, n_sent):
  """'U+XXXX..U+YYYY': the code points under test in digest block b"""
  cps = [c for i in range(b * BLOCK, min(n_sent, (b + 1) * BLOCK)) for c in sentence_cps(family, sel, i)]
  return 'U+%04X..U+%04X' % (min(cps), max(cps))


_CORPORA = {}


def corpus(family, sel=None):
  """(data uint8[nbytes], sent_off int64[n+1]) of the family, built once per
  process (read-only: the tests share it)"""
  if family not in _CORPORA:
    s = sentences(family, sel)
    c = synth.corpus_from_sentences(s, [0, len(s)])
    c.data.setflags(write=False)  # (sent_off goes to torch.from_numpy as it is, which wants it writable)
    _CORPORA[family] = (c.data, c.sent_off)
  return _CORPORA[family]


def sentence_text(data, sent_off, i):
  return bytes(data[sent_off[i]:sent_off[i + 1]]).decode('utf-8')


def _u64(h):
  return np.frombuffer(h.digest(), dtype='<u8')[0]


def corpus_digest(data, sent_off):
  """blake2b-64 over sent_off (little-endian int64) and then the bytes"""
  h = hashlib.blake2b(digest_size=8)
  h.update(np.ascontiguousarray(sent_off, dtype='<i8').tobytes())
  h.update(np.ascontiguousarray(data, dtype=np.uint8).tobytes())
  return _u64(h)


def digest_blocks(ids_per_sentence, ntok):
  """(uint64[nblocks], int64[nblocks]): per block of BLOCK consecutive
  sentences, blake2b-64 over the block's ntok as little-endian int32 followed
  by its ids as little-endian int32, and the block's token total.
  ids_per_sentence: the emitted ids in sentence order, one flat array (CSR by
  ntok) or a sequence of per-sentence sequences."""
  ntok = np.ascontiguousarray(ntok, dtype='<i4')
  if isinstance(ids_per_sentence, np.ndarray) and ids_per_sentence.ndim == 1 and ids_per_sentence.dtype != object:
    flat = ids_per_sentence
  else:
    flat = np.fromiter((x for s in ids_per_sentence for x in s), dtype=np.int64)
  flat = np.ascontiguousarray(flat, dtype='<i4')
  off = np.zeros(len(ntok) + 1, np.int64)
  np.cumsum(ntok, out=off[1:])
  assert off[-1] == len(flat), (int(off[-1]), len(flat))
  nb = (len(ntok) + BLOCK - 1) // BLOCK
  dig = np.zeros(nb, np.uint64)
  tot = np.zeros(nb, np.int64)
  for b in range(nb):
    s0, s1 = b * BLOCK, min(len(ntok), (b + 1) * BLOCK)
    h = hashlib.blake2b(digest_size=8)
    h.update(ntok[s0:s1].tobytes())
    h.update(flat[off[s0]:off[s1]].tobytes())
    dig[b] = _u64(h)
    tot[b] = off[s1] - off[s0]
  return dig, tot


def emitted_index(ntok, sent_off):
  """positions of the emitted ids in the sparse layout (sentence s's ids from
  byte offset sent_off[s] - sent_off[0] on), in sentence order"""
  ntok = np.asarray(ntok, dtype=np.int64)
  starts = np.asarray(sent_off[:-1], dtype=np.int64) - int(sent_off[0])
  return np.repeat(starts, ntok) + (np.arange(int(ntok.sum())) - np.repeat(np.cumsum(ntok) - ntok, ntok))


def flat_ids(sparse, ntok, sent_off):
  """sparse ids (oracle.OracleTokenizer.run, test_tokenize_gpu.run_hip) -> the flat CSR ids as int32"""
  return np.asarray(sparse)[emitted_index(ntok, sent_off)].astype(np.int32)


def first_bad_blocks(dig, tot, gdig, gtot):
  """indices of the blocks whose digest or token total differs from the golden's"""
  if len(dig) != len(gdig):
    return [min(len(dig), len(gdig))]
  return np.flatnonzero((dig != gdig) | (tot != gtot)).tolist()


def golden_key(vocab, family, what):
  return '%s_%s_%s' % (vocab, family, what)


def golden_selection(g):
  return {'marks': g['sel_marks'], 'len100': g['sel_len100'], 'kept': g['sel_kept'], 'kept_class': g['sel_kept_class']}
