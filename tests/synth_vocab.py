"""Synthetic vocabularies for the tokenizer, table and masking tests: each one
is built to reach a path of lddl_amd/csrc/tok_tables.h, tokenize_split.hip or
pack_wave.hip that bert_vocab.txt and codebert_52000_vocab.txt never reach
(DESIGN.md section 4 lists them).  Everything is a deterministic function of
the vocabulary's name.  The small ones are also committed under
tests/golden/vocabs/ (tests/test_vocab_oracle.py checks they still match);
the large ones are generated at test time, and so is 'widths' (the render
tests' vocabulary: no tokenizer golden, not one of NAMES).  Plain helper
module: no fixtures, no pytest settings.

  vocab_bytes(name)   the vocab.txt bytes
  vocab_path(name)    a file holding them (golden/vocabs/ or a temp dir)
  targeted(name)      sentences written for the vocabulary's cases
  common_sentences()  synthetic wiki + adversarial sentences, the same for all
"""
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB_DIR = os.path.join(HERE, 'golden', 'vocabs')
SPECIALS = ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]']
LETTERS = 'abcdefghijklmnopqrstuvwxyz'
DIGITS = '0123456789'
PUNCT = list('.,;:!?()[]\'"-/%$&*+=<>_#@')
WORDS = ['the', 'of', 'and', 'in', 'to', 'was', 'is', 'for', 'as', 'on', 'with', 'by', 'he', 'at', 'from', 'his',
         'an', 'were', 'are', 'which', 'hello', 'world', 'un', '##able', '##aff', '##ing', '##ed', '##ly']

SMALL = ['collide', 'long_a', 'long_b', 'ext', 'utf8', 'sparse_a', 'sparse_b', 'specials', 'specials_padlast',
         'blanks', 'crlf', 'dupspecial', 'tiny5', 'tiny6', 'tiny64', 'tiny65']
SIZES = [32768, 32769, 61440, 61441, 65535, 65536]
LARGE = ['v%d' % v for v in SIZES]
NAMES = SMALL + LARGE
# vocabularies whose lines need parsing decisions: HF's token -> id map of each is in golden/vocab_lines_hf.json
LINE_VOCABS = ['blanks', 'crlf', 'dupspecial', 'specials', 'specials_padlast']


def _base():
  """single letters / digits and their '##' forms, punctuation, a few words:
  every ASCII word tokenises to something"""
  return (list(LETTERS) + list(DIGITS) + ['##' + c for c in LETTERS + DIGITS] + PUNCT + WORDS)


def _pat(n, salt):
  """n letters, a fixed function of salt; _pat(n, s) is a prefix of _pat(m, s) for n < m"""
  out, x = [], (salt * 2654435761 + 12345) & 0xFFFFFFFF
  for _ in range(n):
    x = (x * 1103515245 + 12345) & 0x7FFFFFFF
    out.append(LETTERS[(x >> 16) % 26])
  return ''.join(out)


# ---- collide: groups sharing the first 12 bytes, the length and the flag ----
# (vhash, common.h, reads nothing else: a group's members share a home bucket)
GROUP = 6  # two slots of the home bucket, two of the next, two of a third


def _collide_groups():
  """[(cont, members, non_member)]"""
  groups = []
  k = 0
  for cont in (0, 1):
    for n in (13, 14, 16, 17, 20, 24):
      stem = _pat(12, 100 + k)
      k += 1
      tails = [_pat(n - 12, 200 + 10 * k + j) for j in range(GROUP + 1)]
      assert len(set(tails)) == GROUP + 1 or n == 13
      if n == 13:
        tails = list('abcdefg')
      groups.append((cont, [stem + t for t in tails[:GROUP]], stem + tails[GROUP]))
  for cont in (0, 1):
    # members that differ only in bytes 12..23 (byte 20), at 24 bytes
    stem = _pat(20, 300 + cont)
    groups.append((cont, [stem + c + 'xyz' for c in 'abcdef'], stem + 'gxyz'))
    # members that differ only after byte 24 (byte 27), at 30 bytes: the slot
    # keys are equal, the pool compare decides
    stem = _pat(27, 310 + cont)
    groups.append((cont, [stem + c + 'xy' for c in 'abcdef'], stem + 'gxy'))
  return groups


def _collide():
  v = SPECIALS + _base() + ['zq']
  words = []
  for cont, members, non in _collide_groups():
    v += [('##' if cont else '') + m for m in members]
    for w in members + [non]:
      words.append(('zq' if cont else '') + w)
  return v, words


def collide_displaced_words():
  """whole-word members past the first of each group: their home slot 0 holds
  the group's first member, so the scan cannot resolve them (a record each)"""
  return [m for cont, members, _ in _collide_groups() if not cont for m in members[1:]]


# ---- long: keys of 24..100 bytes / chars --------------------------------------
LONG_N = (24, 25, 26, 55, 56, 57, 99, 100)
CYR = 'бвгджзклмнпрстфхцчшщ'  # 2-byte lowercase letters without a decomposition


def _cpat(n, salt):
  return ''.join(CYR[LETTERS.index(c) % len(CYR)] for c in _pat(n, salt))


def _long(variant):
  """variant 'a': maxb[0] (200) < maxb[1] (202); 'b': the reverse"""
  v = SPECIALS + _base() + ['zq'] + list(CYR) + ['##' + c for c in CYR]
  words = []
  for cont in (0, 1):
    pre, tp = ('##', 'zq') if cont else ('', '')
    keys = [_pat(n, 400 + cont) for n in LONG_N]             # nested: each a prefix of the next
    keys += [_pat(n, 410 + cont + n) for n in LONG_N]        # unrelated stems
    keys += [_cpat(n, 420 + cont) for n in LONG_N]           # n chars = 2n bytes, nested
    for n in (26, 57, 100):                                  # equal through byte 24 (and far beyond)
      p = _pat(n - 1, 430 + cont + n)
      keys += [p + 'a', p + 'b']
      words += [tp + p + 'c']
    unreachable = _cpat(101, 440 + cont)                     # 101 chars: the word is [UNK] before any lookup
    if (variant == 'a') == (cont == 1):
      keys.append(unreachable)
      words.append(tp + unreachable)
    v += [pre + k for k in keys]
    for k in keys:
      words += [tp + k, tp + k + 'x', tp + k[:-1], tp + k + k[:3]]
  return v, words


# ---- ext: the extension chain of the dword-group Bloom scan ------------------
def _ext():
  s1, s2, s3 = _pat(24, 500), _pat(24, 501), _pat(24, 502)
  s4 = _pat(24, 503)
  v = SPECIALS + _base()
  v += [s1[:k] for k in range(2, 25)]          # every length of one stem (1 is a letter of the base)
  v += [s2]                                    # 24 bytes, no shorter prefix of it a key but its first letter
  v += ['##' + s3]
  v += [s4[:2], s4[:3], s4]                    # extension bits set for 4..20 bytes, real matches of 2 and 3
  v += ['##' + s4[:k] for k in (5, 9, 13, 17, 21)]
  words = []
  for k in range(1, 25):
    words += [s1[:k], s1[:k - 1] + ('q' if s1[k - 1] != 'q' else 'j'), s1[:k] + 'qq']
    words += [s2[:k], s3[0] + s3[:k], s4[:k], s4[:k] + s4[:k]]
  words += [s2 + 'x', 'x' + s3 + 'x', s4 + s4, s1 + s1]
  return v, words


# ---- utf8: keys of multi-byte characters ending at bytes 23, 24, 25 -----------
HIRA = 'あいうえおかきくけこさしすせそたちつてと'  # 3-byte, not CJK ideographs, no decomposition
GOTH = '𐌰𐌱𐌲𐌳𐌴𐌵𐌶𐌷𐌸𐌹'                      # 4-byte, caseless


def _utf8():
  c2, c3, c4 = CYR, HIRA, GOTH
  keys = [
      'a' + c2[:11], c2[:12], 'a' + c2[:12],               # 23, 24, 25 bytes of 2-byte chars
      'ab' + c3[:7], c3[:8], 'a' + c3[:8], 'a' + c3[:7] + c3[9],  # 23, 24, 25; 25 with a char over byte 24
      'abc' + c4[:5], c4[:6], 'a' + c4[:6],                # 23, 24, 25 bytes of 4-byte chars
      'ab' + c2[3] + c3[3] + c4[3] + 'cd' + c2[4] + c3[4] + c4[4] + 'e',  # mixed, 23
      c3[10:18] + c2[0], c3[10:18] + c2[1],                # 26 bytes, equal through byte 24
      c2[5:18] + c3[0] + c4[0],                            # 33 bytes
      'cafe', 'istanbul', 'strasse', 'ångström', 'école',  # the last two hold accents: unreachable
      '中', '文', '中文', '字',
  ]
  single = list(c2) + list(c3) + list(c4)
  v = SPECIALS + _base() + single + ['##' + c for c in single] + keys + ['##' + k for k in keys[:14]]
  words = []
  for k in keys[:14]:
    words += [k, k + 'x', k[:-1], 'a' + k, k + k[-1], k.upper()]
  # words longer than maxb whose cut falls inside a character
  words += ['ab' + c3 * 2, 'a' + c3 * 2, c3 * 2, 'abc' + c4 * 3, 'a' + c2 * 2 + c3, c4 * 4 + c2]
  words += ['Café', 'CAFÉ', 'café', 'İstanbul', 'ISTANBUL', 'Straße', 'ångström', 'Ångström', 'école', 'Ecole',
            '中文', '中文字abc中', 'a中b', '字' * 5]
  return v, words


# ---- sparse -------------------------------------------------------------------
def _sparse_a():
  """no single-letter keys: most words are [UNK]"""
  return SPECIALS + WORDS + PUNCT, ['the', 'theory', 'hello', 'helloworld', 'unaffable', 'x', 'of', 'off']


def _sparse_b():
  """single characters and '##x' only: a word of n letters is n pieces"""
  v = SPECIALS + list(LETTERS + DIGITS) + ['##' + c for c in LETTERS + DIGITS] + PUNCT
  return v, [_pat(n, 600 + n) for n in (1, 2, 4, 5, 27, 28, 29, 30, 56, 57, 60, 100, 101)]


# ---- specials at odd ids, duplicates, an empty line, no final newline ----------
def _specials_lines(pad_last):
  b = _base()
  h = len(b) // 2
  mid = ['dup', 'first', 'dup', '', 'second', '##dup', 'third', '##dup']
  tail = ['[MASK]', '[PAD]'] if pad_last else ['[PAD]', '[MASK]']
  return ['[UNK]'] + b[:h] + ['[CLS]'] + mid + ['[SEP]'] + b[h:] + ['dup'] + tail


SPECIALS_WORDS = ['dup', 'first', 'second', 'third', 'xdup', 'dupdup', 'thedup', '[CLS]dup[SEP]', '[MASK]', '[PAD]x',
                  '[UNK]', 'a[MASK]b']

# ---- vocab lines with trailing blanks (HF trims every trailing White_Space) -----
# every code point with the Unicode White_Space property, and some that look
# like blanks but lack it: one vocab line 'wsNN' + the code point each
WHITE_SPACE = ([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
               [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
NOT_WHITE_SPACE = [0x1C, 0x1D, 0x1E, 0x1F, 0x180E, 0x200B, 0x200C, 0x2060, 0xFEFF]


def _ws_key(k):
  return 'ws' + LETTERS[k // 26] + LETTERS[k % 26]


WS_LINES = [_ws_key(k) + chr(c) for k, c in enumerate(WHITE_SPACE) if c != 0x0A]  # (a line feed ends the line)
NWS_LINES = [_ws_key(30 + k) + chr(c) for k, c in enumerate(NOT_WHITE_SPACE)]
BLANK_LINES = (['ab ', 'cd\t', 'ef \t ', 'gh\u00a0', 'ij\u3000', 'kl\x0b', 'mn\x1c', 'op\u200b', ' qr', 'st st',
                'ab', 'uv\r', 'wx\r ', '##yz ', 'ab  ', 'yz\u2003\u00a0 \u3000\t'] + WS_LINES + NWS_LINES)
BLANK_WORDS = (['ab', 'cd', 'ef', 'gh', 'ij', 'kl', 'mn', 'op', 'qr', 'st', 'uv', 'wx', 'yz', 'abyz', 'abab', 'mn\x1c',
                'op\u200b', 'ab cd ef gh ij kl mn op qr st uv wx'] +
               [_ws_key(k) for k in range(len(WHITE_SPACE))] + [_ws_key(30 + k) for k in range(len(NOT_WHITE_SPACE))] +
               NWS_LINES)

# ---- a special on two lines: the last one is the special's id ---------------
DUPSPECIAL_WORDS = ['[MASK]', '[SEP]', '[CLS]', 'a[MASK]b', 'the [SEP] of [MASK]', '[SEP][SEP]', '[PAD] [UNK] x',
                    'mask', '[mask]', 'hello [CLS] world [SEP]']


def _dupspecial_lines():
  """[MASK] and [SEP] twice, [UNK] twice with the later one last in the file"""
  b = _base()
  h = len(b) // 2
  return ['[PAD]', '[UNK]', '[CLS]', '[SEP]', '[MASK]'] + b[:h] + ['[MASK]', '[UNK]'] + b[h:] + ['[SEP]']


def _filler(i):
  """a 7-letter word unique to i, not in the base"""
  s = ''
  for _ in range(5):
    s = LETTERS[i % 26] + s
    i //= 26
  return 'qj' + s


def _sized(V):
  b = SPECIALS + _base()
  v = b + [_filler(i) for i in range(len(b), V)]
  ids = sorted({len(b), V - 1, V - 2, 0xEFFF, 0xF000, 0xF001, 0xFFFE, 0xFFFF, 0x7FFF, 0x8000} | set(range(1000, V, 997)))
  words = [v[i] for i in ids if len(b) <= i < V]
  words += [w + 'x' for w in words[:20]] + [_filler(V), _filler(V + 1)]
  return v, words


# ---- widths: an entry of every byte length the rendering tables hold ------------
# (tests/test_render_gpu.py; vinfo keeps a length in 8 bits and a pool offset,
# the pool is 4-aligned: every length 0..255 and every offset residue occurs)
WIDTHS_EMPTY = len(SPECIALS)  # the id of the empty line


def _widths():
  v = SPECIALS + ['']
  v += [_pat(n, 700 + n) for n in range(1, 256)]  # id 5 + n: n ASCII bytes, no period (a shifted offset shows)
  v += ['##' + _pat(253, 999)]                    # 255 bytes with its '##'
  v += ['ab' + CYR[0], 'abc' + HIRA[0], 'a' + GOTH[0]]  # ending in a 2-, 3- and 4-byte character
  v += [_pat(251, 998) + GOTH[1], HIRA[1] + CYR[1] * 124 + HIRA[2]]  # 255 bytes ending in 4; 254 of 3- and 2-byte ones
  return v, []


def widths_id(nbytes):
  """the id of widths' ASCII entry of nbytes bytes (0: the empty line)"""
  return WIDTHS_EMPTY + nbytes


def _build(name):
  if name == 'widths':
    return _widths()
  if name == 'collide':
    return _collide()
  if name in ('long_a', 'long_b'):
    return _long(name[-1])
  if name == 'ext':
    return _ext()
  if name == 'utf8':
    return _utf8()
  if name == 'sparse_a':
    return _sparse_a()
  if name == 'sparse_b':
    return _sparse_b()
  if name == 'tiny5':
    return list(SPECIALS), ['a', 'the']
  if name == 'tiny6':
    return SPECIALS + ['a'], ['a', 'aa', 'the']
  if name in ('tiny64', 'tiny65'):
    v = SPECIALS + list(LETTERS) + ['##' + c for c in LETTERS] + ['the', '.', ',', 'of', 'and', 'in', '##ing', '##ed'][:int(name[4:]) - 57]
    return v, ['the', 'cat', 'of', 'x.']
  if name.startswith('v'):
    return _sized(int(name[1:]))
  raise KeyError(name)


def vocab_bytes(name):
  if name in ('specials', 'specials_padlast'):
    return '\n'.join(_specials_lines(name == 'specials_padlast')).encode()  # no final newline
  if name == 'blanks':
    return ('\n'.join(SPECIALS + _base() + BLANK_LINES) + '\n').encode()
  if name == 'dupspecial':
    return ('\n'.join(_dupspecial_lines()) + '\n').encode()
  if name == 'crlf':
    return ('\r\n'.join(SPECIALS + _base() + ['crlfword', '##tail']) + '\r\n').encode()
  v, _ = _build(name)
  assert len(v) == len(set(v)), name
  return ('\n'.join(v) + '\n').encode()


def vocab_size(name):
  b = vocab_bytes(name)
  return b.count(b'\n') + (0 if b.endswith(b'\n') else 1)


def targeted_words(name):
  if name in ('specials', 'specials_padlast'):
    return list(SPECIALS_WORDS)
  if name == 'blanks':
    return list(BLANK_WORDS)
  if name == 'dupspecial':
    return list(DUPSPECIAL_WORDS)
  if name == 'crlf':
    return ['crlfword', 'crlfwordtail', 'atail', 'crlfword\r', 'tail']
  return _build(name)[1]


def targeted(name):
  """each targeted word alone, then three shuffles of them cut into sentences of 1..12 words"""
  words = targeted_words(name)
  rng = np.random.default_rng(len(name) * 1000 + len(words))
  out = list(words)
  for _ in range(3):
    order = rng.permutation(len(words))
    i = 0
    while i < len(order):
      k = int(rng.integers(1, 13))
      out.append(' '.join(words[j] for j in order[i:i + k]))
      i += k
  return out


_COMMON = None


def common_sentences():
  """about 300 sentences of synthetic wiki text and 200 adversarial ones"""
  global _COMMON
  if _COMMON is None:
    from lddl_amd import synth
    from test_tokenize_gpu import adversarial_sentences
    w = synth.make_wiki(40_000, seed=101)
    wiki = [w.sentence(i) for i in range(min(w.n_sent, 300))]
    adv = adversarial_sentences(np.random.default_rng(202), 200)
    _COMMON = wiki + adv
  return list(_COMMON)


def sentences(name):
  return targeted(name) + common_sentences()


_TMP = None


def vocab_path(name):
  """the committed file of a small vocabulary; a large one (or a small one
  not yet written out) goes to a temp dir once per process"""
  p = os.path.join(VOCAB_DIR, name + '.txt')
  if name in SMALL and os.path.exists(p):
    return p
  global _TMP
  if _TMP is None:
    _TMP = tempfile.TemporaryDirectory(prefix='synth_vocab_')
  p = os.path.join(_TMP.name, name + '.txt')
  if not os.path.exists(p):
    with open(p, 'wb') as f:
      f.write(vocab_bytes(name))
  return p


def load_golden(golden, name):
  """(data, sent_off, ids per sentence at 512, ntok) of tools/gen_golden_vocab.py:
  the vocabulary's targeted sentences followed by the common ones"""
  g, c = golden('tok_synth_%s.npz' % name), golden('tok_synth_common.npz')
  data = np.concatenate([g['data'], c['data']])
  off = np.concatenate([g['sent_off'], c['sent_off'][1:] + g['sent_off'][-1]]).astype(np.int64)
  ids = np.split(g['ids'].astype(np.int64), np.cumsum(g['ntok'])[:-1])
  return data, off, ids, g['ntok'].astype(np.int32)


def sentence_text(data, off, i):
  return bytes(data[off[i]:off[i + 1]]).decode('utf-8', 'replace')
