"""Shared builders of tests/test_tok_contract_host.py and
tests/test_tok_contract_gpu.py: what include/lddl_amd.h promises about
lddl_tokenize and the pack calls, put in front of the kernels.

  placed        a corpus that does not start at offset 0 of a buffer that is
                only 4-byte aligned, with text-like filler around it
  Guarded       an output buffer inside sentinel guards
  base_corpus   about 60 KiB (60 tiles, four super-tiles) whose listed windows
                tests/window_model.py predicts at every placement
  cut_points    the out_cap values of the truncation test
  long_corpus   sentences of more tokens than 512, 2048 and 65534
  pack_corpus   documents for the packers on un-rebased offsets

No GPU is needed to build any of them (Guarded allocates where it is told)."""
import functools
import types

import numpy as np

import window_model as wm

MARGIN = 64 * 1024
ASCII_ZONE = 6144     # filler this close to the corpus is ASCII: a read that starts up to 6 KiB early starts on a character
PAD = 16              # zero bytes behind a corpus (every test appends them)
GUARD_BYTES = 64 * 1024
IDS_SENTINEL = 0xA5A5
NTOK_SENTINEL = 0x5A5A5A5A
TOFF_SENTINEL = 0x5A5A5A5A5A5A5A5A

LONG_WORD = 'q' * 60  # a word WordPiece has to split, longer than a record's 56 key bytes
RANKED = '᭄'     # BALINESE ADEG ADEG: a spacing mark with a canonical reordering rank
PIECE_WORD = 'pneumonoultramicroscopicsilicovolcanoconiosis'  # 45 bytes, 17 pieces (BERT): a record and its extension slot
# words of 6 to 21 pieces under either vocabulary, none longer than a record's 56 key bytes
PIECE_WORDS = ['electroencephalographically', 'antidisestablishmentarianism', 'supercalifragilisticexpialidocious',
               'hippopotomonstrosesquippedaliophobia', 'thermoluminescencespectrophotometricallyunquestionable',
               'interconnectednessmisunderstandingsoverwhelmingly', 'zqxjvkwyzqxjvkwyzqxjvkwy', 'zqxjvkzqxjvkzqxjvk']
M_VALUES = (0, 4, 8, 12)
B_VALUES = (0, 1, 3, 15, 16, 17, 1023, 1024, 1025, 2053)
# characters of the adversarial atoms that neither expand under the normaliser
# nor carry a reordering rank: with them a window is listed only for its length
# or for a word that does not fit a record (see triggers)
SAFE_CHARS = set('ïé中文😀ﬁ')


# ---------------------------------------------------------------- filler --
def filler(n, ascii_head=0, ascii_tail=0):
  """exactly n bytes of text that tokenizes to something: ASCII words and
  spaces, a [SEP], and (outside the first ascii_head and last ascii_tail
  bytes) a few 2- and 3-byte characters; valid UTF-8 as a whole"""
  plain = b'the quick brown fox [SEP] jumps over a lazy dog, twice. '
  mixed = 'naïve café 中文 [SEP] and so on. '.encode()
  out = bytearray()
  k = 0
  while len(out) < n:
    room = n - len(out)
    in_ascii = len(out) < ascii_head or room <= ascii_tail + len(mixed)
    piece = plain if in_ascii or k % 3 else mixed
    k += 1
    out += piece if len(piece) <= room else b'x' * room
  return bytes(out)


def placed(corpus, m, B, margin=MARGIN):
  """corpus (bytes at data[sent_off[0] : sent_off[-1]]) inside filler:
    buf       filler[margin + m + B] | corpus | 16 zero bytes | filler[margin]
    view0     margin + m: the device view is buf[view0:], m past a 16-byte boundary
              when buf itself is 16-byte aligned (margin is a multiple of 16)
    sent_off  the corpus' offsets rebased to 0, plus B (absolute in the view)
  A wrong offset of up to B bytes then reads filler, not another allocation."""
  assert margin % 16 == 0 and m % 4 == 0 and 0 <= m < 16 and B >= 0
  so = np.asarray(corpus.sent_off, dtype=np.int64)
  nbytes = int(so[-1] - so[0])
  text = np.asarray(corpus.data[int(so[0]):int(so[-1])], dtype=np.uint8).tobytes()
  front = filler(margin + m + B, ascii_tail=ASCII_ZONE)
  back = filler(margin, ascii_head=ASCII_ZONE)
  buf = np.frombuffer(front + text + b'\0' * PAD + back, dtype=np.uint8).copy()
  return types.SimpleNamespace(buf=buf, view0=margin + m, m=m, B=B, margin=margin, nbytes=nbytes,
                               sent_off=so - so[0] + B, n_sent=len(so) - 1, front=front, back=back)


def device_view(p, device):
  """(whole buffer, the 4-byte aligned view the call gets, sent_off) on the device"""
  import torch
  whole = torch.from_numpy(p.buf).to(device)
  assert whole.data_ptr() % 16 == 0
  view = whole[p.view0:]
  assert view.data_ptr() % 16 == p.m
  return whole, view, torch.from_numpy(np.ascontiguousarray(p.sent_off)).to(device)


class Guarded:
  """n entries of dtype inside two guards of at least 64 KiB, all pre-filled
  with a sentinel; .view is what a call writes (16-byte aligned)"""

  def __init__(self, n, dtype, sentinel, device):
    import torch
    size = torch.empty(0, dtype=dtype).element_size()
    self.g = GUARD_BYTES // size
    self.n = n
    self.sentinel = int(np.array([sentinel], dtype=np.uint64).astype({2: np.uint16, 4: np.uint32, 8: np.uint64}[size])
                        .view({2: np.int16, 4: np.int32, 8: np.int64}[size])[0])
    self.full = torch.full((2 * self.g + n,), self.sentinel, dtype=dtype, device=device)
    self.view = self.full[self.g:self.g + n]
    assert self.view.data_ptr() % 16 == 0

  def refill(self):
    self.full.fill_(self.sentinel)

  def host(self):
    return self.full.cpu().numpy()

  def check(self, written, what):
    """the guards and view[written:] still hold the sentinel -> the written part (host)"""
    h = self.host()
    for name, part in (('front guard', h[:self.g]), ('back guard', h[self.g + self.n:]),
                       ('entries past the written ones', h[self.g + written:self.g + self.n])):
      bad = np.flatnonzero(part != self.sentinel)
      assert bad.size == 0, '%s: %s trampled at %s' % (what, name, bad[:8].tolist())
    return h[self.g:self.g + written]


# --------------------------------------------------------------- corpora --
class TextCorpus:
  """sentences as bytes + offsets (rebased), with the marks the tests use"""

  def __init__(self, sents, **marks):
    from lddl_amd.synth import corpus_from_sentences
    c = corpus_from_sentences(sents, [0, len(sents)])
    self.sents = sents
    self.data, self.sent_off, self.n_sent, self.nbytes = c.data, c.sent_off, len(sents), int(c.sent_off[-1])
    self.__dict__.update(marks)


def word_bytes(oracle, s):
  """(bytes, characters) of every pre-tokenised, normalised word of s"""
  return [(len(w.encode()), len(w)) for w in oracle.words(s)]


def triggers(oracle, s):
  """the scan lists the window of sentence s whatever the vocabulary: it holds
  the ranked mark, or a word of more than 56 bytes (a record's key) that is
  not [UNK] for its length (more than 100 characters)"""
  return RANKED in s or any(nb > 56 and nc <= 100 for nb, nc in word_bytes(oracle, s))


def predictable(s):
  return all(ord(ch) < 128 or ch in SAFE_CHARS for ch in s)


def edge_sentence(n, k):
  """n ASCII bytes of short vocabulary words"""
  words = ['the', 'of', 'and', 'window', 'edge', 'a', 'is', 'river', 'on']
  out = ''
  i = k
  while len(out) < n:
    out += words[i % len(words)] + ' '
    i += 1
  out = out[:n]
  return out[:-1] + 'a' if out.endswith(' ') else out


@functools.lru_cache(maxsize=None)
def base_corpus():
  """See the module docstring.  Marks: .trigger (bool per sentence: its window
  is listed), .edge (the 16 sentences of 2033 .. 2048 bytes), .piece_sent (a
  sentence 'the PIECE_WORD is'), .serial_sent (a sentence with LONG_WORD), .mid
  (an ordinary sentence in the middle)."""
  from oracle.oracle import OracleTokenizer
  from test_oracle_golden import VOCABS
  from test_tokenize_dense_gpu import plain_wiki_sentences
  from test_tokenize_gpu import adversarial_sentences
  ot = OracleTokenizer(VOCABS['bert'])
  wiki = plain_wiki_sentences(14 * 1024, seed=61)
  # adversarial sentences the window model can predict (no fuzz string, no
  # atom that expands or carries a rank): a few hundred, about 10 KiB
  adv, n = [], 0
  for s in adversarial_sentences(np.random.default_rng(62), 6000):
    if predictable(s) and len(s.encode()) <= 1200:
      adv.append(s)
      n += len(s.encode())
      if len(adv) >= 400 or n >= 10 * 1024:
        break
  pieces = ['%s is %s and %s' % tuple(PIECE_WORDS[:3]), ' '.join(PIECE_WORDS[3:]), 'the %s is' % PIECE_WORD]
  longs = ['a b c %s d e f' % LONG_WORD, LONG_WORD, 'word, %s.' % LONG_WORD]
  ranked = ['a%sb' % RANKED, RANKED, 'the %s mark' % RANKED]
  edge = [edge_sentence(2033 + k, k) for k in range(16)]
  over = [edge_sentence(2500, 3), edge_sentence(3100, 5)]
  # (an empty and a short sentence behind each edge sentence join its window exactly when it fits)
  tail = lambda es: [x for e in es for x in (e, '', 'so on')]  # noqa: E731
  w = len(wiki)
  sents = (wiki[:w // 4] + [''] * 40 + adv[:len(adv) // 2] + pieces + tail(edge[:8]) + [''] * 3 + wiki[w // 4:w // 2] +
           longs[:2] + [over[0]] + ranked[:2] + [''] * 70 + adv[len(adv) // 2:] + tail(edge[8:]) + wiki[w // 2:3 * w // 4] +
           [over[1], longs[2], ranked[2]] + [''] * 33 + wiki[3 * w // 4:])
  trig = np.array([triggers(ot, s) for s in sents], dtype=bool)
  return TextCorpus(sents, trigger=trig, edge=[sents.index(e) for e in edge], piece_sent=sents.index(pieces[2]),
                    serial_sent=sents.index(longs[0]), mid=sents.index(wiki[w // 4 + 5]), n_adv=len(adv))


def listed(case, sent_off, seg, base_align):
  """listed windows per segment of a call over sent_off (absolute offsets of
  case's sentences) into a buffer base_align past a 16-byte boundary: the
  windows that pass 2048 bytes and those holding a trigger sentence
  (test_tokenize_dense_gpu.Case.listed with base_align and absolute offsets)"""
  trig = np.concatenate([[0], np.cumsum(case.trigger)])
  return [sum(1 for cs, ns in ws if trig[cs + ns] > trig[cs] or wm.too_long(sent_off, cs, ns, base_align))
          for ws in wm.windows(sent_off, seg, base_align)]


def edge_too_long(case, sent_off, base_align):
  """how many of the 2033 .. 2048 byte sentences open a window that passes 2048 bytes"""
  first = {cs: ns for ws in wm.windows(sent_off, 1 << 40, base_align) for cs, ns in ws}
  return sum(1 for s in case.edge if s in first and wm.too_long(sent_off, s, first[s], base_align))


def cut_points(oids, ontok, case=None):
  """{name: out_cap} for a corpus whose oracle result is (oids, ontok); T is
  its total.  piece_k: exactly k pieces of PIECE_WORD lie below the cut (four
  live in a record's 16-byte head, the rest in its pieces buffer)."""
  case = case or base_corpus()
  off = np.concatenate([[0], np.cumsum(ontok)]).astype(np.int64)
  T = int(off[-1])
  s, p, q = case.mid, case.piece_sent, case.serial_sent
  out = {'zero': 0, 'one': 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1,
         'mid_first_out': int(off[s]), 'mid_first_in': int(off[s]) + 1,
         'mid_last_out': int(off[s + 1]) - 1, 'mid_last_in': int(off[s + 1]),
         'serial': int(off[q]) + int(ontok[q]) // 2}
  for k in (1, 3, 4, 5):
    out['piece_%d' % k] = int(off[p]) + 1 + k  # ('the' is one token)
  return out


@functools.lru_cache(maxsize=None)
def long_corpus():
  """sentences of more tokens than the tests' max_tok values: window path
  (under 2 KiB), serial path, and one past the 16-bit edge"""
  rng = np.random.default_rng(64)
  letters = 'zqxjvkwy'
  words, n = [], 0
  while n < 1500:
    k = int(rng.integers(12, 50))
    words.append(''.join(letters[int(x)] for x in rng.integers(0, len(letters), k)))
    n += k + 1
  many_pieces = ' '.join(words)[:1500].rstrip()
  sents = ['!' * 2040, 'A short one.', '', '! ' * 1000, '', many_pieces, 'a b', 'hello ' * 3000, '',
           '.' * 70000, 'The end.', '']
  return TextCorpus(sents, window_2040=0, window_1000=3, pieces=5, serial_3000=7, serial_70000=9)


@functools.lru_cache(maxsize=None)
def pack_corpus():
  """about 60 documents in three partitions for the packers: prose of short
  sentences; document 5 starts with an empty sentence, document 17 with a
  whitespace-only one (bytes, no tokens), document 29 has no docstring
  segments, document 30 only empty sentences.  doc_nseg_doc is read by the
  CodeBERT packer alone."""
  from lddl_amd.synth import corpus_from_sentences
  from test_tokenize_dense_gpu import plain_wiki_sentences
  src = [s for s in plain_wiki_sentences(120 * 1024, seed=65) if len(s) < 160]
  rng = np.random.default_rng(66)
  sents, dso, nseg, k = [], [0], [], 0
  for d in range(60):
    n = int(rng.integers(2, 9))
    doc = src[k:k + n]
    k += n
    nd = int(rng.integers(0, 3))
    if d == 5:
      doc = [''] + doc
      nd = 2
    elif d == 17:
      doc = ['  \t '] + doc
      nd = 1
    elif d == 29:
      nd = 0
    elif d == 30:
      doc = ['', '']
      nd = 1
    elif d % 11 == 3:
      doc = doc[:2] + [''] + doc[2:]
    sents += doc
    dso.append(len(sents))
    nseg.append(min(nd, len(doc) - 1))
  c = corpus_from_sentences(sents, dso, np.array(nseg, dtype=np.int32))
  assert k <= len(src)
  return c, np.array([0, 19, 41, 60], dtype=np.int64)
