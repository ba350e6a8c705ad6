"""The preconditions of tests/test_tok_contract_gpu.py, on any machine: the
builders of tests/tok_contract.py produce what the GPU tests rely on, by the
oracle and the window model alone, so that no GPU case is vacuous."""
import numpy as np
import pytest

import tok_contract as tc
import window_model as wm
from oracle.oracle import OracleTokenizer, compact
from test_oracle_golden import VOCABS


@pytest.fixture(scope='module')
def ot():
  return OracleTokenizer(VOCABS['bert'])


@pytest.fixture(scope='module')
def base_oracle(ot):
  c = tc.base_corpus()
  return ot.run(c.data, c.sent_off, 512, nthreads=8)


def test_base_corpus_shape(ot):
  c = tc.base_corpus()
  assert wm.tile_count(c.nbytes) >= 40 and c.nbytes < 80 * 1024
  lens = np.diff(c.sent_off)
  assert c.n_adv >= 100 and (lens == 0).sum() >= 140
  assert sorted(int(lens[s]) for s in c.edge) == list(range(2033, 2049))
  assert (lens > 2048).sum() == 2
  assert sum(1 for s in c.sents if tc.LONG_WORD in ot.words(s)) == 3 and c.trigger.sum() >= 6
  assert all(c.sents[s].isascii() for s in c.edge)
  # words of 5 to 30 pieces that stay within a 56-byte record
  words = [tc.PIECE_WORD] + tc.PIECE_WORDS
  assert all(w in ' '.join(c.sents[c.piece_sent - 2:c.piece_sent + 1]).split() for w in words)
  for w in words:
    data = np.frombuffer(w.encode(), np.uint8)
    _, n = ot.run(data, np.array([0, len(data)]), 512)
    assert len(w) <= 56 and 5 <= n[0] <= 30, (w, n[0])


def test_placement_layout():
  c = tc.base_corpus()
  for m, B in ((0, 0), (4, 1), (12, 2053)):
    p = tc.placed(c, m, B)
    at = p.view0 + B
    assert at == tc.MARGIN + m + B and p.nbytes == c.nbytes
    assert np.array_equal(p.buf[at:at + c.nbytes], c.data[:c.nbytes])
    assert not p.buf[at + c.nbytes:at + c.nbytes + 16].any()
    assert len(p.buf) == at + c.nbytes + 16 + tc.MARGIN
    assert p.sent_off[0] == B and np.array_equal(p.sent_off - B, c.sent_off)
    assert p.nbytes >= p.sent_off[-1] - p.sent_off[0]


def test_filler_is_text_wherever_a_read_starts(ot):
  """valid UTF-8 as a whole, ASCII within 4 KiB of the corpus (a read that
  starts up to B + 2048 bytes early, or ends that much late, starts on a character), and it tokenizes
  to something, with multi-byte characters and a [SEP]"""
  for m, B in ((0, 0), (12, 2053)):
    p = tc.placed(tc.base_corpus(), m, B)
    assert len(p.front) == tc.MARGIN + m + B and len(p.back) == tc.MARGIN
    for part, near in ((p.front, p.front[-tc.ASCII_ZONE:]), (p.back, p.back[:tc.ASCII_ZONE])):
      text = part.decode('utf-8')  # strict
      assert near.isascii() and max(tc.B_VALUES) + wm.CAP <= tc.ASCII_ZONE
      assert any(len(ch.encode()) == 2 for ch in text) and any(len(ch.encode()) == 3 for ch in text)
      assert '[SEP]' in text and ' ' in text
      data = np.frombuffer(part, np.uint8)
      ids, n = ot.run(data, np.array([0, 1000, len(data)]), 512)
      assert n[0] > 100 and n[1] == 512 and len(set(ids[:1000].tolist())) > 8


def test_windows_move_with_the_placement():
  """the window model differs between (m, B) settings at every segment size,
  and the too-long windows among the 2033 .. 2048 byte sentences take at least
  three values over the sweep: the sweep moves windows"""
  c = tc.base_corpus()
  for seg in (1 << 40, 16, 7):
    seen = {}
    for m in tc.M_VALUES:
      for B in tc.B_VALUES:
        ws = wm.windows(c.sent_off + B, seg, base_align=m)
        seen.setdefault(((m + B) & 15), []).append(ws)
    assert len(seen) >= 8
    distinct = {repr(v[0]) for v in seen.values()}
    assert len(distinct) >= 4, seg
    # the same alignment gives the same windows: the model depends on (m + B) & 15 and the rebased offsets alone
    for v in seen.values():
      assert all(x == v[0] for x in v)
  counts = {(m, B): tc.edge_too_long(c, c.sent_off + B, m) for m in tc.M_VALUES for B in tc.B_VALUES}
  assert len(set(counts.values())) >= 3, counts
  totals = {sum(tc.listed(c, c.sent_off + B, 1 << 40, m)) for m in tc.M_VALUES for B in tc.B_VALUES}
  assert len(totals) >= 3
  # a scan that took aoff from the offset alone (base_align 0) would list another number of windows
  # at every m != 0: the GPU test's count equality tells the two apart
  for m in tc.M_VALUES[1:]:
    for seg in (1 << 40, 16, 1):
      assert any(sum(tc.listed(c, c.sent_off + B, seg, m)) != sum(tc.listed(c, c.sent_off + B, seg, 0))
                 for B in tc.B_VALUES), (m, seg)


def test_triggers_are_what_the_model_lists(ot):
  c = tc.base_corpus()
  for s in np.flatnonzero(c.trigger):
    assert tc.RANKED in c.sents[s] or tc.LONG_WORD in c.sents[s] or any(
        56 < nb and nc <= 100 for nb, nc in tc.word_bytes(ot, c.sents[s]))
  # every sentence is one the model predicts: no character that expands or carries a rank but the ranked mark
  assert all(tc.predictable(s.replace(tc.RANKED, '')) for s in c.sents)
  assert c.trigger[c.serial_sent] and not c.trigger[c.piece_sent] and not c.trigger[c.mid]


def test_cut_points_lie_where_their_names_say(ot, base_oracle):
  c = tc.base_corpus()
  oids, ontok = base_oracle
  cuts = tc.cut_points(oids, ontok)
  off = np.concatenate([[0], np.cumsum(ontok)])
  T = int(off[-1])
  assert (cuts['zero'], cuts['one'], cuts['T-1'], cuts['T'], cuts['T+1']) == (0, 1, T - 1, T, T + 1)
  assert len(set(cuts.values())) == len(cuts) and all(0 <= v <= T + 1 for v in cuts.values())
  # a sentence in the middle, of several tokens
  s = c.mid
  assert ontok[s] >= 4 and T // 4 < off[s] < 3 * T // 4
  assert cuts['mid_first_out'] == off[s] and cuts['mid_first_in'] == off[s] + 1
  assert cuts['mid_last_out'] == off[s + 1] - 1 and cuts['mid_last_in'] == off[s + 1]
  # the piece word: the oracle on the word alone, then its place in the sentence
  w = np.frombuffer(tc.PIECE_WORD.encode(), np.uint8)
  wids, wn = ot.run(w, np.array([0, len(w)]), 512)
  k = int(wn[0])
  assert k >= 6 and len(w) <= 56
  sent = compact(oids, ontok, c.sent_off)[c.piece_sent]
  assert len(sent) == k + 2 and np.array_equal(sent[1:1 + k], wids[:k])
  for j in (1, 3, 4, 5):
    cap = cuts['piece_%d' % j]
    assert cap - off[c.piece_sent] - 1 == j < k
  # the piece sentence runs on the window path, the serial one is listed, at every placement
  for m in tc.M_VALUES:
    for B in (0, 1, 1025):
      so = c.sent_off + B
      win = {s2: (cs, ns) for ws in wm.windows(so, 1 << 40, m) for cs, ns in ws for s2 in range(cs, cs + ns)}
      cs, ns = win[c.piece_sent]
      assert not c.trigger[cs:cs + ns].any() and not wm.too_long(so, cs, ns, m)
      cs, ns = win[c.serial_sent]
      assert c.trigger[cs:cs + ns].any()
  q = c.serial_sent
  assert off[q] < cuts['serial'] < off[q + 1]


def test_long_corpus_counts(ot):
  """the oracle takes every max_tok of the range; at 65534 the corpus holds
  sentences of more than 512 and more than 2048 tokens, and one whose 70 000
  tokens are cut at 65534 (a count cannot pass max_tok)"""
  c = tc.long_corpus()
  lens = np.diff(c.sent_off)
  assert lens[c.window_2040] == 2040 and lens[c.window_1000] == 2000 and lens[c.pieces] <= 1500
  assert lens[c.serial_3000] > 2048 and lens[c.serial_70000] == 70000
  # the first sentence starts 16-byte aligned: it fits one window
  assert c.sent_off[c.window_2040] % 16 == 0 and not wm.too_long(c.sent_off, 0, 1)
  oids, n = ot.run(c.data, c.sent_off, 65534, nthreads=4)
  assert n[c.window_2040] == 2040 and n[c.window_1000] == 1000 and n[c.serial_3000] == 3000
  assert n[c.serial_70000] == 65534 and n[c.pieces] > 100
  assert (n > 512).sum() >= 4 and (n > 2048).sum() >= 2
  dot = ot.run(np.frombuffer(b'.', np.uint8), np.array([0, 1]), 512)[0][0]
  at = int(c.sent_off[c.serial_70000])
  assert (oids[at:at + 65534] == dot).all()
  whole = compact(oids, n, c.sent_off)
  for max_tok in (1, 2, 4, 5, 511, 512, 513, 2047, 2048):
    ids, k = ot.run(c.data, c.sent_off, max_tok, nthreads=4)
    assert np.array_equal(k, np.minimum(n, max_tok))
    for a, b in zip(compact(ids, k, c.sent_off), whole):
      assert np.array_equal(a, b[:max_tok])


def test_pack_corpus_shape(ot):
  c, pdo = tc.pack_corpus()
  assert c.n_doc == 60 and len(pdo) == 4 and pdo[-1] == c.n_doc
  _, n = ot.run(c.data, c.sent_off, 512, nthreads=4)
  lens = np.diff(c.sent_off)
  first = c.doc_sent_off[:-1]
  assert lens[first[5]] == 0
  assert lens[first[17]] > 0 and n[first[17]] == 0
  assert c.doc_nseg_doc[29] == 0 and c.doc_nseg_doc[5] > 0
  assert n[first[30]:first[31]].sum() == 0
  assert n.max() < 60  # a docstring line taken whole stays below seq - 3: no error exit of the CodeBERT packer
