"""The split tokenizer where sentences are dense: many more sentences than
bytes / 32, so the scan's windows close after 31 sentences and their number
per tile is bounded by the sentence count, not by bytes.  Every window may be
listed for the serial path (fb_list); the list's capacity is fb_list_cap
(lddl_amd/csrc/tokenize.h), checked against a model of the windows on the CPU
in tests/test_fb_cap_host.py.  Here the same model (tests/window_model.py)
says which windows hold a sentence the scan does not model, and every dense
case asserts, before anything else, that its input lists more ranges in one
segment than the earlier capacity of 2 * seg + 64 held and no more than the
present one; then ntok and every id against the oracle, with the CSR
invariants (sparse_of_dense)."""
import numpy as np
import pytest
import torch

from oracle.oracle import OracleTokenizer, compact
from test_oracle_golden import VOCABS
from test_tokenize_gpu import sparse_of_dense
import window_model as wm

pytestmark = pytest.mark.gpu

# sentences the scan hands to the serial path, whatever the vocabulary:
LONG_WORD = 'q' * 60  # a word WordPiece has to split, longer than a record's 56 key bytes
RANKED = '᭄'     # BALINESE ADEG ADEG, 3 bytes: a spacing mark with a canonical reordering rank


def new_cap(seg, n_sent):
  """fb_list_cap of tokenize.h, in ranges (tests/test_fb_cap_host.py holds the header to the model)"""
  return 2 * seg + 64 + (n_sent + 30) // 31


class Case:
  """sentences as bytes + offsets, and the oracle's result per (vocab, max_tok), computed once"""

  def __init__(self, sents):
    from lddl_amd.synth import corpus_from_sentences
    c = corpus_from_sentences(sents, [0, len(sents)])
    self.data, self.sent_off, self.n_sent, self.nbytes = c.data, c.sent_off, len(sents), int(c.sent_off[-1])
    self.lens = np.diff(c.sent_off)
    self._oracle = {}

  def oracle(self, name, max_tok):
    if (name, max_tok) not in self._oracle:
      self._oracle[name, max_tok] = OracleTokenizer(VOCABS[name]).run(self.data, self.sent_off, max_tok, nthreads=8)
    return self._oracle[name, max_tok]

  def listed(self, seg, trigger_len):
    """windows per segment that hold a sentence of trigger_len bytes (the
    corpus' only sentences the scan does not model) or pass 2048 bytes.
    Device buffers are 16-B aligned and sent_off[0] is 0: base_align 0."""
    trig = np.concatenate([[0], np.cumsum(self.lens == trigger_len)]) if trigger_len else None
    out = []
    for ws in wm.windows(self.sent_off, seg):
      out.append(sum(1 for cs, ns in ws
                     if (trig is not None and trig[cs + ns] > trig[cs]) or wm.too_long(self.sent_off, cs, ns)))
    return out

  def seg_tiles(self, seg):
    return min(seg, wm.tile_count(self.nbytes))


def run_case(tok, case, max_tok=512):
  """lddl_tokenize over the case's real byte count (test_tokenize_gpu.run_hip
  counts its 16 pad bytes in), in the oracle's sparse layout"""
  d = torch.from_numpy(np.concatenate([case.data, np.zeros(16, np.uint8)])).cuda()
  o = torch.from_numpy(np.ascontiguousarray(case.sent_off)).cuda()
  ids, ntok, toff = tok.tokenize_device(d, o, max_tok, nbytes=case.nbytes)
  torch.cuda.synchronize()
  n = case.n_sent
  ntok = ntok.cpu().numpy()[:n]
  ids = ids.cpu().numpy().view(np.uint16)
  return sparse_of_dense(ids, ntok, toff.cpu().numpy()[:n + 1], case.sent_off, case.nbytes), ntok


def assert_oracle(tok, case, name, max_tok):
  ids, ntok = run_case(tok, case, max_tok)
  oids, ontok = case.oracle(name, max_tok)
  ontok = ontok[:case.n_sent]
  bad = np.flatnonzero(ntok != ontok)
  assert bad.size == 0, [(int(i), int(ntok[i]), int(ontok[i])) for i in bad[:5]]
  total = int(ntok.sum())
  idx = np.repeat(case.sent_off[:-1], ntok) + (np.arange(total) - np.repeat(np.cumsum(ntok) - ntok, ntok))
  if not np.array_equal(ids[idx].astype(np.int64), oids[idx].astype(np.int64)):
    got, exp = compact(ids, ntok, case.sent_off), compact(oids, ontok, case.sent_off)
    assert False, [i for i, (a, b) in enumerate(zip(got, exp)) if not np.array_equal(a, b)][:10]


def assert_listed(tok, case, seg, trigger_len, dense):
  """fallback_tiles of the last call = the model's listed windows (summed over
  the segments); dense: one segment lists more than the old capacity held,
  none more than the list holds"""
  per_seg = case.listed(seg, trigger_len)
  s = case.seg_tiles(seg)
  got = tok.stats()['fallback_tiles']
  print('seg %d: listed ranges %d, worst segment %d, old capacity %d, capacity %d' %
        (s, got, max(per_seg), wm.old_cap(s), new_cap(s, case.n_sent)))
  assert got == sum(per_seg)
  if dense:
    assert max(per_seg) > wm.old_cap(s)
    assert max(per_seg) <= new_cap(s, case.n_sent)


def dense_sentences(trigger, reps):
  return ([trigger] + [''] * 30) * reps


def padding(n):
  """a sentence of exactly n >= 1 bytes of one- and two-letter vocabulary words"""
  return ('a' if n % 2 else 'an') + ' a' * ((n - 1) // 2)


def plain_wiki_sentences(target_bytes, seed):
  """synthetic Wikipedia sentences the scan models whatever the window: ASCII, no word past 24 bytes"""
  from lddl_amd import synth
  c = synth.make_wiki(2 * target_bytes, seed=seed)
  out, n = [], 0
  for i in range(c.n_sent):
    s = c.sentence(i)
    if s.isascii() and s.isprintable() and all(len(w) <= 24 for w in s.split()) and 0 < len(s) < 1000:
      out.append(s)
      n += len(s)
      if n >= target_bytes:
        break
  return out


@pytest.fixture(scope='module')
def dense_long():
  return Case(dense_sentences(LONG_WORD, 2000))  # 117 KiB, 62 000 sentences, a listed window per 60 bytes


@pytest.fixture(scope='module')
def dense_ranked():
  return Case(dense_sentences(RANKED, 4000))  # 12 KiB, 124 000 sentences, a listed window per 3 bytes


def make_tok(monkeypatch, name, algo='5', timing=True, **env):
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', algo)
  monkeypatch.delenv('LDDL_SPLIT_SEG', raising=False)
  monkeypatch.delenv('LDDL_SPLIT_CHUNKS', raising=False)
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  tok = Tokenizer(VOCABS[name])
  if timing:
    tok.set_timing(True)
  return tok


@pytest.mark.parametrize('name', ['bert', 'codebert'])
def test_dense_fallbacks_one_segment(gpu, monkeypatch, dense_long, name):
  """a window per long word, about 17 a tile, all in one segment: seven times
  what 2 * seg + 64 held"""
  tok = make_tok(monkeypatch, name)
  for max_tok in (512, 3):
    assert_oracle(tok, dense_long, name, max_tok)
    assert_listed(tok, dense_long, 1 << 40, len(LONG_WORD), dense=True)


@pytest.mark.parametrize('algo', ['0'])
def test_dense_corpus_other_algorithms(gpu, monkeypatch, dense_long, algo):
  """the serial path (a range per tile at the most) over the same corpus: ids"""
  tok = make_tok(monkeypatch, 'bert', algo=algo, timing=False)
  for max_tok in (512, 3):
    assert_oracle(tok, dense_long, 'bert', max_tok)


@pytest.mark.parametrize('seg', [97, 61, 7, 1])
@pytest.mark.parametrize('name', ['bert', 'codebert'])
def test_dense_fallbacks_across_segment_seams(gpu, monkeypatch, dense_long, dense_ranked, name, seg):
  """segments of 97 and 61 tiles with the long word, of 7 and 1 tiles with the
  3-byte ranked mark (341 listed windows a tile: past the 64 of the old
  capacity's constant term)"""
  case, trig = (dense_long, LONG_WORD) if seg > 16 else (dense_ranked, RANKED)
  tok = make_tok(monkeypatch, name, LDDL_SPLIT_SEG=str(seg))
  for max_tok in (512, 3):
    assert_oracle(tok, case, name, max_tok)
    assert_listed(tok, case, seg, len(trig.encode()), dense=True)


def test_dense_fallbacks_with_record_capacity_fallbacks(gpu, monkeypatch, dense_long):
  """segments of 61 tiles and 3 record chunks: windows that run out of record
  slots are listed too, how many depends on the waves' timing -- ids only"""
  tok = make_tok(monkeypatch, 'bert', LDDL_SPLIT_SEG='61', LDDL_SPLIT_CHUNKS='3')
  for max_tok in (512, 3):
    assert_oracle(tok, dense_long, 'bert', max_tok)
    assert tok.stats()['fallback_tiles'] >= sum(dense_long.listed(61, len(LONG_WORD)))


@pytest.mark.parametrize('kind', ['empty', 'empty_two_a', 'one_byte'])
def test_sentence_density_without_fallbacks(gpu, monkeypatch, kind):
  """100 000 empty sentences and nothing else (no bytes at all), the same with
  an 'a' in the middle and at the end, 50 000 one-byte sentences: thousands of
  windows on one tile, none of them listed"""
  sents = {'empty': [''] * 100_000,
           'empty_two_a': [''] * 50_000 + ['a'] + [''] * 49_998 + ['a'],
           'one_byte': ['a', '.', 'b', ','] * 12_500}[kind]
  case = Case(sents)
  assert case.nbytes == {'empty': 0, 'empty_two_a': 2, 'one_byte': 50_000}[kind]
  assert sum(len(ws) for ws in wm.windows(case.sent_off, 1 << 40)) >= case.n_sent // 31
  tok = make_tok(monkeypatch, 'bert')
  assert_oracle(tok, case, 'bert', 512)
  assert_listed(tok, case, 1 << 40, 0, dense=False)
  assert tok.stats()['fallback_tiles'] == 0


@pytest.fixture(scope='module')
def runs_between_wiki():
  """plain Wikipedia sentences with runs of 5 000 empty sentences starting
  exactly on a tile (5), a super-tile (32) and, in segments of 16 tiles, a
  segment boundary (32, 48)"""
  src = plain_wiki_sentences(80 * 1024, seed=51)
  sents, n, k = [], 0, 0
  for t in (5, 32, 48):
    while n + len(src[k]) < t * 1024:
      sents.append(src[k])
      n += len(src[k])
      k += 1
    if n < t * 1024:
      sents.append(padding(t * 1024 - n))
      n = t * 1024
    sents += [''] * 5000
  sents += src[k:k + 60]
  case = Case(sents)
  for t in (5, 32, 48):
    s = int(np.searchsorted(case.sent_off[:-1], t * 1024))
    assert np.all(case.sent_off[s:s + 5001] == t * 1024)
  return case


@pytest.mark.parametrize('seg', [None, 16])
def test_runs_of_empty_sentences_on_boundaries(gpu, monkeypatch, runs_between_wiki, seg):
  env = {} if seg is None else {'LDDL_SPLIT_SEG': str(seg)}
  tok = make_tok(monkeypatch, 'bert', **env)
  assert_oracle(tok, runs_between_wiki, 'bert', 512)
  assert_listed(tok, runs_between_wiki, seg or (1 << 40), 0, dense=False)
  assert tok.stats()['fallback_tiles'] == 0


def test_fallback_list_regrows_with_the_sentence_count(gpu, monkeypatch):
  """one Tokenizer: a Wikipedia corpus, the dense corpus of the same byte
  count (the same tiles and segment, 40 times the sentences: the list has to
  grow with n_sent alone), the Wikipedia corpus again"""
  from lddl_amd import synth
  w = synth.make_wiki(128 * 1024, seed=53)
  wiki = Case([w.sentence(i) for i in range(w.n_sent)])
  reps = wiki.nbytes // len(LONG_WORD)
  rest = wiki.nbytes - reps * len(LONG_WORD)
  dense = Case(dense_sentences(LONG_WORD, reps) + ([padding(rest)] if rest else []))
  assert dense.nbytes == wiki.nbytes and dense.n_sent > 30 * wiki.n_sent
  tok = make_tok(monkeypatch, 'bert')
  assert_oracle(tok, wiki, 'bert', 512)
  few = tok.stats()['fallback_tiles']
  assert few <= wm.old_cap(wiki.seg_tiles(1 << 40))
  assert_oracle(tok, dense, 'bert', 512)
  assert_listed(tok, dense, 1 << 40, len(LONG_WORD), dense=True)
  assert_oracle(tok, wiki, 'bert', 512)
  assert tok.stats()['fallback_tiles'] == few
