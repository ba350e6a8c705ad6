"""HIP tokenizer over the synthetic vocabularies of tests/synth_vocab.py (bucket
overflow, keys past 24 bytes, the extension chain, multi-byte keys at the
24-byte edge, sparse vocabularies, specials at odd ids, vocab-line parsing,
the size edges 61440 / 61441 / 65535 / 65536) vs HF tokenizers 0.22.2
(tools/gen_golden_vocab.py) and vs the oracle, sentence by sentence."""
import numpy as np
import pytest

import synth_vocab as sv
from oracle.oracle import OracleTokenizer, compact
from test_tokenize_gpu import run_hip

pytestmark = pytest.mark.gpu


def check(tok, data, off, exp, gtok, max_tok, oracle=None):
  """ids and counts of one call equal exp (per-sentence ids at 512) cut to max_tok, and the oracle's"""
  ids, ntok = run_hip(tok, data, off, max_tok)
  got = compact(ids, ntok, off)
  ref = [e[:max_tok] for e in exp]
  if oracle is not None:
    oids, ontok = oracle.run(data, off, max_tok, nthreads=4)
    orc = compact(oids, ontok, off)
    bad = [i for i in range(len(ref)) if not np.array_equal(ref[i], orc[i])]
    assert not bad, ('oracle vs HF', [(i, sv.sentence_text(data, off, i)[:80]) for i in bad[:5]])
  bad = [i for i in range(len(ref)) if ntok[i] != len(ref[i]) or not np.array_equal(ref[i], got[i].astype(np.int64))]
  assert not bad, [(i, sv.sentence_text(data, off, i)[:80], ref[i][:10].tolist(), got[i][:10].tolist(), int(ntok[i]))
                   for i in bad[:5]]


@pytest.mark.parametrize('algo', ['5', '0'])
@pytest.mark.parametrize('name', sv.NAMES)
def test_synthetic_vocab_matches_hf_and_oracle(gpu, golden, monkeypatch, name, algo):
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', algo)
  data, off, exp, gtok = sv.load_golden(golden, name)
  tok = Tokenizer(sv.vocab_path(name))
  assert tok.vocab_size == sv.vocab_size(name)
  orc = OracleTokenizer(sv.vocab_path(name))
  for max_tok in (512, 3):
    check(tok, data, off, exp, gtok, max_tok, orc)


@pytest.mark.parametrize('env', [{'LDDL_SPLIT_SEG': '1'}, {'LDDL_SPLIT_SEG': '7'}, {'LDDL_SPLIT_CHUNKS': '3'}])
@pytest.mark.parametrize('name', ['collide', 'long_a', 'long_b', 'utf8'])
def test_synthetic_vocab_segments_and_capacity(gpu, golden, monkeypatch, name, env):
  """one-tile and seven-tile segments (seams) and too few record chunks (tiles
  go to the serial path, which then sees the colliding / long / multi-byte keys)"""
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', '5')
  for k, v in env.items():
    monkeypatch.setenv(k, v)
  data, off, exp, gtok = sv.load_golden(golden, name)
  tok = Tokenizer(sv.vocab_path(name))
  for max_tok in (512, 3):
    check(tok, data, off, exp, gtok, max_tok)


@pytest.mark.parametrize('name', ['collide', 'long_a'])
def test_two_corpora_one_tokenizer(gpu, golden, monkeypatch, name):
  """one Tokenizer, two different corpora of one vocabulary, then the first
  again: no record, piece count or extension slot of an earlier call shows"""
  from lddl_amd.synth import corpus_from_sentences
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', '5')
  data, off, exp, gtok = sv.load_golden(golden, name)
  n = len(exp)
  order = np.random.default_rng(5).permutation(n)
  sents = [sv.sentence_text(data, off, i) for i in order if i % 3]
  c = corpus_from_sentences(sents, [0, len(sents)])
  exp2 = [exp[i] for i in order if i % 3]
  tok = Tokenizer(sv.vocab_path(name))
  check(tok, data, off, exp, gtok, 512)
  check(tok, c.data, c.sent_off, exp2, None, 512)
  check(tok, data, off, exp, gtok, 512)
  check(tok, c.data, c.sent_off, exp2, None, 3)


def stats_of(tok, sents):
  """tok.stats() of one call over sents, whose ids equal the oracle's"""
  from lddl_amd.synth import corpus_from_sentences
  c = corpus_from_sentences(sents, [0, len(sents)])
  oids, ontok = OracleTokenizer(tok.vocab_file).run(c.data, c.sent_off, 512)
  exp = [x.astype(np.int64) for x in compact(oids, ontok, c.sent_off)]
  tok.set_timing(True)  # (stats() reads the call's counters with its events)
  check(tok, c.data, c.sent_off, exp, None, 512)
  return tok.stats()


def test_paths_reached(gpu, monkeypatch):
  """tok.stats() of the split tokenizer over the targeted sentences alone (the
  common ones hold words of 100+ bytes and thousands of multi-piece words of
  their own).  'long': the words of 57+ bytes put windows on the fallback
  list, the same sentences without them put none.  'collide': every
  occurrence of a whole word displaced from slot 0 of its home bucket runs as
  a WordPiece record -- the same text with each displaced word replaced by
  its group's first member (found in slot 0 by the scan, when it is of <= 24
  bytes) runs exactly that many fewer."""
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.setenv('LDDL_TOKENIZE_ALGO', '5')
  for name in ('long_a', 'long_b'):
    tok = Tokenizer(sv.vocab_path(name))
    assert tok.set_algo(5) == 5
    sents = sv.targeted(name)
    short = [' '.join(w for w in s.split(' ') if len(w.encode()) <= 56) for s in sents]
    short = [s for s in short if s]
    assert any(len(w.encode()) >= 57 for s in sents for w in s.split(' ')) and short != sents
    assert stats_of(tok, sents)['fallback_tiles'] > 0
    assert stats_of(tok, short)['fallback_tiles'] == 0
  first = {m: members[0] for cont, members, _ in sv._collide_groups() if not cont for m in members[1:]}
  assert set(first) == set(sv.collide_displaced_words())
  sents = sv.targeted('collide')
  occ = sum(1 for s in sents for w in s.split(' ') if w in first)
  assert occ >= 4 * len(first) >= 32
  tok = Tokenizer(sv.vocab_path('collide'))
  assert tok.set_algo(5) == 5
  rec = stats_of(tok, sents)['records']
  rec0 = stats_of(tok, [' '.join(first.get(w, w) for w in s.split(' ')) for s in sents])['records']
  # (a word past 24 bytes is a record wherever its key sits: the scan probes whole words of <= 24 bytes only)
  occ24 = sum(1 for s in sents for w in s.split(' ') if w in first and len(w) <= 24)
  assert occ - occ24 == 4 * 5 and rec >= occ and rec - rec0 == occ24, (rec, rec0, occ, occ24)


def test_size_edges(gpu, golden, monkeypatch):
  """V = 61440 (SPLIT_EDEF) still runs the split tokenizer, V = 61441 only the
  serial path; at V = 65536 the id 65535 (the split tokenizer's 'empty unit'
  entry value) comes back where HF has it"""
  from lddl_amd.tokenizer import Tokenizer
  monkeypatch.delenv('LDDL_TOKENIZE_ALGO', raising=False)
  for v, algo in ((61440, 5), (61441, 0), (65536, 0)):
    name = 'v%d' % v
    tok = Tokenizer(sv.vocab_path(name))
    assert tok.set_algo(5) == algo, v
    data, off, exp, gtok = sv.load_golden(golden, name)
    check(tok, data, off, exp, gtok, 512)
    ids, ntok = run_hip(tok, data, off, 512)
    flat = np.concatenate(compact(ids, ntok, off)).astype(np.int64)
    for i in [i for i in (v - 1, 0xEFFF, 0xF000, 0xFFFF) if i < v]:
      assert (flat == i).sum() == (np.concatenate(exp) == i).sum() > 0, (v, i)


@pytest.mark.parametrize('name', sv.LINE_VOCABS)
def test_tokenize_and_convert_round_trip(gpu, name):
  """Tokenizer.tokenize / convert_tokens_to_ids with specials at odd ids, a
  duplicate line (its last id), trimmed lines: the strings are the
  vocabulary's and convert back to the ids encode_batch gives"""
  import json
  import os
  from conftest import GOLDEN
  from lddl_amd.tokenizer import Tokenizer
  both = json.load(open(os.path.join(GOLDEN, 'vocab_lines_hf.json')))
  hf = both[name]
  tok = Tokenizer(sv.vocab_path(name))
  assert [tok.pad_id, tok.unk_id, tok.cls_id, tok.sep_id, tok.mask_id] == both[name + ':special_ids']
  n = sv.vocab_size(name)
  assert tok.vocab == hf  # token -> id: duplicates at their last id, lines trimmed as HF trims them
  if name == 'specials':
    assert (tok.unk_id, tok.pad_id, tok.mask_id) == (0, n - 2, n - 1) and 0 < tok.cls_id < tok.sep_id < n - 2
  for s in sv.targeted(name):
    ids = tok.encode_batch([s])[0]
    toks = tok.tokenize(s)
    assert toks == [tok.ids_to_tokens[i] for i in ids], s
    assert tok.convert_tokens_to_ids(toks) == ids, (s, toks, ids)
    assert all(hf[t] == i for t, i in zip(toks, ids)), s
  if name.startswith('specials'):
    assert tok.tokenize('dup xdup [MASK] [CLS]') == ['dup', 'x', '##dup', '[MASK]', '[CLS]']
    assert tok.convert_tokens_to_ids(['dup', '##dup', 'nosuch']) == [hf['dup'], hf['##dup'], tok.unk_id]
    assert hf['dup'] == n - 3
