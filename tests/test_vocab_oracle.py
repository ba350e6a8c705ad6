"""The oracle (C restatement of HF tokenizers) against HF tokenizers 0.22.2 on
the synthetic vocabularies of tests/synth_vocab.py (goldens:
tools/gen_golden_vocab.py), and the generator against what is committed.
CPU only."""
import json
import os

import numpy as np
import pytest

import synth_vocab as sv
from conftest import GOLDEN
from oracle.oracle import OracleTokenizer, compact, lib


@pytest.mark.parametrize('name', sv.SMALL)
def test_committed_vocab_is_what_the_generator_makes(name):
  with open(os.path.join(sv.VOCAB_DIR, name + '.txt'), 'rb') as f:
    assert f.read() == sv.vocab_bytes(name)


@pytest.mark.parametrize('name', sv.NAMES)
def test_golden_corpus_is_what_the_generator_makes(golden, name):
  from lddl_amd.synth import corpus_from_sentences
  s = sv.sentences(name)
  c = corpus_from_sentences(s, [0, len(s)])
  data, off, ids, ntok = sv.load_golden(golden, name)
  assert np.array_equal(c.data, data) and np.array_equal(c.sent_off, off)
  assert len(ids) == len(s) == len(ntok)
  assert c.nbytes < 330_000


def test_goldens_reach_the_ids_they_were_written_for(golden):
  """the last id of every size, 0xEFFF / 0xF000 (the split tokenizer's first
  'queued word' entry value) and 0xFFFF (its 'empty unit' value, a legal id
  at V = 65536) appear in the expected output"""
  for v in sv.SIZES:
    flat = np.concatenate(sv.load_golden(golden, 'v%d' % v)[2])
    want = {v - 1} | {i for i in (0x7FFF, 0x8000, 0xEFFF, 0xF000, 0xFFFE, 0xFFFF) if i < v}
    assert want <= set(flat.tolist()), (v, sorted(want - set(flat.tolist())))
  for name in ('specials', 'specials_padlast'):
    flat = set(np.concatenate(sv.load_golden(golden, name)[2]).tolist())
    n = sv.vocab_size(name)
    assert {0, n - 1, n - 2} <= flat  # [UNK] at 0, [PAD] / [MASK] at the end


@pytest.mark.parametrize('max_tok', [512, 3])
@pytest.mark.parametrize('name', sv.NAMES)
def test_oracle_matches_hf(golden, name, max_tok):
  data, off, exp, ntok = sv.load_golden(golden, name)
  ids, n = OracleTokenizer(sv.vocab_path(name)).run(data, off, max_tok, nthreads=4)
  got = compact(ids, n, off)
  bad = [i for i in range(len(exp)) if n[i] != min(ntok[i], max_tok) or not np.array_equal(exp[i][:max_tok], got[i])]
  assert not bad, [(i, sv.sentence_text(data, off, i)[:80], exp[i][:8].tolist(), got[i][:8].tolist()) for i in bad[:5]]


@pytest.mark.parametrize('name', sv.LINE_VOCABS)
def test_oracle_vocab_lines_as_hf(name):
  """HF's token -> id map of the vocabularies with trailing blanks, CRLF
  lines, duplicates and an empty line: every such token, alone in a
  sentence, gets that id from the oracle when it is reachable at all (no
  blank inside, not split by the pre-tokenizer)"""
  both = json.load(open(os.path.join(GOLDEN, 'vocab_lines_hf.json')))
  hf = both[name]
  tok = OracleTokenizer(sv.vocab_path(name))
  # [PAD] [UNK] [CLS] [SEP] [MASK]: a special on two lines has the later id
  assert [lib().orc_tok_special_id(tok.h, k) for k in range(5)] == both[name + ':special_ids']
  assert both[name + ':special_ids'] == [hf[s] for s in sv.SPECIALS]
  from lddl_amd.synth import corpus_from_sentences
  words = [(t, i) for t, i in hf.items() if t and not t.startswith('##') and t.isalnum() and t.isascii()]
  assert len(words) > 20
  c = corpus_from_sentences([t for t, _ in words], [0, len(words)])
  ids, n = tok.run(c.data, c.sent_off, 512)
  for (t, i), g in zip(words, compact(ids, n, c.sent_off)):
    assert g.tolist() == [i], (t, i, g.tolist())
