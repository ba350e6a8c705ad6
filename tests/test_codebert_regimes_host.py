"""tests/codebert_regimes.py on the host: for every configuration the GPU
tests run, the oracle's walk alone reaches every regime of the CodeBERT packer
that the configuration is there for (conditions on the corpus and the pinned
seeds, not measurements: a corpus or seed that misses one fails here), the
main corpus raises nowhere and each error corpus raises exactly its
exception."""
import pytest

import codebert_regimes as cr
from oracle import pack_oracle as po


@pytest.mark.parametrize('seq,ssp', cr.CONFIGS)
def test_oracle_walk_reaches_required_regimes(seq, ssp):
  visits, rows, counts = cr.oracle_rows(seq, ssp)  # (trace() checks every visit against the oracle's draws and rows)
  got = cr.classify(visits, seq)
  req = cr.required(seq, ssp)
  assert not req - got, sorted(req - got, key=str)
  assert len(counts) == cr.N_PART and sum(counts[1]) == 0 and all(sum(c) for k, c in enumerate(counts) if k != 1)


@pytest.mark.parametrize('seq,ssp', cr.CONFIGS)
def test_required_names_the_issue_list(seq, ssp):
  """what required() must hold, written out: the edges of the drop rule, the
  round sizes, the twist, the window crossings, and per ssp the docstring
  regimes"""
  req = cr.required(seq, ssp)
  assert {('drop', 15), ('keep_later', 16), ('keep_first', 15), ('lost_tail',), ('stay',), ('single_over',),
          ('E', 'code', 64), ('E', 'code', 65), ('E>128', 'code'), ('cut', 'code'), ('start_at_twist', 'code'),
          ('windows', True, True), ('docs>64',), ('doc', 'none')} <= req
  assert (('doc', 'unflushed') in req and ('empty_doc_row',) in req) == (ssp < 1.0)
  assert (('flush_window', 1) in req) == (seq >= 512 and ssp < 1.0)
  assert (('doc', 'short_long') in req) == (ssp > 0.0)


def test_rows_with_an_empty_docstring_and_without_one():
  """the rows the readers had never seen: has_docstring with no docstring
  token ([CLS] [SEP] code [SEP]) beside rows of two special tokens"""
  _, rows, _ = cr.oracle_rows(128, 0.0)
  assert any(has and not dt for (_, dt, _, _, has) in rows)
  assert any(not has for (_, _, _, _, has) in rows)
  assert cr.row_tokens((0, [], [7, 8], 5, True), 1, 2) == [1, 2, 7, 8, 2]
  assert cr.row_tokens((0, [], [7, 8], 4, False), 1, 2) == [1, 7, 8, 2]
  assert cr.row_tokens((0, [5], [7, 8], 6, True), 1, 2) == [1, 5, 2, 7, 8, 2]


def test_twist_partitions_by_hand():
  """partition 2's second visit truncates from draw 312 exactly (one serial
  coin at the twist, then 63); partition 3's from draw 302 with 10 coins left
  in the state (a cut round, the serial coin, 54)"""
  for seq, ssp in cr.CONFIGS:
    visits, _, _ = cr.oracle_rows(seq, ssp)
    w = visits[2][1]
    assert (w['draw'], w['chunks'][0]['at'], w['chunks'][0]['E']) == (311, 312, 64)
    assert cr.rounds(312, 64) == [('serial', 1), ('wave', 63)]
    w = visits[3][1]
    assert (w['draw'], w['chunks'][0]['at'], w['chunks'][0]['E']) == (301, 302, 65)
    assert cr.rounds(302, 65) == [('cut', 10), ('serial', 1), ('wave', 54)]
  assert cr.rounds(1, 310) == [('wave', 64)] * 4 + [('wave', 54)]
  assert cr.rounds(250, 130) == [('cut', 62), ('serial', 1), ('wave', 64), ('wave', 3)]


def test_walk_by_hand():
  """visits written out by hand against the kernel's formulas (seq 128: max_doc 32)"""
  w = cr.walk([5, 6], [4, 9, 3], 128, False)  # the stop index 2 lies past the 2 lines: never flushed
  assert (w['flush'], w['dn'], w['doc_len'], w['lim']) == (None, 0, 0, 125)
  w = cr.walk([5, 6], [4, 9, 3], 128, True)
  assert (w['flush'], w['dn'], w['doc_len'], w['lim']) == (None, 1, 5, 120)
  w = cr.walk([5, 6, 7], [4, 9], 128, False)  # the stop index 1
  assert (w['flush'], w['dn'], w['doc_len']) == (1, 2, 11)
  w = cr.walk([31, 2, 3], [9], 128, False)  # one code segment: the stop index 0 flushes line 0 alone
  assert (w['flush'], w['dn'], w['doc_len']) == (0, 1, 31)
  w = cr.walk([31, 2, 3], [9, 9, 9], 128, False)  # 33 > 32 at line 1: the line is left out
  assert (w['flush'], w['dn'], w['doc_len']) == (1, 1, 31)
  w = cr.walk([96], [9], 128, False)
  assert (w['flush'], w['dn'], w['Ed'], w['doc_len']) == (0, 1, 64, 32)
  w = cr.walk([], [127, 15], 128, False)  # max_num 126: cut by 1, then 15 tokens dropped
  assert [(c['cn'], c['stay'], c['E'], c['n'], c['kept']) for c in w['chunks']] == [(1, False, 1, 126, True),
                                                                                   (1, False, 0, 15, False)]
  w = cr.walk([], [116, 30], 128, False)  # the tail overflows a chunk of 2, stays and is lost
  assert [(c['cn'], c['stay'], c['E'], c['n']) for c in w['chunks']] == [(2, True, 20, 126)] and w['lost_tail']
  w = cr.walk([], [123, 10, 6], 128, False)  # 10 stays, 10 + 6 = 16 kept
  assert [(c['cs'], c['cn'], c['stay'], c['n'], c['kept'], c['carried']) for c in w['chunks']] == [
      (0, 2, True, 126, True, 0), (1, 2, False, 16, True, 10)]
  assert cr.walk([125], [9], 128, True)['error'] == 'AssertionError'
  assert cr.walk([126], [9], 128, True)['error'] == 'IndexError'
  assert cr.walk([3], [1], 5, False)['error'] == 'IndexError' and cr.walk([2], [1], 5, False)['error'] == 'AssertionError'


@pytest.mark.parametrize('seq,ssp,exc', cr.ERROR_CONFIGS)
def test_error_corpora_raise_exactly(seq, ssp, exc):
  """the oracle raises that exception in partition 1 and in no other"""
  docs, ndoc, pdo = cr.error_corpus(seq, exc)
  raised = []
  for p in range(3):
    D, nd = cr.partition_docs(docs, ndoc, pdo, p)
    try:
      po.partition_pairs(D, cr.PACK_SEED + p, lambda X, di, r: po.codebert_pairs(X, nd, di, seq, ssp, r), cr.DUP)
      raised.append(None)
    except (IndexError, AssertionError) as e:
      raised.append(type(e).__name__)
  assert raised == [None, exc, None]


def test_smallest_accepted_seq_raises():
  """5 is lddl_pack_codebert's smallest target_seq_length (capi_pack.hip);
  the ordinary docstring path raises IndexError there"""
  assert (5, 0.0, 'IndexError') in cr.ERROR_CONFIGS
