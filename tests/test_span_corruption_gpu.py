"""Span-corruption collate (lddl_collate_corrupt_rows*, CodeCollate.collate_span_corruption*) bit for bit against
tests/corrupt_model.py, on the hand-made row tables of tests/test_infill_gpu.py; sentinels outside 'tiny65'."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import corrupt_model as cm
import infill_model as im
import stream_cases as sc
import test_infill_gpu as ti
import test_span_mask_gpu as ts
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

CLS, SEP, MASK, IGNORE, EINVAL, ECAPACITY, EINDEX = ti.CLS, ti.SEP, ti.MASK, ti.IGNORE, ti.EINVAL, ti.ECAPACITY, ti.EINDEX
SEED = 108  # a draw at which every batch holds what its rows are there for (asserted on the model below)
LAWS, SIZES, ROWS, EXTRA, ALL, P = ti.LAWS, ti.SIZES, ti.ROWS, ti.EXTRA, ti.ALL, ti.P
SENT = (1000, 2048)  # more sentinels than a row can have runs
KEYS = ('input_ids', 'attention_mask', 'decoder_input_ids', 'labels', 'encoder_lengths', 'decoder_lengths')


@functools.lru_cache(maxsize=None)
def expect(idx, law, sent=SENT):
  """[(the row, the encoder's tokens, the target, selected, ord)] of the batch ROWS[idx], computed once and shared"""
  q, cdf = im.params(law[2], law[1], law[0])
  out = []
  for r, g in enumerate(idx):
    a, b, s, _ = ROWS[g]
    ids = np.asarray([CLS] + a + [SEP] * s + b + [SEP], np.int64)
    sp = np.isin(np.arange(len(ids)), [0, len(a) + 1 if s else 0, len(ids) - 1])
    out.append((ids,) + cm.row(ids, sp, ts.cont_table(), SEED, 0, r, q, cdf, law[2], sent[0], sent[1], SEP))
  return out


def planes(idx, law, S, sent=SENT):
  n = len(idx)
  w = {k: np.zeros((n, S), np.int64) for k in KEYS[:3]}
  w['labels'] = np.full((n, S), IGNORE, np.int64)
  for r, (_, enc, tgt, _, _) in enumerate(expect(idx, law, sent)):
    w['input_ids'][r, :len(enc)], w['attention_mask'][r, :len(enc)] = enc, 1
    w['labels'][r, :len(tgt)], w['decoder_input_ids'][r, :len(tgt)] = tgt, np.concatenate([[CLS], tgt[:-1]])
  w['encoder_lengths'] = np.asarray([len(x[1]) for x in expect(idx, law, sent)], np.int32)
  w['decoder_lengths'] = np.asarray([len(x[2]) for x in expect(idx, law, sent)], np.int32)
  return w


def corrupt(idx, law, unpadded=False, align=8, res=None, sent=SENT):
  col = ts.collate('mlm', None, seed=SEED, align=align)
  f = col.collate_span_corruption_unpadded if unpadded else col.collate_span_corruption
  out = f(res or ti.table(), idx, mask_ratio=law[0], poisson_lambda=law[1], max_span=law[2], sentinels=sent)
  assert col.counter == 1
  return out


def check_padded(out, idx, law, S, sent=SENT):
  assert tuple(out['input_ids'].shape) == (len(idx), S) and set(out) == set(KEYS)
  for k, v in planes(idx, law, S, sent).items():
    assert np.array_equal(ts.host(out[k]), v), k


@pytest.mark.parametrize('law', LAWS)
@pytest.mark.parametrize('n', SIZES)
def test_padded_against_model(gpu, n, law):
  idx = (SIZES.index(n),) + EXTRA
  sel, od = [x[3] for x in expect(idx, law)], [x[4] for x in expect(idx, law)]
  # what the rows are there for happens at this draw: a run across columns 63 | 64 that keeps its ordinal, a run that
  # opens at a first lane, no run over the inner [SEP]
  assert any(len(s) > 64 and s[63] and s[64] and o[63] == o[64] for s, o in zip(sel, od))
  assert any(s[j] and not s[j - 1] for s in sel for j in range(64, len(s), 64))
  assert not sel[4][24] and sel[4][1:24].any() and sel[4][25:].any()
  check_padded(corrupt(idx, law), idx, law, max(n, 201) + 7 & ~7)
  check_padded(corrupt(idx, law, align=1), idx, law, max(n, 201))  # 201: rows at odd offsets of the planes


@pytest.mark.parametrize('count', [2, 11])
def test_sentinel_cap(gpu, count):
  law, sent = LAWS[1], (1000, count)
  ex = expect(ALL, law, sent)
  runs = [int(x[4].max()) + 1 for x in ex]
  assert sum(k > 2 for k in runs) > len(ALL) // 2 and any(k > count for k in runs)
  late = False
  for (ids, enc, _, _, od), k in zip(ex, runs):
    if k > count:  # behind the last corrupted run the row is verbatim, later runs included
      end = np.flatnonzero(od == count - 1)[-1] + 1
      assert np.array_equal(enc[len(enc) - (len(ids) - end):], ids[end:]) and (od[end:] >= count).any()
      late |= np.flatnonzero(od == count - 1)[0] >= 64 > np.flatnonzero(od == 0)[0]
  assert late or count == 2  # count 11: the last sentinel's run opens in a later step than the first's
  check_padded(corrupt(ALL, law, sent=sent), ALL, law, 2048, sent)


def test_limits(gpu):
  out = corrupt(ALL, (0.0, 3.0, 10))
  check_padded(out, ALL, (0.0, 3.0, 10), 2048)
  assert ts.host(out['encoder_lengths']).tolist() == [ts.row_len(ROWS, g) for g in ALL]
  assert ts.host(out['decoder_lengths']).tolist() == [1] * len(ALL) and bool((out['labels'][:, 0] == SEP).all())
  out = corrupt((0, 10), (1.0, 3.0, 10))
  check_padded(out, (0, 10), (1.0, 3.0, 10), 104)
  assert ts.host(out['input_ids'])[:, :6].tolist() == [[CLS, 1000, SEP, 0, 0, 0], [CLS, 1000, SEP, 1001, SEP, 0]]
  doc, code = ROWS[10][:2]
  lab = ts.host(out['labels'])
  assert lab[0, :4].tolist() == [1000, ROWS[0][1][0], SEP, IGNORE]  # t_r = n = 3
  assert lab[1, :99].tolist() == [1000] + doc + [1001] + code + [SEP, IGNORE]
  assert ts.host(out['decoder_lengths']).tolist() == [3, 98]


def test_unpadded_is_the_padded_batch_without_its_padding(gpu):
  law, parity = LAWS[0], set()
  for idx in (ALL, ALL[1:]):
    pad, flat = corrupt(idx, law), corrupt(idx, law, unpadded=True)
    cols = np.arange(2048)[None, :]
    for side, names in (('', ('input_ids',)), ('decoder_', ('decoder_input_ids', 'labels'))):
      lens = ts.host(pad[(side or 'encoder_') + 'lengths']).astype(np.int64)
      assert np.array_equal(ts.host(flat[side + 'cu_seqlens']), np.concatenate([[0], np.cumsum(lens)]))
      assert flat[side + 'max_seqlen'] == lens.max()
      assert np.array_equal(ts.host(flat[side + 'position_ids']), np.concatenate([np.arange(x) for x in lens]))
      for k in names:
        assert np.array_equal(ts.host(flat[k]), ts.host(pad[k])[cols < lens[:, None]]), k
      parity.add((side, int(lens.sum()) % 2))
  assert len(parity) == 4  # both totals even and odd: 16-B pairs, and lane = token behind an odd total


def call_padded(idx, S, sent, outs, lens, law=LAWS[0]):
  rows = torch.as_tensor(idx, dtype=torch.int64, device='cuda')
  res = ti.table()
  return _lib.lib().lddl_collate_corrupt_rows(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, len(idx),
      res.n_pairs, S, IGNORE, law[2], law[1], law[0], sent[0], sent[1], SEED, 0, *[P(o) for o in outs], P(lens[0]),
      P(lens[1]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_errors(gpu):
  outs = torch.full((4, 2, 208), -7, dtype=torch.int64, device='cuda')
  lens = torch.full((2, 2), -7, dtype=torch.int32, device='cuda')
  for bad in (len(ROWS), -1):
    assert call_padded([8, bad], 208, SENT, outs, lens) == EINDEX
    assert bool((outs[:, 1] == -7).all()) and lens[:, 1].tolist() == [-7, -7]
  short = torch.full((4, 2, 200), -7, dtype=torch.int64, device='cuda')
  assert call_padded([2, 8], 200, SENT, short, lens) == ECAPACITY  # row 8 has 201 columns
  assert bool((short[:, 1] == -7).all()) and bool((short[:, 0] != -7).all())
  outs.fill_(-7)
  assert call_padded([2, 8], 2049, SENT, outs, lens) == ECAPACITY
  for sent in ((1000, 0), (-1, 4), (65000, 537), (MASK, 1)):
    assert call_padded([2, 8], 208, sent, outs, lens) == EINVAL and b'sentinels' in _lib.lib().lddl_last_error()
  assert bool((outs == -7).all())
  assert call_padded([2, 8], 208, (65000, 536), outs, lens) == 0  # the last id that the staging holds


@pytest.mark.parametrize('unpadded', [False, True])
def test_default_sentinels_come_from_the_collate_vocabulary(gpu, unpadded):
  with pytest.raises(ValueError, match='sentinels'):  # 'tiny65' has no [unused0]
    corrupt((2, 8), LAWS[0], unpadded=unpadded, sent=None)


@pytest.mark.parametrize('side', [0, 1])
def test_tampered_cu_seqlens(gpu, side):
  """every row's offsets hold one token too many: every row is refused and nothing is written"""
  law, res, n = LAWS[0], ti.table(), len(ALL)
  flat = corrupt(ALL, law, unpadded=True)
  cu = [flat['cu_seqlens'].clone(), flat['decoder_cu_seqlens'].clone()]
  cu[side] += torch.arange(n + 1, dtype=torch.int32, device='cuda')
  T = [int(cu[0][-1]), int(cu[1][-1])]
  outs = [torch.full((T[k],), -7, dtype=torch.int64, device='cuda') for k in (0, 0, 1, 1, 1)]
  rows = torch.as_tensor(ALL, dtype=torch.int64, device='cuda')
  rc = _lib.lib().lddl_collate_corrupt_rows_unpadded(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, n,
      res.n_pairs, P(cu[0]), P(cu[1]), T[0], T[1], IGNORE, law[2], law[1], law[0], *SENT, SEED, 0, *[P(o) for o in outs],
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == EINVAL and b'cu_seqlens' in _lib.lib().lddl_last_error()
  assert all(bool((o == -7).all()) for o in outs)


@pytest.mark.parametrize('unpadded', [False, True])
def test_side_stream_behind_a_pending_producer(gpu, unpadded):
  # stream_cases' harness: the ids arrive behind a delay on a side stream, and every pass must wait for them there
  res = ts.make_table(ROWS, CLS, SEP)  # its own: the ids are overwritten
  idx = (8, 9, 10, 4, 5)

  def call(stream, which):
    with torch.cuda.stream(stream):  # (None: a no-op)
      return corrupt(idx, LAWS[0], unpadded=unpadded, res=res)
  case = sc.Case('collate_span_corruption[%d]' % unpadded, 'corrupt', (('ids', 'values'),))
  a = res.ids.cpu().numpy().view(np.uint16)  # every id of the table is a vocabulary id: so is every mixture with its roll
  base_a, base_b, got = sc.run_delayed(case, [('ids', 'values', res.ids, a)], call, sc.calibrate()[0], {})
  sc.assert_same(case, base_a, base_b, got)
