"""Text-infilling collate (lddl_collate_infill_rows*, CodeCollate.collate_infill*) bit for bit against
tests/infill_model.py, on hand-made row tables over the 'tiny65' vocabulary as tests/test_span_mask_gpu.py builds them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import infill_model as im
import stream_cases as sc
import test_span_mask_gpu as ts
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

CLS, SEP, MASK, IGNORE, SEED = ts.CLS, ts.SEP, ts.MASK, -1, 31
EINVAL, ECAPACITY, EINDEX = -1, -6, -7
LAWS = [(0.3, 3.0, 10), (0.5, 1.0, 1), (0.9, 6.0, 16)]  # (mask_ratio, poisson_lambda, max_span)
# the smallest lengths that reach a lane boundary (3), a step boundary (64 .. 66), a third step (128, 129) and the
# whole LDS slice (2048); there is no two-column-per-lane path
SIZES = [3, 64, 65, 66, 128, 129, 2048]
ROWS = [([], ts.mix(n - 2, k), 0, 0) for k, n in enumerate(SIZES)] + [
    ([], ts.word(100, 3), 0, 0),    # 7: one word of 100 pieces: the head and span carries cross a step
    ([], ts.plain(199, 1), 0, 0),   # 8, 9: every token a word; 201 columns: an odd padded length at alignment 1
    ([], ts.plain(150, 9), 0, 0),
    (ts.word(3, 2) + ts.plain(20, 5), ts.pieces(2, 7) + ts.mix(70, 50), 1, 0),  # 10: [CLS] doc [SEP] code [SEP], [SEP] at 24
    ([], ts.mix(30, 51), 1, 0),     # 11: a = 0, s = 1: [CLS] [SEP] code [SEP]
]
EXTRA, ALL = (7, 8, 9, 10, 11, 7), tuple(range(len(ROWS)))
P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731


@functools.lru_cache(maxsize=None)
def table():
  return ts.make_table(ROWS, CLS, SEP)


@functools.lru_cache(maxsize=None)
def expect(idx, law):
  """[(the row, the encoder's tokens, selected)] of the batch ROWS[idx], computed once and shared"""
  q, cdf = im.params(law[2], law[1], law[0])
  out = []
  for r, g in enumerate(idx):
    a, b, s, _ = ROWS[g]
    ids = np.asarray([CLS] + a + [SEP] * s + b + [SEP], np.int64)
    sp = np.isin(np.arange(len(ids)), [0, len(a) + 1 if s else 0, len(ids) - 1])
    out.append((ids,) + im.row(ids, sp, ts.cont_table(), SEED, 0, r, q, cdf, law[2], MASK))
  return out


def planes(idx, law, S):
  n = len(idx)
  w = {k: np.zeros((n, S), np.int64) for k in ('input_ids', 'attention_mask', 'decoder_input_ids')}
  w['labels'] = np.full((n, S), IGNORE, np.int64)
  for r, (row, enc, _) in enumerate(expect(idx, law)):
    w['input_ids'][r, :len(enc)], w['attention_mask'][r, :len(enc)] = enc, 1
    w['decoder_input_ids'][r, :len(row) - 1], w['labels'][r, :len(row) - 1] = row[:-1], row[1:]
  w['encoder_lengths'] = np.asarray([len(enc) for _, enc, _ in expect(idx, law)], np.int32)
  return w


def infill(idx, law, unpadded=False, align=8, res=None, **pick):
  col = ts.collate('mlm', None, seed=SEED, align=align)
  f = col.collate_infill_unpadded if unpadded else col.collate_infill
  out = f(res or table(), idx, mask_ratio=law[0], poisson_lambda=law[1], max_span=law[2], **pick)
  assert col.counter == 1
  return out


def check_padded(out, idx, law, S):
  assert tuple(out['input_ids'].shape) == (len(idx), S)
  for k, v in planes(idx, law, S).items():
    assert np.array_equal(ts.host(out[k]), v), k


@pytest.mark.parametrize('law', LAWS)
@pytest.mark.parametrize('n', SIZES)
def test_padded_against_model(gpu, n, law):
  idx = (SIZES.index(n),) + EXTRA
  sel = [s for _, _, s in expect(idx, law)]
  # what the rows are there for happens at this draw: a selected run across columns 63 | 64, no span over the inner [SEP]
  assert any(len(s) > 64 and s[63] and s[64] for s in sel)
  assert not sel[4][24] and sel[4][1:24].any() and sel[4][25:].any()
  check_padded(infill(idx, law), idx, law, max(n, 201) + 7 & ~7)
  check_padded(infill(idx, law, align=1), idx, law, max(n, 201))  # 201: rows at odd offsets of the planes


def test_limits(gpu):
  out = infill(ALL, (0.0, 3.0, 10))
  check_padded(out, ALL, (0.0, 3.0, 10), 2048)
  assert ts.host(out['encoder_lengths']).tolist() == [ts.row_len(ROWS, g) for g in ALL]
  out = infill((1, 10), (1.0, 3.0, 10))
  check_padded(out, (1, 10), (1.0, 3.0, 10), 104)
  assert ts.host(out['input_ids'])[:, :6].tolist() == [[CLS, MASK, SEP, 0, 0, 0], [CLS, MASK, SEP, MASK, SEP, 0]]


def call_padded(idx, S, law, outs, lens):
  rows = torch.as_tensor(idx, dtype=torch.int64, device='cuda')
  res = table()
  return _lib.lib().lddl_collate_infill_rows(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, len(idx),
      res.n_pairs, S, IGNORE, law[2], law[1], law[0], SEED, 0, *[P(o) for o in outs], P(lens),
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_row_picking_and_errors(gpu):
  law, idx = LAWS[0], (8, 2, 8, 9, 8)
  out = infill(idx, law)
  check_padded(out, idx, law, 208)
  enc = ts.host(out['input_ids'])
  assert not np.array_equal(enc[0], enc[2]) and not np.array_equal(enc[2], enc[4])  # the draw is keyed by the batch row
  check_padded(infill(None, law, row0=7, n_rows=3), (7, 8, 9), law, 208)
  outs = torch.full((4, 2, 208), -7, dtype=torch.int64, device='cuda')
  lens = torch.full((2,), -7, dtype=torch.int32, device='cuda')
  for bad in (len(ROWS), -1):
    assert call_padded([8, bad], 208, law, outs, lens) == EINDEX
    assert bool((outs[:, 1] == -7).all()) and lens.tolist()[1] == -7
  short = torch.full((4, 2, 200), -7, dtype=torch.int64, device='cuda')
  assert call_padded([2, 8], 200, law, short, lens) == ECAPACITY  # row 8 has 201 columns
  assert bool((short[:, 1] == -7).all()) and bool((short[:, 0] != -7).all())
  outs.fill_(-7)
  assert call_padded([2, 8], 2049, law, outs, lens) == ECAPACITY and bool((outs == -7).all())


@pytest.mark.parametrize('law', LAWS)
def test_unpadded_is_the_padded_batch_without_its_padding(gpu, law):
  parity = set()
  for idx in (ALL, ALL[:1] + ALL[2:]):
    pad, flat = infill(idx, law), infill(idx, law, unpadded=True)
    e = ts.host(pad['encoder_lengths']).astype(np.int64)
    m = np.asarray([ts.row_len(ROWS, g) - 1 for g in idx])
    cols = np.arange(2048)[None, :]
    for side, lens, keep, names in (('', e, cols < e[:, None], ('input_ids',)),
                                    ('decoder_', m, cols < m[:, None], ('decoder_input_ids', 'labels'))):
      assert np.array_equal(ts.host(flat[side + 'cu_seqlens']), np.concatenate([[0], np.cumsum(lens)]))
      assert flat[side + 'max_seqlen'] == lens.max()
      assert np.array_equal(ts.host(flat[side + 'position_ids']), np.concatenate([np.arange(x) for x in lens]))
      for k in names:
        assert np.array_equal(ts.host(flat[k]), ts.host(pad[k])[keep]), k
      parity.add((side, int(lens.sum()) % 2))
  assert {('decoder_', 0), ('decoder_', 1)} <= parity  # 16-B pairs, and lane = token behind an odd total


@pytest.mark.parametrize('side', [0, 1])
def test_tampered_cu_seqlens(gpu, side):
  """every row's offsets hold one token too many: every row is refused and nothing is written"""
  law, res, n = LAWS[0], table(), len(ALL)
  flat = infill(ALL, law, unpadded=True)
  cu = [flat['cu_seqlens'].clone(), flat['decoder_cu_seqlens'].clone()]
  cu[side] += torch.arange(n + 1, dtype=torch.int32, device='cuda')
  T = [int(cu[0][-1]), int(cu[1][-1])]
  outs = [torch.full((T[k],), -7, dtype=torch.int64, device='cuda') for k in (0, 0, 1, 1, 1)]
  rows = torch.as_tensor(ALL, dtype=torch.int64, device='cuda')
  rc = _lib.lib().lddl_collate_infill_rows_unpadded(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, n,
      res.n_pairs, P(cu[0]), P(cu[1]), T[0], T[1], IGNORE, law[2], law[1], law[0], SEED, 0, *[P(o) for o in outs],
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
      return infill(idx, LAWS[0], unpadded=unpadded, res=res)
  case = sc.Case('collate_infill[%d]' % unpadded, 'infill', (('ids', 'values'),))
  a = res.ids.cpu().numpy().view(np.uint16)  # every id of the table is a vocabulary id: so is every mixture with its roll
  base_a, base_b, got = sc.run_delayed(case, [('ids', 'values', res.ids, a)], call, sc.calibrate()[0], {})
  sc.assert_same(case, base_a, base_b, got)
