"""Exact-count span corruption (lddl_collate_corrupt_exact_rows*, CodeCollate.collate_span_corruption_exact*) bit for
bit against tests/segment_model.py, on hand-made row tables as tests/test_span_corruption_gpu.py builds them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import segment_model as sg
import stream_cases as sc
import test_infill_gpu as ti
import test_span_mask_gpu as ts
from lddl_amd import _lib, loader

pytestmark = pytest.mark.gpu

CLS, SEP, IGNORE, EINVAL, ECAPACITY, EINDEX, P = ti.CLS, ti.SEP, ti.IGNORE, ti.EINVAL, ti.ECAPACITY, ti.EINDEX, ti.P
SEED = 108
# T5's default; S = N = c - N: all gaps chosen, the take-all exit; S = 1, K = 0: one long span crossing many steps
LAWS = [(0.15, 3.0), (0.5, 1.0), (0.3, 1000.0)]
# c < 2 (2, 3); the smallest real case; a span and a cut word straddling the 64-column step; three steps; at 0.15 / 3.0
# the sentinel clip engages, 102 spans wanted and 99 given
SIZES = [2, 3, 4, 65, 66, 67, 130, 2048]
ROWS = [([], ts.mix(n - 2, k), 0, 0) for k, n in enumerate(SIZES)] + [
    (ts.plain(20, 5), ts.mix(70, 50), 1, 0),  # 8: [CLS] doc [SEP] code [SEP]: the inner [SEP] at 21 is an ordinary unit
    ([], ts.mix(30, 51), 1, 0),               # 9: a = 0, s = 1
]
EXTRA, ALL = (8, 9, 5), tuple(range(len(ROWS)))
MANY = (5, 8, 6) * 4
SENT = (1000, 99)  # the count of the BERT vocabulary's default run
KEYS = ('input_ids', 'attention_mask', 'decoder_input_ids', 'labels', 'encoder_lengths', 'decoder_lengths')


@functools.lru_cache(maxsize=None)
def table():
  return ts.make_table(ROWS, CLS, SEP)


def row_ids(g):
  a, b, s, _ = ROWS[g]
  return np.asarray([CLS] + a + [SEP] * s + b + [SEP], np.int64)


@functools.lru_cache(maxsize=None)
def expect(idx, law, sent=SENT, r0=0):
  """[(the encoder's tokens, the target, selected)] of the batch ROWS[idx] at batch rows r0 .., computed once"""
  return [sg.row(row_ids(g), SEED, 0, r0 + r, law[0], law[1], sent[0], sent[1], SEP) for r, g in enumerate(idx)]


def corrupt(idx, law, unpadded=False, align=8, res=None, sent=SENT, **pick):
  col = ts.collate('mlm', None, seed=SEED, align=align)
  f = col.collate_span_corruption_exact_unpadded if unpadded else col.collate_span_corruption_exact
  out = f(res or table(), idx, noise_density=law[0], mean_span=law[1], sentinels=sent, **pick)
  assert col.counter == 1
  return out


def check_padded(out, idx, law, S, sent=SENT, ex=None):
  n = len(idx)
  assert tuple(out['input_ids'].shape) == (n, S) and set(out) == set(KEYS)
  w = {k: np.zeros((n, S), np.int64) for k in KEYS[:3]}
  w['labels'] = np.full((n, S), IGNORE, np.int64)
  closed = np.asarray([loader.span_corruption_lengths(len(row_ids(g)), *law, num_sentinels=sent[1]) for g in idx])
  for r, (enc, tgt, _) in enumerate(ex or expect(idx, law, sent)):
    w['input_ids'][r, :len(enc)], w['attention_mask'][r, :len(enc)] = enc, 1
    w['labels'][r, :len(tgt)], w['decoder_input_ids'][r, :len(tgt)] = tgt, np.concatenate([[CLS], tgt[:-1]])
    at = np.flatnonzero(enc >= sent[0])  # S sentinels, in order, never adjacent, never first or last in the interior
    assert (len(enc), len(tgt), len(at)) == (closed[r, 0], closed[r, 1], closed[r, 3])
    assert np.array_equal(enc[at], sent[0] + np.arange(len(at))) and (np.diff(at) > 1).all()
  w['encoder_lengths'], w['decoder_lengths'] = closed[:, 0].astype(np.int32), closed[:, 1].astype(np.int32)
  for k, v in w.items():
    assert np.array_equal(ts.host(out[k]), v), k


@pytest.mark.parametrize('law', LAWS)
@pytest.mark.parametrize('n', SIZES)
def test_padded_against_model(gpu, n, law):
  idx = (SIZES.index(n),) + EXTRA
  S = max(n, 93)
  check_padded(corrupt(idx, law), idx, law, S + 7 & ~7)
  check_padded(corrupt(idx, law, align=1), idx, law, S)  # 93: rows at odd offsets of the planes


@pytest.mark.parametrize('law, sent, top, clipped', [(LAWS[0], (1000, 5), 5, 2),         # the clip rules at 130 columns too
                                                     (LAWS[1], (1000, 2048), 1023, 0)])  # take-all over 16 cut words
def test_sentinel_counts(gpu, law, sent, top, clipped):
  S, free = ([sg.counts(len(row_ids(g)), *law, k)[1] for g in ALL] for k in (sent[1], 4096))
  assert max(S) == top and sum(x != y for x, y in zip(S, free)) == clipped
  check_padded(corrupt(ALL, law, sent=sent), ALL, law, 2048, sent)


def test_the_selection_crosses_the_inner_sep_and_a_step(gpu):
  """what the rows are there for happens at the draws of the tests around this one (the model alone)"""
  sel = [x[2] for law in LAWS for n in SIZES for x in expect((SIZES.index(n),) + EXTRA, law)]
  assert expect(MANY, LAWS[0])[10][2][21] and len(row_ids(MANY[10])) == 93       # the inner [SEP] is noise
  assert any(s[j - 1] and s[j] for s in sel for j in range(64, len(s), 64))      # a span across two steps
  assert any(not s[j - 1] and s[j] for s in sel for j in range(64, len(s), 64))  # a span that opens at a first lane
  assert any(s[j - 1] and not s[j] for s in sel for j in range(64, len(s), 64))  # a span that ends with its step
  assert all(not s[0] and not s[-1] and (len(s) < 4 or (s[-2] and not s[1])) for s in sel)


@pytest.mark.parametrize('law', LAWS)
def test_unpadded_is_the_padded_batch_without_its_padding(gpu, law):
  for idx in (ALL, ALL[1:]):
    pad, flat = corrupt(idx, law), corrupt(idx, law, unpadded=True)
    closed = np.asarray([loader.span_corruption_lengths(len(row_ids(g)), *law) for g in idx], np.int64)
    cols = np.arange(2048)[None, :]
    for side, lens, names in (('', closed[:, 0], ('input_ids',)), ('decoder_', closed[:, 1], ('decoder_input_ids', 'labels'))):
      assert np.array_equal(ts.host(flat[side + 'cu_seqlens']), np.concatenate([[0], np.cumsum(lens)]))
      assert flat[side + 'max_seqlen'] == lens.max()
      assert np.array_equal(ts.host(flat[side + 'position_ids']), np.concatenate([np.arange(x) for x in lens]))
      for k in names:
        assert np.array_equal(ts.host(flat[k]), ts.host(pad[k])[cols < lens[:, None]]), k


@pytest.mark.parametrize('side', [0, 1])
def test_tampered_cu_seqlens(gpu, side):
  """row 6's offsets hold one token too many: it is refused and left unwritten, whatever the other rows do"""
  law, res, n = LAWS[0], table(), len(ALL)
  flat = corrupt(ALL, law, unpadded=True)
  cu = [flat['cu_seqlens'].clone(), flat['decoder_cu_seqlens'].clone()]
  cu[side][7:] += 1
  T = [int(cu[0][-1]), int(cu[1][-1])]
  outs = [torch.full((T[k],), -7, dtype=torch.int64, device='cuda') for k in (0, 0, 1, 1, 1)]
  rows = torch.as_tensor(ALL, dtype=torch.int64, device='cuda')
  rc = _lib.lib().lddl_collate_corrupt_exact_rows_unpadded(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, n,
      res.n_pairs, P(cu[0]), P(cu[1]), T[0], T[1], IGNORE, law[0], law[1], *SENT, SEED, 0, *[P(o) for o in outs],
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == EINVAL and b'cu_seqlens' in _lib.lib().lddl_last_error()
  for o, k in zip(outs, (0, 0, 1, 1, 1)):
    assert bool((o[int(cu[k][6]):int(cu[k][7])] == -7).all()) and bool((o[:int(cu[k][6])] != -7).all())


def test_row_picking(gpu):
  law, idx = LAWS[0], (6, 5, 6, 8, 6)
  out = corrupt(idx, law)
  check_padded(out, idx, law, 136)
  enc = ts.host(out['input_ids'])
  assert not np.array_equal(enc[0], enc[2]) and not np.array_equal(enc[2], enc[4])  # the draw is keyed by the batch row
  check_padded(corrupt(None, law, row0=4, n_rows=3), (4, 5, 6), law, 136)


def test_more_rows_than_one_pass_of_the_grid(gpu):
  n = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
  idx, law = MANY * (n // 12) + MANY[:n % 12], LAWS[0]
  out = corrupt(idx, law)
  for lo in (0, n - 12):  # the model's share: the first rows and the last; a row's draw is its batch index's
    part = {k: v[lo:lo + 12] for k, v in out.items()}
    check_padded(part, idx[lo:lo + 12], law, 136, ex=expect(idx[lo:lo + 12], law, SENT, lo))


@pytest.mark.parametrize('unpadded', [False, True])
def test_side_stream_behind_a_pending_producer(gpu, unpadded):
  # stream_cases' harness: the ids arrive behind a delay on a side stream, and every pass must wait for them there
  res = ts.make_table(ROWS, CLS, SEP)  # its own: the ids are overwritten
  idx = (6, 8, 9, 4, 5)

  def call(stream, which):
    with torch.cuda.stream(stream):  # (None: a no-op)
      return corrupt(idx, LAWS[0], unpadded=unpadded, res=res)
  case = sc.Case('collate_span_corruption_exact[%d]' % unpadded, 'corrupt', (('ids', 'values'),))
  a = res.ids.cpu().numpy().view(np.uint16)  # every id of the table is a vocabulary id: so is every mixture with its roll
  base_a, base_b, got = sc.run_delayed(case, [('ids', 'values', res.ids, a)], call, sc.calibrate()[0], {})
  sc.assert_same(case, base_a, base_b, got)


@pytest.mark.parametrize('idx, S, law, code', [((5, 8), 96, (0.0, 3.0), EINVAL), ((5, 8), 96, (1.0, 3.0), EINVAL),
                                               ((5, 8), 96, (0.15, 0.5), EINVAL), ((5, 8), 1, LAWS[0], ECAPACITY),
                                               ((5, len(ROWS)), 96, LAWS[0], EINDEX), ((5, -1), 96, LAWS[0], EINDEX)])
def test_refusals(gpu, idx, S, law, code):
  outs = torch.full((4, 2, 96), -7, dtype=torch.int64, device='cuda')
  lens = torch.full((2, 2), -7, dtype=torch.int32, device='cuda')
  rows, res = torch.as_tensor(idx, dtype=torch.int64, device='cuda'), table()
  rc = _lib.lib().lddl_collate_corrupt_exact_rows(
      ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, 2,
      res.n_pairs, S, IGNORE, law[0], law[1], *SENT, SEED, 0, *[P(o) for o in outs], P(lens[0]), P(lens[1]),
      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  assert rc == code
  assert bool((outs[:, 1] == -7).all()) and lens[:, 1].tolist() == [-7, -7]  # the refused row is left unwritten
  assert bool((outs[:, 0] != -7).all()) == (code == EINDEX)  # a refused call launches nothing
