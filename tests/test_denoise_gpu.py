"""BART's full denoising collate (lddl_collate_denoise_rows*, CodeCollate.collate_denoise*) bit for bit against
tests/denoise_model.py, on hand-made row tables over the 'tiny65' vocabulary as tests/test_infill_gpu.py builds them.
The full stop is 'z' (id 30); no other token of the rows is."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import denoise_model as dm
import infill_model as im
import test_infill_gpu as ti
import test_span_mask_gpu as ts
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

CLS, SEP, MASK, V, IGNORE, SEED, STOP = ts.CLS, ts.SEP, ts.MASK, ts.V, -1, 1, 30
EINVAL, ECAPACITY, EINDEX, LAWS, P = -1, -6, -7, ti.LAWS[:2], ti.P


def body(k, seed=0):
  return [t - (t == STOP) for t in ts.mix(k, seed)]


def sents(m, seed=0):  # m sentences of three tokens, the last without its stop
  return sum([body(2, seed + i) + [STOP] for i in range(m - 1)], []) + body(2, seed + m)


ROWS = [
    ([], body(40, 1), 0, 0),                                   # 0: no stop: m = 1
    ([], body(5, 2) + [STOP] + body(7, 3), 0, 0),              # 1: m = 2
    ([], sents(64, 4), 0, 0),                                  # 2, 3: the rank leaves the registers, the destination
    ([], sents(65, 5), 0, 0),                                  #       carry crosses a step
    ([], body(60, 6) + [STOP] + body(10, 7) + [STOP] + body(5, 8), 0, 0),  # 4: a sentence over columns 62 .. 72
    ([], [STOP] + body(6, 9) + [STOP] + body(4, 10), 0, 0),    # 5: opens with a stop
    ([], body(4, 11) + [STOP] * 3 + body(5, 12) + [STOP] + body(3, 13), 0, 0),  # 6: a '...' run
    (sents(3, 14), sents(3, 15) + [STOP], 1, 0),               # 7: [CLS] doc [SEP] code [SEP], the code ends with a stop
    ([], sents(4, 16), 1, 0),                                  # 8: a = 0, s = 1
    ([], body(100, 17) + [STOP] + body(98, 18), 0, 0),         # 9: 201 columns: an odd padded length at alignment 1
    ([], [STOP] + [5, STOP] * 1022 + [5], 0, 0),               # 10: 2048 columns, 1024 sentences: the tables' capacity
]
SMALL, BIG = tuple(range(10)), (10, 7, 1)


@functools.lru_cache(maxsize=None)
def table():
  return ts.make_table(ROWS, CLS, SEP)


@functools.lru_cache(maxsize=None)
def expect(idx, law, permute, random):
  """[(the row, its denoise_model.Row)] of the batch ROWS[idx], computed once and shared"""
  q, cdf = im.params(law[2], law[1], law[0])
  out = []
  for r, g in enumerate(idx):
    a, b, s, _ = ROWS[g]
    ids = np.asarray([CLS] + a + [SEP] * s + b + [SEP], np.int64)
    sp = np.isin(np.arange(len(ids)), [0, len(a) + 1 if s else 0, len(ids) - 1])
    out.append((ids, dm.row(ids, sp, ts.cont_table(), SEED, 0, r, q, cdf, law[2], MASK, V, permute, random, STOP)))
  return out


def denoise(idx, law, permute, random, unpadded=False, align=8):
  col = ts.collate('mlm', None, seed=SEED, align=align)
  f = col.collate_denoise_unpadded if unpadded else col.collate_denoise
  out = f(table(), idx, mask_ratio=law[0], poisson_lambda=law[1], max_span=law[2], permute_sentences=permute,
          random_ratio=random, full_stop=STOP)
  assert col.counter == 1
  return out


def check(idx, law, permute, random, S):
  want = expect(idx, law, permute, random)
  lens = np.asarray([len(m.enc) for _, m in want])
  for align in (8, 1):
    pad, flat = (denoise(idx, law, permute, random, u, align) for u in (False, True))
    W = S + align - 1 & -align
    assert tuple(pad['input_ids'].shape) == (len(idx), W)
    w = {k: np.zeros((len(idx), W), np.int64) for k in ('input_ids', 'attention_mask', 'decoder_input_ids')}
    w['labels'] = np.full((len(idx), W), IGNORE, np.int64)
    for r, (row, m) in enumerate(want):
      w['input_ids'][r, :len(m.enc)], w['attention_mask'][r, :len(m.enc)] = m.enc, 1
      w['decoder_input_ids'][r, :len(row) - 1], w['labels'][r, :len(row) - 1] = row[:-1], row[1:]
    w['encoder_lengths'] = lens.astype(np.int32)
    for k, v in w.items():
      assert np.array_equal(ts.host(pad[k]), v), (k, align)
    rows = [row for row, _ in want]
    for k, v in {'input_ids': [m.enc for _, m in want], 'position_ids': [np.arange(n) for n in lens],
                 'decoder_input_ids': [x[:-1] for x in rows], 'labels': [x[1:] for x in rows],
                 'decoder_position_ids': [np.arange(len(x) - 1) for x in rows]}.items():
      assert np.array_equal(ts.host(flat[k]), np.concatenate(v)), (k, align)
    for side, n in (('', lens), ('decoder_', np.asarray([len(x) - 1 for x in rows]))):
      assert np.array_equal(ts.host(flat[side + 'cu_seqlens']), np.concatenate([[0], np.cumsum(n)]))
      assert flat[side + 'max_seqlen'] == n.max()


@pytest.mark.parametrize('law', LAWS)
@pytest.mark.parametrize('random', [0.0, 0.5])
@pytest.mark.parametrize('permute', [0.5, 1.0])
def test_against_model(gpu, permute, random, law):
  want = expect(SMALL, law, permute, random)
  # the rows do their job at this seed: a real permutation, a partial one, nothing across the inner [SEP], both
  # outcomes of the replacement draw
  orders = [o for _, m in want for o in m.orders.values()]
  assert any((o != np.arange(len(o))).any() for o in orders)
  if permute == 0.5:
    assert any((o != np.arange(len(o))).any() and (o == np.arange(len(o))).any() for o in orders)
  row, m = want[7]
  assert all(sorted(row[s]) == sorted(m.permuted[s]) and (row[s] != m.permuted[s]).any() for s in (slice(1, 9), slice(10, 19)))
  hit = np.concatenate([m.replaced for _, m in want])
  assert not hit.any() if random == 0 else hit.any() and not hit.all()
  check(SMALL, law, permute, random, 201)


@pytest.mark.parametrize('random', [0.0, 0.5])
@pytest.mark.parametrize('permute', [0.5, 1.0])
def test_table_capacity(gpu, permute, random):
  order = expect(BIG, LAWS[0], permute, random)[0][1].orders[0]
  assert len(order) == 1024 and (order != np.arange(1024)).sum() > 400
  check(BIG, LAWS[0], permute, random, 2048)


@pytest.mark.parametrize('unpadded', [False, True])
def test_reductions(gpu, unpadded):
  law, keys = LAWS[0], ('decoder_input_ids', 'labels')
  col = ts.collate('mlm', None, seed=SEED)
  fill = col.collate_infill_unpadded if unpadded else col.collate_infill
  base = fill(table(), SMALL, mask_ratio=law[0], poisson_lambda=law[1], max_span=law[2])
  same = denoise(SMALL, law, 0.0, 0.0, unpadded)  # no permutation, no replacement: text infilling
  assert base.keys() == same.keys()
  for k, v in base.items():
    assert v == same[k] if isinstance(v, int) else torch.equal(v, same[k]), k
  whole = denoise(SMALL, (0.0,) + law[1:], 1.0, 0.5, unpadded)  # nothing selected: the permuted rows themselves
  want = [m.permuted for _, m in expect(SMALL, (0.0,) + law[1:], 1.0, 0.5)]
  got = ts.host(whole['input_ids'])
  if unpadded:
    assert np.array_equal(got, np.concatenate(want))
  else:
    assert ts.host(whole['encoder_lengths']).tolist() == [len(x) for x in want]
    assert all(np.array_equal(got[r, :len(x)], x) for r, x in enumerate(want))
  assert all(torch.equal(whole[k], base[k]) for k in keys)


@pytest.mark.parametrize('which', ['rows', 'cu_seqlens', 'unpadded'])
def test_refusals(gpu, which):
  law, res, idx = LAWS[0], table(), [5, 1, 6]
  good = denoise(tuple(idx), law, 1.0, 0.5, unpadded=True)
  T = [int(good['cu_seqlens'][-1]), int(good['decoder_cu_seqlens'][-1])]
  st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

  def call(idx=idx, S=24, permute=1.0, random=0.5, stop=STOP, cu=None):
    rows = torch.as_tensor(idx, dtype=torch.int64, device='cuda')
    tab = (ts.tok().handle, P(res.ids), P(res.src0), P(res.src1), P(res.len0), P(res.len1), P(res.flags), P(rows), 0, len(idx),
           res.n_pairs)
    draw = (law[2], law[1], law[0], permute, random, stop, SEED, 0)
    L = _lib.lib()
    if which == 'rows':
      outs = torch.full((4, len(idx), S), -7, dtype=torch.int64, device='cuda')
      lens = torch.full((len(idx),), -7, dtype=torch.int32, device='cuda')
      rc = L.lddl_collate_denoise_rows(*tab, S, IGNORE, *draw, *[P(o) for o in outs], P(lens), st)
      return rc, [outs[:, r] for r in range(len(idx))]
    if which == 'cu_seqlens':
      cu2 = torch.full((2, len(idx) + 1), -7, dtype=torch.int32, device='cuda')
      tot, mx = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
      return L.lddl_collate_denoise_rows_cu_seqlens(*tab, *draw, P(cu2[0]), P(cu2[1]), tot, mx, st), []
    cu = cu or [good['cu_seqlens'], good['decoder_cu_seqlens']]
    outs = [torch.full((T[k],), -7, dtype=torch.int64, device='cuda') for k in (0, 0, 1, 1, 1)]
    rc = L.lddl_collate_denoise_rows_unpadded(*tab, P(cu[0]), P(cu[1]), T[0], T[1], IGNORE, *draw, *[P(o) for o in outs], st)
    c = [ts.host(x) for x in cu]
    return rc, [torch.cat([o[c[k][r]:c[k][r + 1]] for o, k in zip(outs, (0, 0, 1, 1, 1))]) for r in range(len(idx))]

  assert call()[0] == 0
  for bad in (dict(permute=1.5), dict(permute=float('nan')), dict(random=-0.1), dict(random=float('inf')), dict(stop=-1),
              dict(stop=65536)):
    assert call(**bad)[0] == EINVAL, bad
  for bad in (len(ROWS), -1):
    rc, rows = call(idx=[5, bad, 6])
    assert rc == EINDEX and (which == 'cu_seqlens' or (bool((rows[1] == -7).all()) and bool((rows[0] != -7).all())))
  if which == 'rows':
    rc, rows = call(S=14)  # row 1 has 15 columns
    assert rc == ECAPACITY and bool((rows[0] != -7).all()) and bool((rows[1] == -7).all())
  if which == 'unpadded':
    for side in (0, 1):
      cu = [good['cu_seqlens'].clone(), good['decoder_cu_seqlens'].clone()]
      cu[side][1] += 1  # row 0 a token longer, row 1 a token shorter; the last row and the totals stay
      rc, rows = call(cu=cu)
      assert rc == EINVAL and b'cu_seqlens' in _lib.lib().lddl_last_error()
      assert bool((rows[0] == -7).all()) and bool((rows[1] == -7).all()) and bool((rows[2] != -7).all())
