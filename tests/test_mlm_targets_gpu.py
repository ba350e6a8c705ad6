"""lddl_mlm_targets and the compact_mlm option of BertCollate / CodeCollate on
the GPU, bit for bit against tests/mlm_targets_model.py: the dense labels of
the same call define the result completely.

The bare call runs on hand-made labels (lane and wave edges, the chunk of the
offsets scan, more rows than one pass of the grid, both row layouts, the
capacity and every refusal), every output buffer with a guard region behind
it.  The routes run over a small hand-made row table (as
tests/test_wwm_gpu.py builds one) over the 'tiny64' vocabulary of
tests/synth_vocab.py: ids 5..30 are the letters, 31..56 their '##' forms;
[CLS] 2, [SEP] 3, [MASK] 4.
"""
import collections
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import mlm_targets_model as tm
import synth_vocab as sv
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -6
IGNORE = -1
GUARD = 16                        # entries behind each output that no call may touch
SENT64, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
BIG = (1 << 40) + 5               # a label that needs more than 32 bits


# ---- the bare call -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tok():
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(sv.vocab_path('tiny64'), 0)


def host(t):
  return t.cpu().numpy()


def ptr(t):
  return ctypes.c_void_p(0 if t is None else t.data_ptr())


Out = collections.namedtuple('Out', 'rc count positions target_labels offsets guards_ok')


def bare(labels, ignore=IGNORE, cu=None, capacity=None, ctx=True, **over):
  """lddl_mlm_targets itself; over: arguments given in place of what the labels' shape says"""
  labels = np.ascontiguousarray(labels, np.int64)
  n, S = (labels.shape if cu is None else (len(cu) - 1, 0))
  a = dict(n_rows=n, seq_len=S, total=labels.size)
  a.update(over)
  cap = labels.size if capacity is None else capacity
  flat = torch.from_numpy(labels.reshape(-1)).cuda()
  cu_t = None if cu is None else torch.tensor(cu, dtype=torch.int32).cuda()
  pos = torch.full((cap + GUARD,), SENT64, dtype=torch.int64, device='cuda')
  lab = torch.full((cap + GUARD,), SENT64, dtype=torch.int64, device='cuda')
  off = torch.full((n + 1 + GUARD,), SENT32, dtype=torch.int32, device='cuda')
  count = ctypes.c_int64(-7)
  torch.cuda.synchronize()
  rc = _lib.lib().lddl_mlm_targets(tok().handle if ctx else None, ptr(flat), a['n_rows'], a['seq_len'], ptr(cu_t),
                                   a['total'], ignore, cap, ptr(pos), ptr(lab), ptr(off), ctypes.byref(count), None)
  torch.cuda.synchronize()
  pos, lab, off = host(pos), host(lab), host(off)
  ok = (pos[cap:] == SENT64).all() and (lab[cap:] == SENT64).all() and (off[n + 1:] == SENT32).all()
  return Out(rc, count.value, pos[:cap], lab[:cap], off[:n + 1], bool(ok))


def check(labels, ignore=IGNORE, cu=None, capacity=None):
  """a call that succeeds: every entry of the three outputs is the model's, the padded tail included"""
  labels = np.ascontiguousarray(labels, np.int64)
  cap = labels.size if capacity is None else capacity
  o = bare(labels, ignore, cu, cap)
  t = tm.targets(labels, ignore, cu, cap)
  assert o.rc == 0, _lib.lib().lddl_last_error()
  assert o.count == t.count
  assert np.array_equal(o.offsets, t.offsets) and o.offsets.dtype == np.int32
  assert np.array_equal(o.positions, t.positions)
  assert np.array_equal(o.target_labels, t.target_labels)
  assert o.guards_ok
  return o


def random_labels(shape, p, ignore=IGNORE, seed=0):
  rng = np.random.default_rng(seed)
  lab = rng.integers(0, 30522, shape).astype(np.int64)  # 0 is a label
  lab[rng.random(shape) >= p] = ignore
  return lab


@pytest.mark.parametrize('selected', [True, False])
def test_one_element(gpu, selected):
  o = check([[17 if selected else IGNORE]])
  assert o.count == int(selected)


@pytest.mark.parametrize('ignore', [-1, -100])
@pytest.mark.parametrize('shape', [(2, 63), (3, 64), (3, 65), (2, 129)])
def test_lane_and_wave_edges(gpu, shape, ignore):
  lab = random_labels(shape, 0.3, ignore, seed=shape[1])
  lab[0, 0], lab[0, -1], lab[-1, 0], lab[-1, -1] = 0, 1, 2, 3  # the first and the last lane of a row's steps
  if shape[1] > 64:
    lab[0, 63], lab[0, 64] = 4, 5
  o = check(lab, ignore)
  assert 0 < o.count < lab.size
  assert (o.target_labels == 0).any()  # the label 0 is selected: only ignore_index is not
  if ignore == -100:
    lab[1, 1] = -1  # any value but ignore_index is a label, a negative one too
    o = check(lab, ignore)
    assert (o.target_labels == -1).any()


def test_an_empty_row_between_two_full_rows(gpu):
  lab = random_labels((3, 70), 1.0)
  lab[1] = IGNORE
  o = check(lab)
  assert o.offsets.tolist() == [0, 70, 70, 140]


def test_everything_and_nothing_selected(gpu):
  o = check(random_labels((3, 65), 1.0))
  assert o.count == 195 and np.array_equal(o.positions, np.arange(195))
  o = check(np.full((3, 65), IGNORE))
  assert o.count == 0 and not o.offsets.any()
  assert not o.positions.any() and (o.target_labels == IGNORE).all()


def test_many_steps_of_one_wave(gpu):
  check(random_labels((1, 4100), 0.3, seed=1))


def test_more_rows_than_a_chunk_of_the_scan(gpu):
  lab = random_labels((2050, 3), 0.4, seed=2)  # kChunk = 2048 rows per block of the offsets scan
  lab[2047], lab[2048], lab[2049] = [1, IGNORE, 2], [IGNORE, 3, IGNORE], [4, 5, 6]
  o = check(lab)
  assert o.offsets[2048] < o.offsets[2049] <= o.offsets[2050]


def test_more_rows_than_one_pass_of_the_grid(gpu):
  # the grid is capped at 8 blocks per CU x 4 rows per block: 8192 rows on 256 CUs
  lab = random_labels((8200, 2), 0.4, seed=3)
  lab[-1] = [7, 8]
  o = check(lab)
  assert o.positions[o.count - 1] == 2 * 8200 - 1


def test_a_label_beyond_32_bits_comes_back_intact(gpu):
  lab = np.full((2, 66), IGNORE, np.int64)
  lab[0, 3], lab[1, 65], lab[1, 0] = BIG, -BIG, (1 << 62) + 1
  o = check(lab)
  assert o.target_labels[:3].tolist() == [BIG, (1 << 62) + 1, -BIG]


# ---- the offsets layout --------------------------------------------------------------
def test_rows_at_odd_and_even_offsets(gpu):
  cu = [0, 3, 8, 9, 74, 139, 140, 269]  # rows of 3, 5, 1, 65, 65, 1 and 129 tokens
  o = check(random_labels(269, 0.4, seed=4), cu=cu)
  assert {c % 2 for c in cu[:-1]} == {0, 1} and o.count > 0


def test_empty_rows_first_in_the_middle_and_last(gpu):
  cu = [0, 0, 70, 70, 70, 75, 75]
  lab = random_labels(75, 0.5, seed=5)
  lab[0], lab[69], lab[70], lab[74] = 1, 2, 3, 4
  o = check(lab, cu=cu)
  assert o.offsets[0] == o.offsets[1] == 0 and o.offsets[2] == o.offsets[3] == o.offsets[4]
  assert o.offsets[5] == o.offsets[6] == o.count
  o = check(lab, cu=[0, 0, 0])  # only empty rows: legal, nothing selected
  assert o.count == 0


def test_tokens_behind_the_last_row_are_ignored(gpu):
  lab = random_labels(200, 1.0, seed=6)
  o = check(lab, cu=[0, 64, 130])
  assert o.count == 130 and o.positions[129] == 129
  o = check(lab, cu=[5, 64, 130])  # and in front of the first
  assert o.count == 125 and o.positions[0] == 5


def test_both_layouts_agree_when_the_rows_tile_the_tensor(gpu):
  lab = random_labels((5, 67), 0.3, seed=7)
  a = check(lab)
  b = check(lab.reshape(-1), cu=[67 * r for r in range(6)])
  assert np.array_equal(a.positions, b.positions) and np.array_equal(a.target_labels, b.target_labels)
  assert np.array_equal(a.offsets, b.offsets)


# ---- capacity ------------------------------------------------------------------------
def test_capacity(gpu):
  lab = random_labels((4, 70), 0.5, seed=8)
  M = int((lab != IGNORE).sum())
  assert M > 64
  check(lab, capacity=M)  # M == K
  o = check(lab, capacity=M + 5)
  assert o.positions[M:].tolist() == [0] * 5 and o.target_labels[M:].tolist() == [IGNORE] * 5
  o = bare(lab, capacity=M - 1)  # M == K + 1
  assert o.rc == ECAPACITY and o.count == M and o.guards_ok
  assert b'capacity' in _lib.lib().lddl_last_error()
  o = bare(lab, capacity=0)
  assert o.rc == ECAPACITY and o.count == M and o.guards_ok
  check(np.full((2, 5), IGNORE), capacity=0)  # M == K == 0
  check(lab)  # the ctx is as good as before


# ---- refusals ------------------------------------------------------------------------
GOOD = random_labels((3, 70), 0.3, seed=9)
REFUSALS = {
    'null ctx': dict(ctx=False),
    'ignore_index 0': dict(ignore=0),
    'ignore_index 7': dict(ignore=7),
    'n_rows 0': dict(n_rows=0),
    'n_rows -1': dict(n_rows=-1),
    'total != n * S': dict(total=209),
    'seq_len 0': dict(seq_len=0),
    'cu decreasing': dict(cu=[0, 100, 60, 210]),
    'cu[0] = -1': dict(cu=[-1, 70, 140, 210]),
    'cu[n] > total': dict(cu=[0, 70, 140, 211]),
    'cu[n] far beyond total': dict(cu=[0, 70, 140, (1 << 31) - 1]),
}


@pytest.mark.parametrize('case', list(REFUSALS))
def test_refusals(gpu, case):
  kw = dict(REFUSALS[case])
  lab = GOOD.reshape(-1) if 'cu' in kw else GOOD
  o = bare(lab, **kw)
  assert o.rc == EINVAL and o.guards_ok
  assert _lib.lib().lddl_last_error()
  if 'cu' not in kw:
    # refused on the host: no output is touched
    assert o.count == -7 and (o.positions == SENT64).all() and (o.offsets == SENT32).all()
  check(lab, cu=[0, 70, 140, 210] if 'cu' in kw else None)  # a good call on the same ctx


def test_null_outputs_are_refused(gpu):
  L, h = _lib.lib(), tok().handle
  lab = torch.from_numpy(GOOD).cuda()
  buf = torch.empty(GOOD.size, dtype=torch.int64, device='cuda')
  off = torch.empty(4, dtype=torch.int32, device='cuda')
  count = ctypes.c_int64()
  for outs in [(None, ptr(buf), ptr(off), ctypes.byref(count)), (ptr(buf), None, ptr(off), ctypes.byref(count)),
               (ptr(buf), ptr(buf), None, ctypes.byref(count)), (ptr(buf), ptr(buf), ptr(off), None)]:
    assert L.lddl_mlm_targets(h, ptr(lab), 3, 70, None, 210, IGNORE, 210, *outs, None) == EINVAL
  assert L.lddl_mlm_targets(h, None, 3, 70, None, 210, IGNORE, 210, ptr(buf), ptr(buf), ptr(off),
                            ctypes.byref(count), None) == EINVAL
  check(GOOD)


def test_the_same_call_twice_gives_the_same(gpu):
  lab = random_labels((300, 130), 0.15, seed=10)
  a, b = bare(lab), bare(lab)
  assert a.rc == b.rc == 0 and a.count == b.count
  for x, y in zip(a[2:5], b[2:5]):
    assert np.array_equal(x, y)


# ---- the routes ----------------------------------------------------------------------
def w(i):
  return 5 + i % 26


def plain(k, i=0):
  return [w(i + t) for t in range(k)]


def word(k, i=0):
  return [w(i)] + [31 + (i + t) % 26 for t in range(k - 1)]


CLS, SEP, MASK = 2, 3, 4
# (A / doc, B / code, s, is_random_next).  Columns: [CLS] 0, A 1 .. a, [SEP] a + 1, B from a + 2.
ROWS = [
    (plain(58) + word(6, 3) + plain(6, 7), plain(3, 2) + word(2, 5), 1, 0),  # 78 tokens: a word across columns 63 / 64
    (plain(3, 4), word(2, 9), 1, 1),                                         # 8
    (plain(1, 6), [], 1, 0),                                                 # 4
    (plain(30, 8), word(33, 1), 1, 1),                                       # 66
    ([], word(4, 2) + plain(6, 11), 0, 0),                                   # CodeBERT without docstring: 12
    (word(3, 5) + plain(1), plain(7, 3), 1, 0),                              # 14
]
BERT_ROWS = [0, 1, 2, 3, 1]
CODE_ROWS = [5, 4, 0, 4, 3]
P, SEED, COUNTER = 0.3, 77, 5
NEW_KEYS = {'masked_lm_positions', 'masked_lm_labels', 'masked_lm_offsets'}


def row_len(g):
  a, b, s, _ = ROWS[g]
  return len(a) + len(b) + 2 + s


def static_positions(g):
  return [1, row_len(g) - 2]


@functools.lru_cache(maxsize=None)
def table(static=False):
  """ROWS as a PackResult with spans; static: two static masks per row (the collates then default to mode 1)"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  n = len(ROWS)
  ids, src0, src1 = [0], [], []  # (an id in front: no span starts at 0)
  for a, b, _, _ in ROWS:
    src0.append(len(ids))
    ids += a
    src1.append(len(ids))
    ids += b
  lens = np.asarray([row_len(g) for g in range(n)], np.int64)

  def t(a, dt):
    a = np.ascontiguousarray(np.asarray(a, dt))
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t([len(r[0]) for r in ROWS], np.uint16), t([len(r[1]) for r in ROWS], np.uint16),
      t([r[2] * 2 + r[3] for r in ROWS], np.uint8), t(np.zeros(n), np.uint8), t(np.zeros(n), np.int64),
      t([[n]], np.int64))
  res.ids, res.src0, res.src1 = t(ids + [0] * 16, np.uint16), t(src0, np.int64), t(src1, np.int64)
  res.cls_id, res.sep_id = CLS, SEP
  if static:
    res.n_masked, res.mlm_off = 2 * n, t(2 * np.arange(n + 1), np.int64)
    res.mlm_pos = t(sum((static_positions(g) for g in range(n)), []), np.uint16)
    res.mlm_label, res.mlm_token = t([30, 29] * n, np.uint16), t([MASK] * (2 * n), np.uint16)
  return res


def make(kind, compact, wwm=False, align=8):
  from lddl_amd.loader import BertCollate, CodeCollate
  col = (CodeCollate if kind == 'code' else BertCollate)(tokenizer=tok(), sequence_length_alignment=align, base_seed=SEED,
                                                        mlm_probability=P, whole_word_mask=wwm, compact_mlm=compact)
  col.counter = COUNTER
  return col


def check_route(kind, run, wwm=False):
  """run(collate) -> batch.  The option adds the model's three tensors and changes nothing else."""
  plain_col, compact_col = make(kind, False, wwm), make(kind, True, wwm)
  a, b = run(plain_col), run(compact_col)
  assert plain_col.counter == compact_col.counter == COUNTER + 1
  assert set(b) - set(a) == NEW_KEYS and not set(a) & NEW_KEYS
  for k in a:
    assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
  cu = host(b['cu_seqlens']) if 'cu_seqlens' in b else None
  t = tm.targets(host(b['labels']), IGNORE, cu)
  assert t.count > 0
  assert np.array_equal(host(b['masked_lm_positions']), t.positions) and b['masked_lm_positions'].dtype == torch.int64
  assert np.array_equal(host(b['masked_lm_labels']), t.target_labels) and b['masked_lm_labels'].dtype == torch.int64
  assert np.array_equal(host(b['masked_lm_offsets']), t.offsets) and b['masked_lm_offsets'].dtype == torch.int32
  # what a trainer does with them: the labels gathered at the positions
  assert torch.equal(b['labels'].view(-1)[b['masked_lm_positions']], b['masked_lm_labels'])
  return b, t


@pytest.mark.parametrize('wwm', [False, True])
def test_collate_rows_dynamic(gpu, wwm):
  b, _ = check_route('bert', lambda col: col.collate_rows(table(), BERT_ROWS), wwm)
  assert tuple(b['labels'].shape) == (5, 80)


def test_collate_rows_static(gpu):
  b, t = check_route('bert', lambda col: col.collate_rows(table(True), BERT_ROWS))
  S = 80
  assert t.positions.tolist() == sum(([r * S + p for p in static_positions(g)] for r, g in enumerate(BERT_ROWS)), [])
  assert t.target_labels.tolist() == [30, 29] * 5 and t.offsets.tolist() == [0, 2, 4, 6, 8, 10]


@pytest.mark.parametrize('wwm', [False, True])
def test_collate_rows_unpadded_dynamic(gpu, wwm):
  b, _ = check_route('bert', lambda col: col.collate_rows_unpadded(table(), BERT_ROWS), wwm)
  assert b['labels'].dim() == 1 and b['labels'].numel() == sum(row_len(g) for g in BERT_ROWS)
  # the same rows padded: the same labels in the same order, and the same share per row
  pad = make('bert', True, wwm, align=1).collate_rows(table(), BERT_ROWS)
  assert torch.equal(pad['masked_lm_labels'], b['masked_lm_labels'])
  assert torch.equal(pad['masked_lm_offsets'], b['masked_lm_offsets'])


def text(ids):
  names = tok().ids_to_tokens
  return ' '.join(names[i] for i in ids)


def test_string_route_with_3_tuples(gpu):
  samples = [(text(ROWS[g][0]), text(ROWS[g][1]), bool(ROWS[g][3])) for g in BERT_ROWS]
  check_route('bert', lambda col: col(samples))


def test_string_route_with_5_tuples(gpu):
  samples = []
  for g in BERT_ROWS:
    bio = io.BytesIO()
    np.save(bio, np.asarray(static_positions(g), np.uint16))
    samples.append((text(ROWS[g][0]), text(ROWS[g][1]), bool(ROWS[g][3]), bio.getvalue(), text([30, 29])))
  _, t = check_route('bert', lambda col: col(samples))
  assert t.target_labels.tolist() == [30, 29] * 5


def test_code_collate_rows(gpu):
  check_route('code', lambda col: col.collate_rows(table(), CODE_ROWS))


def test_code_collate_rows_unpadded(gpu):
  check_route('code', lambda col: col.collate_rows_unpadded(table(), CODE_ROWS))


@pytest.mark.parametrize('kind', ['bert', 'code'])
def test_mask_tokens_then_mlm_targets(gpu, kind):
  rng = np.random.default_rng(11)
  ids = rng.integers(5, 57, (7, 66)).astype(np.int64)
  sp = (rng.random((7, 66)) < 0.1).astype(np.int64)
  col = make(kind, False)
  _, labels = col.mask_tokens(torch.from_numpy(ids).cuda(), torch.from_numpy(sp).cuda())
  pos, lab, off = col.mlm_targets(labels)
  t = tm.targets(host(labels), IGNORE)
  assert t.count > 0 and tuple(pos.shape) == tuple(lab.shape) == (t.count,)
  assert np.array_equal(host(pos), t.positions) and np.array_equal(host(lab), t.target_labels)
  assert np.array_equal(host(off), t.offsets)
  K = t.count + 9
  pos, lab, off = col.mlm_targets(labels, capacity=K)
  t = tm.targets(host(labels), IGNORE, capacity=K)
  assert tuple(pos.shape) == tuple(lab.shape) == (K,)
  assert np.array_equal(host(pos), t.positions) and np.array_equal(host(lab), t.target_labels)
  with pytest.raises(RuntimeError, match='capacity'):
    col.mlm_targets(labels, capacity=t.count - 1)


def test_mode_0_adds_nothing(gpu):
  col = make('bert', True)
  assert not NEW_KEYS & set(col.collate_rows(table(), BERT_ROWS, mode=0))
  assert not NEW_KEYS & set(col.collate_rows_unpadded(table(), BERT_ROWS, mode=0))
  assert not NEW_KEYS & set(col.to_encoded_inputs([(text(ROWS[1][0]), text(ROWS[1][1]), False)]))
  assert col.counter == COUNTER
  assert not NEW_KEYS & set(make('code', True).collate_rows(table(), CODE_ROWS, mode=0))


def test_a_fixed_capacity_gives_fixed_shapes(gpu):
  K = 5 * 80  # the batch's tokens
  b = make('bert', K).collate_rows(table(), BERT_ROWS)
  t = tm.targets(host(b['labels']), IGNORE, capacity=K)
  assert tuple(b['masked_lm_positions'].shape) == tuple(b['masked_lm_labels'].shape) == (K,)
  assert 0 < t.count < K
  assert np.array_equal(host(b['masked_lm_positions']), t.positions)
  assert np.array_equal(host(b['masked_lm_labels']), t.target_labels)
  assert np.array_equal(host(b['masked_lm_offsets']), t.offsets)
  T = sum(row_len(g) for g in BERT_ROWS)
  b = make('bert', T).collate_rows_unpadded(table(), BERT_ROWS)
  t = tm.targets(host(b['labels']), IGNORE, host(b['cu_seqlens']), capacity=T)
  assert tuple(b['masked_lm_positions'].shape) == (T,)
  assert np.array_equal(host(b['masked_lm_positions']), t.positions)
  assert np.array_equal(host(b['masked_lm_labels']), t.target_labels)
  col = make('bert', 1)  # too small: refused with the count in the message, and the counter has advanced as without it
  with pytest.raises(RuntimeError, match='capacity'):
    col.collate_rows(table(), BERT_ROWS)
  assert col.counter == COUNTER + 1
