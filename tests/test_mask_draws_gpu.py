"""Every dynamic-masking route equals tests/mask_model.py bit for bit.

The four kernels that draw (mask_tokens_kernel and collate_fill_kernel of
collate.hip, the fills of collate_rows.hip and collate_unpadded.hip) inline
one device function, so the suite's kernel-against-kernel tests move together
when it is wrong.  Here each route is held to the numpy model of the
documented draw (include/lddl_amd.h at lddl_mask_tokens) with np.array_equal
on input_ids and labels; tests/test_mask_model_host.py holds the model.

What the shapes and values are for:

* lddl_mask_tokens at (1, 1), (1, 63), (3, 64), (2, 65): one element, one
  short of a wave, whole waves, one over; a thread's (row, col) comes from a
  division of the flat index, which a row length of 65 exercises.
  (1, 2^20 - 1): the widest row the index has bits for (col must not spill
  into the row's bits).  (4099, 257): rows >= 4096, where row << 20 passes
  2^32, and more elements than one pass of the grid, so the grid-stride loop
  runs (asserted from the device's CU count).
* seeds {0, 1, 12345, 2^63, 2^64 - 1} x counters {0, 1, 2^32, 2^64 - 1}: either
  half of either word lost on the way through ctypes or the kernel arguments,
  the counter not hashed, seed and counter not mixed.
* p in {0, 2^-53, 0.15, 0.5, 1 - 2^-53, 1}: the comparison is with a double of
  53 bits, not a float or a rounded integer threshold.
* ignore_index in {-100, -1, 2^31 - 1}; input ids 0, [MASK] itself, the last
  id, 2^40 + 7 and -5: kept ids and labels are 64-bit and signed.
* special_tokens_mask values 0, 1, 2, -1, 2^32: nonzero in any bit is special.
* vocabularies of 5, 6, 64 and 65 entries and CodeBERT's 52 000: the random
  word is below len(tokenizer) and reaches len(tokenizer) - 1.
* string route and row tables: rows of 3, 4, 63, 64, 65 and 2048 tokens
  (a = b = 0, the wave width and its neighbours, the LDS row's limit), padded
  at alignment 1 (odd widths take the 8-B stores of collate_rows) and 8, pad
  columns never selected; more rows than one pass of the fill's grid; index
  lists in descending order with repeats (the draw is keyed by the row of the
  batch, not of the table); the row0 / n_rows form; for the padding-free
  batch the column is the token's position in its row.
* three batches in a row and a RowBatches epoch: the counter a batch draws
  with is the number of batches before it.
"""
import functools

import numpy as np
import pytest
import torch

import mask_model as mm
import synth_vocab as sv
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
SEEDS = [0, 1, 12345, 1 << 63, M64]
COUNTERS = [0, 1, 1 << 32, M64]
PROBS = [0.0, 2.0 ** -53, 0.15, 0.5, 1 - 2.0 ** -53, 1.0]
IGNORES = [-100, -1, (1 << 31) - 1]
BIG_ID = (1 << 40) + 7
SPECIAL_VALUES = np.asarray([0, 0, 0, 0, 0, 0, 1, 2, -1, 1 << 32, 0], np.int64)


@functools.lru_cache(maxsize=None)
def tokenizer(path=_lib.VOCAB_BERT):
  from lddl_amd.tokenizer import Tokenizer
  return Tokenizer(path, 0)


def collate(path=_lib.VOCAB_BERT, align=8, **kw):
  from lddl_amd.loader import BertCollate
  return BertCollate(tokenizer=tokenizer(path), sequence_length_alignment=align, **kw)


def model(col, ids, special, counter, rows=None, cols=None):
  return mm.mask(ids, special, col.seed, counter, col.mlm_probability, col.tok.mask_id, col.tok.vocab_size,
                 col.ignore_index, rows, cols)


def assert_equals_model(ids, labels, m, what=''):
  ids = ids.cpu().numpy() if torch.is_tensor(ids) else ids
  labels = labels.cpu().numpy() if torch.is_tensor(labels) else labels
  assert ids.dtype == np.int64 and labels.dtype == np.int64
  assert ids.shape == m.input_ids.shape and labels.shape == m.labels.shape, (what, ids.shape, m.input_ids.shape)
  bad = int((ids != m.input_ids).sum()), int((labels != m.labels).sum())
  assert np.array_equal(ids, m.input_ids) and np.array_equal(labels, m.labels), \
      '%s: %d input ids and %d labels of %d differ from the model' % (what, bad[0], bad[1], ids.size)


# ---- lddl_mask_tokens ----------------------------------------------------------------
def plane(shape, V, mask_id):
  """(ids, special_tokens_mask): random ids in [0, V) with 2^40 + 7, 0, the
  [MASK] id, V - 1 and -5 at every third element in turn; every value of
  SPECIAL_VALUES in turn.  Element 0 is 2^40 + 7 and not special"""
  n = shape[0] * shape[1]
  k = np.arange(n)
  edge = np.asarray([BIG_ID, 0, mask_id, V - 1, -5], np.int64)
  ids = np.where(k % 3 == 0, edge[(k // 3) % 5], np.random.default_rng(n).integers(0, V, n))
  return ids.astype(np.int64).reshape(shape), SPECIAL_VALUES[(k * 7 + 3) % 11].reshape(shape)


def run_mask_tokens(col, ids, special, counter):
  t = torch.from_numpy(ids).to(col.device)
  out, labels = col.mask_tokens(t, torch.from_numpy(special).to(col.device), counter=counter)
  assert out.data_ptr() == t.data_ptr()  # in place
  return out.cpu().numpy(), labels.cpu().numpy()


@pytest.mark.parametrize('shape', [(1, 1), (1, 63), (3, 64), (2, 65)])
def test_mask_tokens_every_seed_counter_and_probability(gpu, shape):
  tok = tokenizer()
  ids, special = plane(shape, tok.vocab_size, tok.mask_id)
  k = 0
  for seed in SEEDS:
    for counter in COUNTERS:
      for p in PROBS:
        col = collate(base_seed=seed, mlm_probability=p, ignore_index=IGNORES[k % 3])
        k += 1
        assert col.seed == seed
        got = run_mask_tokens(col, ids, special, counter)
        assert_equals_model(got[0], got[1], model(col, ids, special, counter), (shape, seed, counter, p))


# (seed, counter, p, ignore_index): every p and every ignore_index once, the edge seeds and counters in turn
BIG_CASES = [(M64, 1 << 32, 0.0, -100), (1 << 63, M64, 2.0 ** -53, -1), (12345, 0, 0.15, (1 << 31) - 1),
             (1, 1 << 32, 0.5, -100), (1 << 63, 1, 1 - 2.0 ** -53, -1), (0, M64, 1.0, (1 << 31) - 1)]


@pytest.mark.parametrize('shape', [(1, (1 << 20) - 1), (4099, 257)])
def test_mask_tokens_widest_row_and_second_grid_pass(gpu, shape):
  tok = tokenizer()
  n_cu = torch.cuda.get_device_properties(0).multi_processor_count
  if shape[0] > 1:
    assert shape[0] * shape[1] > n_cu * 16 * 256 and shape[0] > 4096  # one pass of the grid is n_cu * 16 blocks of 256
  ids, special = plane(shape, tok.vocab_size, tok.mask_id)
  for seed, counter, p, ignore in BIG_CASES:
    col = collate(base_seed=seed, mlm_probability=p, ignore_index=ignore)
    got = run_mask_tokens(col, ids, special, counter)
    m = model(col, ids, special, counter)
    assert_equals_model(got[0], got[1], m, (shape, seed, counter, p))
    if p == 0.5:  # 64-bit and negative ids come back whole, kept and as labels; every kind of special is left alone
      kept = m.select & ~m.masked & ~m.random
      for v in (BIG_ID, -5):
        assert (got[0][kept] == v).any() and (got[1][m.masked] == v).any()
      for v in (1, 2, -1, 1 << 32):
        assert (got[1][special == v] == ignore).all() and np.array_equal(got[0][special == v], ids[special == v])
      assert (got[0][m.random] < tok.vocab_size).all() and (got[0][m.random] >= 0).all()


@pytest.mark.parametrize('name', ['tiny5', 'tiny6', 'tiny64', 'tiny65', 'codebert'])
def test_small_and_large_vocabularies(gpu, name):
  """every column selected (p = 1) on a 64 x 257 plane: about 1 600 random words"""
  path = _lib.VOCAB_CODEBERT if name == 'codebert' else sv.vocab_path(name)
  tok = tokenizer(path)
  V = 52000 if name == 'codebert' else sv.vocab_size(name)
  assert tok.vocab_size == V
  ids, special = plane((64, 257), V, tok.mask_id)
  special = np.zeros_like(special)
  col = collate(path, base_seed=1 << 63, mlm_probability=1.0, ignore_index=-100)
  got = run_mask_tokens(col, ids, special, 1 << 32)
  m = model(col, ids, special, 1 << 32)
  assert_equals_model(got[0], got[1], m, name)
  words = got[0][m.random]
  assert len(words) > 1400 and words.min() >= 0 and words.max() < V
  if V <= 65:
    assert words.min() == 0 and words.max() == V - 1 and len(np.unique(words)) == V  # the top id is reached
  else:
    assert (0xFFFFFFFF * V) >> 32 == V - 1 and words.max() > V * 0.99


# ---- the string route: BertCollate.__call__ --------------------------------------------
ROW_LENGTHS = [3, 4, 63, 64, 65, 2048]


def sample(tok, rng, n_tokens, a=None):
  """a 3-field sample of n_tokens = len(A) + len(B) + 3 tokens"""
  m = n_tokens - 3
  a = int(rng.integers(0, m + 1)) if a is None else a
  words = [tok.ids_to_tokens[int(i)] for i in rng.integers(1000, tok.vocab_size, m)]
  return (' '.join(words[:a]), ' '.join(words[a:]), bool(rng.integers(0, 2)))


def check_string_batch(col, batch, counter):
  """col(batch) at `counter` against the model over to_encoded_inputs of the same batch"""
  enc = col.to_encoded_inputs(batch)
  ids, special = enc['input_ids'].cpu().numpy(), enc['special_tokens_mask'].cpu().numpy()
  col.counter = counter
  out = col(batch)
  assert col.counter == (counter + 1)
  m = model(col, ids, special, counter)
  assert_equals_model(out['input_ids'], out['labels'], m, 'string route')
  pad = out['attention_mask'].cpu().numpy() == 0
  assert not m.select[pad].any() and (special[pad] == 1).all()
  assert (out['labels'].cpu().numpy()[pad] == col.ignore_index).all() and (out['input_ids'].cpu().numpy()[pad] == 0).all()
  for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
    assert torch.equal(out[k], enc[k]), k
  return out, m


@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('p,ignore', [(0.15, -1), (1.0, -100)])
def test_string_route(gpu, align, p, ignore):
  tok = tokenizer()
  rng = np.random.default_rng(17)
  rows = [sample(tok, rng, n, a=0 if n == 4 else None) for n in ROW_LENGTHS]
  col = collate(align=align, base_seed=1 << 63, mlm_probability=p, ignore_index=ignore)
  for pick, width in (([0, 1, 2, 3, 4, 5], 2048), ([4, 0, 1, 2], 65), ([2, 1, 0], 63), ([0], 3)):
    out, m = check_string_batch(col, [rows[g] for g in pick], 1 << 32)
    assert out['input_ids'].shape == (len(pick), (width + align - 1) // align * align)
    assert m.select.any() == (width > 3)  # a row of 3 tokens has no candidate


def test_string_route_more_rows_than_one_pass_of_the_grid(gpu):
  """the fill's grid is capped at 8 blocks of 4 rows per CU: beyond that a wave
  takes several rows; batch rows >= 4096 put row << 20 past 2^32"""
  tok = tokenizer()
  n = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
  assert n > 4096
  rng = np.random.default_rng(23)
  few = [sample(tok, rng, int(k)) for k in rng.integers(3, 7, 97)]
  batch = [few[i % 97] for i in range(n)]
  out, m = check_string_batch(collate(align=1, base_seed=M64, mlm_probability=0.5), batch, M64)
  lab = out['labels'].cpu().numpy()
  # the same sample at batch rows i and i + 97 draws differently: the first and the last pass of the grid differ
  assert not np.array_equal(lab[:97], lab[97:194]) and not np.array_equal(lab[:97], lab[n - 97:])


# ---- row tables: collate_rows and collate_rows_unpadded -----------------------------
N_IDS = 2101
# (src0, a, src1, b, is_random_next): n = a + b + 3 = ROW_LENGTHS
SHAPES = [(0, 0, 0, 0, 1), (3, 1, 11, 0, 0), (1, 30, 41, 30, 0), (0, 31, 100, 30, 1), (7, 31, 101, 31, 0),
          (17, 1022, 1041, 1023, 1)]
# descending with repeats (the 65-token row at batch rows 1 and 2); the same without the 2048-token row, so that
# alignment 1 gives an odd width; the ascending range as row0 / n_rows
SELECTIONS = [({'rows': [5, 4, 4, 3, 2, 1, 1, 0]}, 2048), ({'rows': [4, 4, 3, 2, 2, 1, 0, 0]}, 65),
              ({'rows': [2, 1, 0]}, 63), ({'row0': 1, 'n_rows': 4}, 65), ({'row0': 0}, 2048)]


@functools.lru_cache(maxsize=None)
def hand_made():
  """a PackResult over hand-made ids and span tables (no static masks), built
  as tests/test_collate_rows_gpu.py::hand_made builds its own"""
  from lddl_amd import pipeline
  dev = torch.device('cuda', 0)
  tok = tokenizer()
  ids = np.concatenate([1000 + np.arange(N_IDS), np.zeros(16, np.int64)]).astype(np.uint16)
  sp = np.asarray(SHAPES, np.int64)
  n = len(SHAPES)
  lens = sp[:, 1] + sp[:, 3] + 3
  assert lens.tolist() == ROW_LENGTHS
  assert all(s0 + a <= N_IDS and s1 + b <= N_IDS for s0, a, s1, b, _ in SHAPES)

  def t(a, dt=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.astype(dt or a.dtype)).to(dev)
  res = pipeline.PackResult(
      n, int(lens.sum()), 1, None, t(np.concatenate([[0], np.cumsum(lens)]), np.int64),
      t(sp[:, 1].astype(np.uint16)), t(sp[:, 3].astype(np.uint16)), t((sp[:, 4] | 2).astype(np.uint8)),
      t(np.zeros(n, np.uint8)), t(np.zeros(n, np.int64)), t(np.asarray([[n]], np.int64)))
  res.ids, res.src0, res.src1 = t(ids), t(sp[:, 0]), t(sp[:, 2])
  res.cls_id, res.sep_id = tok.cls_id, tok.sep_id
  return res


def check_rows_batch(col, res, sel, counter):
  """collate_rows(mode=2) at `counter` against the model over mode 0 of the same call"""
  enc = col.collate_rows(res, mode=0, **sel)
  col.counter = counter
  out = col.collate_rows(res, mode=2, **sel)
  assert col.counter == counter + 1
  ids, special = enc['input_ids'].cpu().numpy(), enc['special_tokens_mask'].cpu().numpy()
  m = model(col, ids, special, counter)
  assert_equals_model(out['input_ids'], out['labels'], m, ('collate_rows', sel))
  pad = out['attention_mask'].cpu().numpy() == 0
  assert not m.select[pad].any() and (out['labels'].cpu().numpy()[pad] == col.ignore_index).all()
  for k in ('token_type_ids', 'attention_mask', 'next_sentence_labels'):
    assert torch.equal(out[k], enc[k]), k
  return out, m


def check_unpadded_batch(col, res, sel, counter):
  """collate_rows_unpadded(mode=2): token t of batch row r is the model's (r, t - cu_seqlens[r])"""
  enc = col.collate_rows_unpadded(res, mode=0, **sel)
  col.counter = counter
  out = col.collate_rows_unpadded(res, mode=2, **sel)
  assert col.counter == counter + 1
  cu = enc['cu_seqlens'].cpu().numpy().astype(np.int64)
  lens = np.diff(cu)
  rows = np.repeat(np.arange(len(lens)), lens)
  cols = np.arange(cu[-1]) - cu[rows]
  assert np.array_equal(cols, out['position_ids'].cpu().numpy()) and torch.equal(out['cu_seqlens'], enc['cu_seqlens'])
  m = model(col, enc['input_ids'].cpu().numpy(), enc['special_tokens_mask'].cpu().numpy(), counter, rows, cols)
  assert_equals_model(out['input_ids'], out['labels'], m, ('collate_rows_unpadded', sel))
  return out, m, cu


@pytest.mark.parametrize('align', [1, 8])
@pytest.mark.parametrize('k', range(len(SELECTIONS)))
def test_collate_rows(gpu, align, k):
  res = hand_made()
  sel, width = SELECTIONS[k]
  col = collate(align=align, base_seed=1 << 63, mlm_probability=0.5, ignore_index=-100)
  out, m = check_rows_batch(col, res, sel, 1 << 32)
  assert out['input_ids'].shape[1] == (width + align - 1) // align * align
  if k == 1:  # one table row at two batch rows: the same ids, other draws
    lab = out['labels'].cpu().numpy()
    assert not np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[3], lab[4])


@pytest.mark.parametrize('k', range(len(SELECTIONS)))
def test_collate_rows_unpadded(gpu, k):
  res = hand_made()
  sel, _ = SELECTIONS[k]
  col = collate(align=8, base_seed=M64, mlm_probability=0.5, ignore_index=(1 << 31) - 1)
  out, m, cu = check_unpadded_batch(col, res, sel, M64)
  if k == 1:
    lab = out['labels'].cpu().numpy()
    assert cu[1] - cu[0] == cu[2] - cu[1] == 65 and not np.array_equal(lab[cu[0]:cu[1]], lab[cu[1]:cu[2]])
  # and it is the padded batch without its padding, against the model on both sides
  pad, _ = check_rows_batch(collate(align=1, base_seed=M64, mlm_probability=0.5, ignore_index=(1 << 31) - 1), res, sel, M64)
  keep = pad['attention_mask'].bool()
  assert torch.equal(pad['input_ids'][keep], out['input_ids']) and torch.equal(pad['labels'][keep], out['labels'])


def test_row_tables_more_rows_than_one_pass_of_the_grid(gpu):
  """both fills are capped at 8 blocks of 4 rows per CU; batch rows >= 4096"""
  res = hand_made()
  n = 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
  assert n > 4096
  idx = np.asarray([4, 3, 2, 1, 0])[np.random.default_rng(1).integers(0, 5, n)]
  sel = {'rows': torch.from_numpy(idx).to('cuda')}
  check_rows_batch(collate(align=1, base_seed=12345, mlm_probability=0.15), res, sel, 1 << 32)
  check_unpadded_batch(collate(base_seed=12345, mlm_probability=0.15), res, sel, 1 << 32)


def test_load_rows_into_collate_rows(gpu):
  """the table that load_rows makes of 3-field samples, collated in descending
  order with a repeat, against the model over the string route's mode 0 of the
  same samples in that order"""
  tok = tokenizer()
  rng = np.random.default_rng(29)
  samples = [sample(tok, rng, n, a=0 if n == 4 else None) for n in ROW_LENGTHS]
  col = collate(align=8, base_seed=1 << 63, mlm_probability=0.5, ignore_index=-100)
  res = col.load_rows(samples)
  pick = [5, 4, 4, 3, 2, 1, 1, 0]
  enc = col.to_encoded_inputs([samples[g] for g in pick])
  col.counter = M64
  out = col.collate_rows(res, pick)  # no static masks: dynamic by default
  m = model(col, enc['input_ids'].cpu().numpy(), enc['special_tokens_mask'].cpu().numpy(), M64)
  assert_equals_model(out['input_ids'], out['labels'], m, 'load_rows')
  assert m.select.any() and torch.equal(out['attention_mask'], enc['attention_mask'])


# ---- the counter a batch draws with --------------------------------------------------
def test_three_batches_in_a_row(gpu):
  """__call__ and collate_rows advance one counter, one per batch, across 2^32"""
  tok = tokenizer()
  res = hand_made()
  rng = np.random.default_rng(31)
  batch = [sample(tok, rng, n) for n in (63, 64, 65, 4)]
  col = collate(align=8, base_seed=12345, mlm_probability=0.5)
  enc = col.to_encoded_inputs(batch)
  enc_rows = col.collate_rows(res, [4, 3, 2], mode=0)
  c0 = (1 << 32) - 2
  col.counter = c0
  outs = [col(batch) for _ in range(3)] + [col.collate_rows(res, [4, 3, 2]) for _ in range(3)]
  assert col.counter == c0 + 6
  for i, out in enumerate(outs):
    e = enc if i < 3 else enc_rows
    m = model(col, e['input_ids'].cpu().numpy(), e['special_tokens_mask'].cpu().numpy(), c0 + i)
    assert_equals_model(out['input_ids'], out['labels'], m, 'batch %d' % i)
  assert not torch.equal(outs[0]['labels'], outs[1]['labels']) and not torch.equal(outs[3]['labels'], outs[4]['labels'])


def test_row_batches_epoch(gpu):
  """a RowBatches epoch on a new BertCollate: batch b draws with counter b"""
  from lddl_amd.loader import RowBatches
  res = hand_made()
  col = collate(align=1, base_seed=1 << 63, mlm_probability=0.5)
  labels = []
  for b, idx in enumerate(RowBatches(res, 2, seed=5)):
    assert col.counter == b
    enc = col.collate_rows(res, idx, mode=0)  # draws nothing, counts nothing
    out = col.collate_rows(res, idx)
    m = model(col, enc['input_ids'].cpu().numpy(), enc['special_tokens_mask'].cpu().numpy(), b)
    assert_equals_model(out['input_ids'], out['labels'], m, 'batch %d' % b)
    labels.append(out['labels'])
  assert col.counter == 3 == len(labels)
