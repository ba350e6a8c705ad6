"""The static-masking packer (pack_bert_wave_kernel<MASK = 1 | 2>) in every
regime of its create_masked_lm_predictions block, against the oracle: the
configurations of tests/mask_regimes.py (tests/test_mask_regimes_host.py shows
that each one reaches its regimes) packed on the GPU and compared by exact
equality -- masked A and B, is_random_next, num_tokens, positions, labels and
the per-partition bin counts -- on the lddl_masked_lm and the
lddl_masked_lm_spans routes, with the per-partition arrays in LDS
(LDDL_PACK_CAPS), and, for the rows no suite had produced before (no masked
position at all; every candidate masked), through the parquet writer, the
shard loader and a static collate."""
import io
import os

import numpy as np
import pytest
import torch

import mask_regimes as mr
from oracle import pack_oracle as po
from test_pack_gpu import shards_from_docs

pytestmark = pytest.mark.gpu


def pack(seq, ratio, spans):
  """a fresh Packer (its first masked-LM arena is the default one) -> (packer, result, oracle rows)"""
  from lddl_amd.pipeline import Packer, VOCAB_BERT
  docs, pdo, exp = mr.oracle_rows(seq, ratio)
  pk = Packer(VOCAB_BERT, 0)
  assert (pk.tok.cls_id, pk.tok.sep_id) == (mr.CLS, mr.SEP)
  sh, ids, ntok = shards_from_docs(docs, part_doc_off=pdo)
  res = pk.pack(sh, ids, ntok, target_seq_length=seq, duplicate_factor=mr.DUP, seed=mr.PACK_SEED, bin_size=seq // 4,
                masking=True, masked_lm_ratio=ratio, spans=spans)
  torch.cuda.synchronize()
  return pk, res, exp


def check(seq, ratio, spans):
  from lddl_amd.pipeline import assert_same_pairs
  pk, res, exp = pack(seq, ratio, spans)
  assert res.spans == spans
  assert_same_pairs(res, exp)  # A, B, is_random_next, num_tokens, positions, labels in the binned order
  assert res.n_masked == sum(len(r[4]) for part in exp for r in part)
  bc = res.bin_count.cpu().numpy()
  assert bc.shape == (mr.N_PART, 4)
  for p, part in enumerate(exp):
    assert np.array_equal(bc[p], np.bincount([po.bin_of(r[3], seq // 4, 4) for r in part], minlength=4)), p
  return pk, res, exp


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('seq,ratio', mr.CONFIGS)
def test_masked_regimes_vs_oracle(gpu, seq, ratio, spans):
  check(seq, ratio, spans)


@pytest.mark.parametrize('caps', ['8192,512,8192', '0,0,256'])
@pytest.mark.parametrize('seq,ratio', [(128, 0.15), (1024, 0.6)])
def test_masked_regimes_with_lds_arrays(gpu, monkeypatch, seq, ratio, caps):
  """the <1, true> and <2, true> instantiations: every per-partition array in
  LDS, and order / num_tokens alone with a capacity of 256 pairs (the seq-128
  partitions fit it, the seq-1024 ones do not)"""
  monkeypatch.setenv('LDDL_PACK_CAPS', caps)
  check(seq, ratio, False)


def test_default_arena_overshoots():
  """Without LDDL_MLM_CAP a pack's first masked-LM arena holds
  n_part * 4 * MLM_CHUNK + dup * n_sent * 4 entries.  The positions of
  (128, 0.15) and (128, 0.0) fit it; every other configuration's positions
  alone exceed it (the chunked allocation only adds to that), so those packs
  above ran twice: once overshooting, once into the regrown arena."""
  over = []
  for seq, ratio in mr.CONFIGS:
    docs, _, exp = mr.oracle_rows(seq, ratio)
    cap = mr.default_arena(sum(len(d) for d in docs))
    if sum(len(r[4]) for part in exp for r in part) > cap:
      over.append((seq, ratio))
  assert over == [c for c in mr.CONFIGS if c not in ((128, 0.15), (128, 0.0))]


def test_zero_position_and_fully_masked_rows_downstream(gpu, tmp_path):
  """(128, 1.0) as spans through write_shards, a parquet read, load_shards and
  a static collate_rows batch: rows without a masked position and rows whose
  every candidate is masked"""
  import pyarrow as pa
  import pyarrow.parquet as pq
  from lddl_amd import writer
  from lddl_amd.loader import BertCollate, load_shards
  seq, ratio = 128, 1.0
  pk, res, exp = check(seq, ratio, True)
  flat = [r for part in exp for r in part]
  zero = [g for g, r in enumerate(flat) if not r[4]]
  full = [g for g, r in enumerate(flat) if len(r[4]) == r[3] - 3 >= 100]
  assert zero and full
  writer.write_shards(pk, res, str(tmp_path), bin_size=seq // 4, masking=True)
  table = pa.concat_tables([pq.read_table(os.path.join(str(tmp_path), 'part.%d.parquet_%d' % (p, b)))
                            for p in range(mr.N_PART) for b in range(4)])
  d = table.to_pydict()
  assert table.num_rows == len(flat)
  with open(pk.tok.vocab_file, encoding='utf-8') as f:
    vocab = {l.rstrip('\n').rstrip('\r'): i for i, l in enumerate(f)}
  for g, r in enumerate(flat):
    pos = np.load(io.BytesIO(d['masked_lm_positions'][g]))
    assert pos.dtype == np.uint16 and pos.shape == (len(r[4]),) and pos.tolist() == r[4], g
    assert [vocab[t] for t in d['masked_lm_labels'][g].split()] == r[5], g
    assert d['num_tokens'][g] == r[3] and d['is_random_next'][g] == r[2], g
  # the shards as a GPU row table, then one static batch that holds both kinds of row
  col = BertCollate(tokenizer=pk.tok, sequence_length_alignment=8)
  got = load_shards(col, str(tmp_path))
  assert got.n_pairs == len(flat) and got.n_masked == res.n_masked
  idx = zero[:3] + full[:3] + list(range(0, len(flat), 7))
  out = col.collate_rows(got, idx, mode=1)
  S = (max(flat[g][3] for g in idx) + 7) // 8 * 8
  ids = np.zeros((len(idx), S), np.int64)
  labels = np.full((len(idx), S), -1, np.int64)
  for k, g in enumerate(idx):
    ma, mb, _, n, pos, lab = flat[g][:6]
    ids[k, :n] = [mr.CLS] + ma + [mr.SEP] + mb + [mr.SEP]
    labels[k, pos] = lab
  assert not (labels[:3] != -1).any() and ((labels[3:6] != -1).sum(1) >= 100).all()
  assert np.array_equal(out['labels'].cpu().numpy(), labels)
  assert np.array_equal(out['input_ids'].cpu().numpy(), ids)
  assert np.array_equal(out['next_sentence_labels'].cpu().numpy(), [int(flat[g][2]) for g in idx])
