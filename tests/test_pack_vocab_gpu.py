"""Static masking over vocabularies of other sizes than bert-base-uncased's
30522 (tests/synth_vocab.py): WaveRng::mlm_choices / randbelow
(lddl_amd/csrc/pack_wave.hip) draw 32 - clz(V) bits and reject words >= V, so
V = 5 and 6 (3 bits, shift 29), 64 (7 bits, half of the draws rejected), 65,
32768 (16 bits, half rejected), 32769 and 65535 take other rejection rates,
pick distances and jump-table walks than every other masking test.  End to
end against oracle/pack_oracle.py (CPython's random: exact for any V), as
tests/test_pack_gpu.py::test_bert_masked_end_to_end_vs_oracle."""
import functools

import numpy as np
import pytest

import synth_vocab as sv
from oracle import pack_oracle as po
from oracle.oracle import OracleTokenizer, lib

pytestmark = pytest.mark.gpu

# V -> masked_lm_ratio (each V at one ratio; both ratios at small, power-of-two and large sizes)
RATIO = {5: 0.5, 6: 0.15, 64: 0.5, 65: 0.15, 32768: 0.15, 32769: 0.5, 65535: 0.15}
RATIO['dupspecial'] = 0.15  # [MASK], [SEP] and [UNK] on two lines each: the later ids are the specials
SEED = 2718


def vocab_name(v):
  return v if isinstance(v, str) else 'tiny%d' % v if v < 100 else 'v%d' % v


@functools.lru_cache(maxsize=None)
def corpus(seq):
  from lddl_amd import synth
  return synth.make_wiki(200_000, seed=1000 + seq)


@functools.lru_cache(maxsize=None)
def expected(v, seq, nparts):
  """the oracle's rows per partition, unbinned, and the mask tuple read from the vocabulary"""
  from lddl_amd import pipeline
  c = corpus(seq)
  path = sv.vocab_path(vocab_name(v))
  ot = OracleTokenizer(path)
  # the lines of the file: what the product draws random tokens below (with duplicate lines the
  # reference's vocab_words is shorter and not in id order; neither the product nor the oracle models that)
  nv = lib().orc_tok_vocab_size(ot.h)
  assert nv == sv.vocab_size(vocab_name(v)) and (isinstance(v, str) or nv == v)
  pad, unk, cls, sep, msk = (lib().orc_tok_special_id(ot.h, k) for k in range(5))
  mask = (RATIO[v], nv, cls, sep, msk)
  oids, ontok = ot.run(c.data, c.sent_off, 512, nthreads=8)
  pdo = pipeline.partition_by_bytes(c, nparts)
  return po.run_bert_shards(c, oids, ontok, pdo, seq, 0.1, 5, SEED, None, masking=mask), ontok, mask, unk, tuple(pdo)


@pytest.mark.parametrize('seq,bin_size,nparts', [(128, 32, 5), (512, 64, 3)])
@pytest.mark.parametrize('v', sorted(k for k in RATIO if not isinstance(k, str)) + ['dupspecial'])
def test_masked_other_vocab_sizes_vs_oracle(gpu, v, seq, bin_size, nparts):
  from lddl_amd import pipeline
  rows, ontok, mask, unk, pdo = expected(v, seq, nparts)
  c = corpus(seq)
  nbins = seq // bin_size
  for spans in (True, False):
    for binned in (False, True):
      res = pipeline.run_bert(c, vocab_file=sv.vocab_path(vocab_name(v)), target_seq_length=seq,
                              bin_size=bin_size if binned else None, n_partitions=nparts, seed=SEED, check_host=True,
                              masking=True, masked_lm_ratio=RATIO[v], spans=spans)
      assert res.spans == spans and tuple(res.part_doc_off) == pdo
      assert np.array_equal(res.ntok_host, ontok)
      exp = rows
      if binned:
        exp = [[part[i] for i in po.binned_order([r[3] for r in part], bin_size, nbins)[0]] for part in rows]
      pipeline.assert_same_pairs(res, exp)
      got = res.rows()
      assert (res.cls_id, res.sep_id) == mask[2:4]
      assert all(r[5][0] == mask[2] and r[5][-1] == mask[3] for r in got)  # this vocabulary's [CLS] and [SEP]
      assert res.n_masked == sum(len(r[4]) for part in rows for r in part) > 0
      labels = {x for r in got for x in r[7]}
      shown = {r[5][q] for r in got for q in r[6]}
      assert max(labels | shown) < mask[1]
      if v == 'dupspecial':  # HF's ids of the repeated specials (tests/golden/vocab_lines_hf.json)
        import json
        import os
        from conftest import GOLDEN
        hf = json.load(open(os.path.join(GOLDEN, 'vocab_lines_hf.json')))['dupspecial:special_ids']
        assert [unk, mask[2], mask[3], mask[4]] == hf[1:] and mask[4] in shown and unk in labels
      if v == 5:  # every word is [UNK]: rows still pack, every label is [UNK]
        assert labels == {unk} and mask[4] in shown


def test_masking_refuses_vocab_of_65536(gpu):
  """ids are 16-bit and 0xFFFF is taken: masking needs V <= 65535 (EINVAL,
  'masking: vocab larger than 65535'); the refused call leaves its result
  empty, and the same vocabulary packs without masking"""
  from lddl_amd import pipeline
  c = corpus(128)
  pk = pipeline.Packer(sv.vocab_path('v65536'), 0, masking=True)
  assert pk.tok.vocab_size == 65536
  sh = pipeline.upload(c, pipeline.partition_by_bytes(c, 2), 'cuda')
  ids, ntok, toff = pk.tokenize(sh)
  with pytest.raises(RuntimeError, match='vocab larger than 65535'):
    pk.pack(sh, ids, ntok, toff, target_seq_length=128, seed=SEED, bin_size=32, masking=True)
  assert pk.result.rows() == -1
  res = pk.pack(sh, ids, ntok, toff, target_seq_length=128, seed=SEED, bin_size=32, masking=False)
  assert pk.result.rows() == res.n_pairs > 0
  with pytest.raises(RuntimeError, match='vocab larger than 65535'):
    pk.pack(sh, ids, ntok, toff, target_seq_length=128, seed=SEED, bin_size=32, masking=True)
  assert pk.result.rows() == res.n_pairs  # an argument error: the earlier result stands


@pytest.mark.parametrize('spans', [False, True])
@pytest.mark.parametrize('name', ['specials', 'long_a', 'blanks'])
def test_rendered_strings_of_synthetic_vocab(gpu, golden, tmp_path, name, spans):
  """lddl_render_strings / the writer over rinfo + rpool of another vocabulary:
  the string columns of a small packed shard are ' '.join(vocab[i]) of the
  oracle's rows -- entries of 200 bytes, '##' pieces, specials at odd ids,
  duplicate lines (each id renders its own line), trimmed lines"""
  import os
  import pyarrow.parquet as pq
  from lddl_amd import pipeline, writer
  from lddl_amd.synth import corpus_from_sentences
  data, off, _, _ = sv.load_golden(golden, name)
  sents = [sv.sentence_text(data, off, i) for i in range(len(off) - 1) if i % 2 == 0 or i < 200][:400]
  c = corpus_from_sentences(sents, list(range(0, len(sents), 8)) + [len(sents)])
  pdo = pipeline.partition_by_bytes(c, 2)
  path = sv.vocab_path(name)
  pk = pipeline.Packer(path, 0)
  res = pk.run(pipeline.upload(c, pdo, gpu), target_seq_length=128, bin_size=32, seed=7, spans=spans)
  writer.write_shards(pk, res, str(tmp_path), bin_size=32, batch_rows=300)
  oids, ontok = OracleTokenizer(path).run(c.data, c.sent_off, 512)
  exp = po.run_bert_shards(c, oids, ontok, pdo, 128, 0.1, 5, 7, 32)
  vocab = pk.tok.ids_to_tokens
  if name == 'blanks':  # HF's token -> id map of the trimmed lines
    import json
    from conftest import GOLDEN
    hf = json.load(open(os.path.join(GOLDEN, 'vocab_lines_hf.json')))[name]
    assert all(vocab[i] == t for t, i in hf.items()) and set(vocab) == set(hf)
  else:
    assert '\n'.join(vocab).encode() == sv.vocab_bytes(name).rstrip(b'\n')
  seen = set()
  for p, rows in enumerate(exp):
    for b in range(4):
      got = pq.read_table(os.path.join(str(tmp_path), 'part.%d.parquet_%d' % (p, b))).to_pydict()
      want = [r for r in rows if po.bin_of(r[3], 32, 4) == b]
      assert got['A'] == [' '.join(vocab[i] for i in r[0]) for r in want]
      assert got['B'] == [' '.join(vocab[i] for i in r[1]) for r in want]
      assert got['num_tokens'] == [r[3] for r in want]
      seen.update(i for r in want for i in r[0] + r[1])
  assert any(vocab[i].startswith('##') for i in seen)
  if name == 'long_a':
    assert max(len(vocab[i].encode()) for i in seen) >= 200
  if name == 'specials':
    assert {pk.tok.unk_id, vocab.index('dup', 100)} <= seen
