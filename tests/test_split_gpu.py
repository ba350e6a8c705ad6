"""The GPU sentence split (lddl_split_len / lddl_split, lddl_amd/csrc/split.hip,
lddl_amd/splitgpu.py) against the host path it replaces,
preprocess.split_records with the rule-based splitter, in both modes: the
sentence bytes, the 16 zero bytes behind them, sent_off, doc_sent_off and the
ids are equal on the record families of tests/split_model.py -- adversarial,
random code points, edge, synthetic Wikipedia, every hand-made structure
shifted through the 64-byte steps and a piece boundary, degenerate records --
a 3 MB record against the byte-level model, two ctxs, one ctx reused with
another size, a non-default stream, and the result fed to Packer.run."""
import functools

import numpy as np
import pytest
import torch

import split_model as M

pytestmark = pytest.mark.gpu

MODES = [pytest.param(False, id='id_body'), pytest.param(True, id='whole_line')]


@pytest.fixture(scope='module')
def tok(gpu):
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer()
  yield t
  t.close()


@functools.lru_cache(maxsize=None)
def family(name):
  if name == 'wiki':
    return tuple(M.wiki(300_000))
  if name == 'sweep':
    return tuple(M.shift_sweep())
  if name == 'random':
    return tuple(M.random_code_points(11, 2000))
  if name == 'edge':
    return tuple(M.EDGE)
  return tuple(M.adversarial(int(name[3:]), 3000))


@functools.lru_cache(maxsize=None)
def expected(name, whole_line):
  return M.reference(list(family(name)), whole_line)


def gpu_split(tok, records, whole_line, **kw):
  from lddl_amd import splitgpu
  sh, ids = splitgpu.split_device(tok, [r.encode('utf-8') for r in records], whole_line, **kw)
  torch.cuda.synchronize()
  return sh, ids


def same(sh, ids, exp, n_rec):
  edata, eso, edso, eids = exp
  assert sh.n_doc == n_rec and sh.n_sent == len(eso) - 1 and sh.nbytes == len(edata)
  assert np.array_equal(sh.doc_sent_off.cpu().numpy(), edso)
  assert np.array_equal(sh.sent_off.cpu().numpy(), eso)
  data = sh.data.cpu().numpy()
  assert data.size == len(edata) + 16
  assert data[:len(edata)].tobytes() == edata
  assert not data[len(edata):].any()
  assert ids == eids


@pytest.mark.parametrize('whole_line', MODES)
@pytest.mark.parametrize('name', ['adv0', 'adv1', 'adv2', 'adv3', 'random', 'edge', 'wiki', 'sweep'])
def test_families(tok, name, whole_line):
  recs = family(name)
  same(*gpu_split(tok, recs, whole_line), expected(name, whole_line), len(recs))


@pytest.mark.parametrize('whole_line', MODES)
def test_degenerate(tok, whole_line):
  for recs in M.degenerate(300_000):
    same(*gpu_split(tok, recs, whole_line), M.reference(recs, whole_line), len(recs))


@pytest.mark.parametrize('whole_line', MODES)
def test_one_3mb_record_against_the_model(tok, whole_line):
  """a whole book as one record: 750 pieces of one record, its breaks counted by many waves"""
  rec = M.book(3_300_000)
  raws = [rec.encode('utf-8')]
  assert len(raws[0]) >= 3_000_000
  buf, rec_off = M.join(raws)
  data, so, dso, id_end = M.split_model(buf, rec_off, 1 if whole_line else 0)
  ids = [''] if whole_line else M.model_ids(raws, id_end, rec_off)
  assert len(so) > 10_000
  same(*gpu_split(tok, [rec], whole_line), (data, so, dso, ids), 1)


def test_two_ctxs_and_workspace_reuse(tok):
  """a second ctx (its own property table and workspace), and one ctx called back to back with a larger, a
  smaller and again the larger input"""
  from lddl_amd.tokenizer import Tokenizer
  big, small = family('adv0'), family('edge')
  t2 = Tokenizer()
  try:
    for t in (tok, t2, tok):
      for name, recs in (('adv0', big), ('edge', small), ('adv0', big)):
        same(*gpu_split(t, recs, False), expected(name, False), len(recs))
  finally:
    t2.close()


def test_non_default_stream(tok):
  recs = family('adv1')
  st = torch.cuda.Stream()
  sh, ids = gpu_split(tok, recs, False, stream=st)
  same(sh, ids, expected('adv1', False), len(recs))


def test_partitions_pass_through(tok):
  recs = family('edge')
  sh, _ = gpu_split(tok, recs, False, part_rec_off=[0, 3, 3, len(recs)])
  assert sh.part_doc_off.cpu().tolist() == [0, 3, 3, len(recs)]
  with pytest.raises(ValueError):
    gpu_split(tok, recs, False, part_rec_off=[0, 3])


def test_feeds_the_packer(gpu):
  """Packer.run over the GPU split's ShardSet packs what it packs from upload(split_records(...))"""
  from lddl_amd import pipeline, preprocess, splitgpu
  recs = M.wiki(50_000, seed=3)
  part = np.array([0, len(recs) // 2, len(recs)], dtype=np.int64)
  pk = pipeline.Packer()
  corpus, _ = preprocess.split_records(recs, False, preprocess._rule_split)
  kw = dict(target_seq_length=128, bin_size=32, seed=7)
  want = pk.run(pipeline.upload(corpus, part, gpu), into=pipeline.PackHandle(pk.tok), **kw)
  sh, _ = splitgpu.split_device(pk.tok, [r.encode('utf-8') for r in recs], part_rec_off=part)
  got = pk.run(sh, into=pipeline.PackHandle(pk.tok), **kw)
  torch.cuda.synchronize()
  assert got.n_pairs == want.n_pairs > 0 and got.n_tokens == want.n_tokens
  assert got.rows() == want.rows()
  assert torch.equal(got.bin_count, want.bin_count)
