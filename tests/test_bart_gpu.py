"""lddl_bart_count / _plan_len / _plan / _render (lddl_amd/csrc/bart.hip,
capi_bart.hip), lddl_amd/bart.py and the CLI's `bart` sub-command, exact
against tests/bart_model.py (which tests/test_bart_host.py pins to the
reference's own output).

  count   sentences of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 1025 bytes; a
          2-byte and a 3-byte whitespace character (and a 2- and 3-byte letter)
          across every 64-byte step of the wave loop; a sentence that begins
          with a letter right after one that ends with a letter; the last
          sentence ending with the last byte of a buffer of exactly nbytes;
          the golden articles; more sentences than one pass of the grid
  plan    documents of 0, 1, 2, 63, 64, 65 and 300 sentences; counts that
          reach T on the last sentence, stop one short, one sentence above T;
          T = 0 and -1; 0-word sentences leading, trailing and as a whole
          document; empty partitions at both ends and in the middle; more
          documents than one pass of the grid
  render  whole and as ranges that start inside the table; 64 guard bytes on
          each side at a 16-B aligned base and one byte off; the size query;
          LDDL_ECAPACITY one byte short; a chunk_nsent / chunk_off entry
          altered by one is LDDL_EINVAL with the chunks concerned unwritten
  e2e     two text files, --num-blocks 3, parquet and txt
"""
import ctypes
import functools
import os
import random

import numpy as np
import pytest
import torch

import bart_model as bm
from lddl_amd import _lib
from test_bart_host import golden_docs

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -6
GUARD = 64
WS2, WS3 = '\u00a0'.encode(), '\u3000'.encode()  # 2- and 3-byte whitespace
CH2, CH3 = '\u00e9'.encode(), '\u4e2d'.encode()  # 2- and 3-byte letters


@pytest.fixture(scope='module')
def tok(gpu):
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer()
  yield t
  t.close()


def dev(a, dtype):
  return torch.from_numpy(np.array(a, dtype=dtype)).cuda()


def ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def last_error():
  return _lib.lib().lddl_last_error().decode()


def shard_set(docs, part_doc_off=None):
  """(pipeline.ShardSet on the device with data of exactly nbytes, host table)"""
  from lddl_amd.pipeline import ShardSet
  data, so, dso = bm.table(docs)
  pdo = np.array([0, len(docs)] if part_doc_off is None else part_doc_off, dtype=np.int64)
  d = dev(data, np.uint8) if data.size else torch.empty(0, dtype=torch.uint8, device='cuda')
  return ShardSet(d, dev(so, np.int64), dev(dso, np.int64), dev(pdo, np.int64), None, int(data.size)), (data, so, dso)


def gpu_count(tok, data, so):
  n = len(so) - 1
  d = dev(data, np.uint8)  # exactly nbytes long: the last sentence ends with the buffer
  out = torch.full((max(n, 1),), -7, dtype=torch.int32, device='cuda')
  rc = _lib.lib().lddl_bart_count(tok.handle, ptr(d), int(data.size), ptr(dev(so, np.int64)), n, ptr(out), None)
  assert rc == 0, last_error()
  return out[:n].cpu().numpy()


def check_count(tok, sents):
  data, so, _ = bm.table([sents])
  got, want = gpu_count(tok, data, so), bm.count_words(data, so)
  bad = np.nonzero(got != want)[0]
  assert bad.size == 0, 'sentence %d (%r): %d words, expected %d' % (bad[0], sents[bad[0]][:80], got[bad[0]], want[bad[0]])


def text_of(nbytes, lead=b''):
  """nbytes bytes of short words, after `lead`"""
  s = lead + b'ab c def gh ' * (nbytes // 12 + 1)
  return s[:nbytes]


# ---- count ----------------------------------------------------------------------
def test_count_lengths_and_edges(tok):
  sents = []
  for n in (0, 1, 2, 63, 64, 65, 127, 128, 129, 1025):
    sents += [text_of(n), text_of(n, b' '), b'x' * n, b' ' * n]
  # multi-byte characters across every 64-byte step (steps are relative to the sentence's first byte)
  for ch in (WS2, WS3, CH2, CH3):
    for edge in (64, 128, 192):
      for before in range(1, len(ch)):  # `before` bytes of the character lie ahead of the edge
        head = edge - before
        sents.append(b'x' * head + ch + b'y' * 70)
        sents.append(b'x' * (head - 1) + b' ' + ch + ch + b' y' * 35)
  sents += [b'abc', b'def', b'g h', b'i', WS3 + b'k', b'l' + WS2]  # letter right after a letter; the last bytes of data
  check_count(tok, sents)


def test_count_golden_articles(tok):
  check_count(tok, [s.encode() for d in golden_docs() for s in d])


def test_count_more_sentences_than_one_grid_pass(tok):
  waves = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 4  # bart.hip wave_grid
  rng = random.Random(3)
  words = [b'a', b'bc', b' ', WS3, b'd e', b'']
  check_count(tok, [b''.join(rng.choice(words) for _ in range(rng.randint(0, 4))) for _ in range(waves + 4097)])


def test_count_refuses_offsets_outside_the_buffer(tok):
  data = np.frombuffer(b'one two three', dtype=np.uint8)
  L = _lib.lib()
  d, out = dev(data, np.uint8), torch.zeros(2, dtype=torch.int32, device='cuda')
  for so in ([0, 7, 14], [0, 8, 7], [-1, 3, 13]):
    assert L.lddl_bart_count(tok.handle, ptr(d), 13, ptr(dev(so, np.int64)), 2, ptr(out), None) == EINVAL
    assert 'sentence' in last_error()
  assert L.lddl_bart_count(tok.handle, ptr(d), 13, ptr(dev([0, 7, 13], np.int64)), 2, ptr(out), None) == 0
  assert out.cpu().tolist() == [2, 1]
  assert L.lddl_bart_count(tok.handle, ptr(d), 13, None, 2, ptr(out), None) == EINVAL
  assert L.lddl_bart_count(tok.handle, ptr(d), 13, ptr(dev([0, 7, 13], np.int64)), -1, ptr(out), None) == EINVAL


# ---- plan -----------------------------------------------------------------------
SEPS = [b' ', b' ', b'  ', b'\t', WS3]


def sent_of(rng, w):
  """a sentence of w words; 0 words: empty or whitespace only"""
  if w == 0:
    return rng.choice([b'', b' ', b'  ', WS3])
  out = b''
  for i in range(w):
    out += (rng.choice(SEPS) if i else b'') + rng.choice([b'w', b'xy', CH3, b'z.'])
  return out


@functools.lru_cache(maxsize=None)
def plan_docs():
  """hand-made documents for T = 5 (target_seq_length 8), with their partitions"""
  rng = random.Random(11)
  counts = [[rng.randint(1, 3) for _ in range(n)] for n in (0, 1, 2, 63, 64, 65, 300)]
  counts += [[2, 3], [2, 2], [9], [9, 1], [1, 9], [5], [4], [6],      # reaches T on the last, one short, above T
             [0, 0, 3, 2], [5, 0, 0], [3, 0], [0, 0, 0], [0], [], [0, 5, 0, 1, 0]]
  docs = [[sent_of(rng, w) for w in c] for c in counts]
  n = len(docs)
  return docs, [0, 0, 3, 3, 7, 7, n, n]  # empty partitions at both ends and in the middle


def run_aggregate(tok, docs, pdo, tsl):
  from lddl_amd import bart
  sh, host = shard_set(docs, pdo)
  return bart.aggregate(sh, None, tsl, tok), host


def check_plan(res, host, pdo, tsl):
  data, so, dso = host
  want = bm.plan(bm.count_words(data, so), so, dso, tsl - 3)
  assert res.n_chunks == len(want['chunk_sent0']) and res.nbytes == int(want['chunk_off'][-1])
  for name, got in (('doc_chunk_off', res.doc_chunk_off), ('chunk_sent0', res.chunk_sent0),
                    ('chunk_nsent', res.chunk_nsent), ('chunk_num_tokens', res.num_tokens),
                    ('chunk_off', res.chunk_off)):
    g = got.cpu().numpy()
    assert g.dtype == want[name].dtype and np.array_equal(g, want[name]), (name, tsl)
  assert np.array_equal(res.part_chunk_off, want['doc_chunk_off'][np.asarray(pdo)])
  return want


@pytest.mark.parametrize('tsl', [8, 3, 2, 128])  # T = 5, 0, -1, 125
def test_plan_and_render_hand_made(tok, tsl):
  docs, pdo = plan_docs()
  res, host = run_aggregate(tok, docs, pdo, tsl)
  want = check_plan(res, host, pdo, tsl)
  eoff, ebytes = bm.render(host[0], host[1], want)
  off, data = res.render()
  assert np.array_equal(off, eoff) and data.tobytes() == ebytes.tobytes()
  nc = res.n_chunks
  for c0, n in ((0, 0), (nc, 0), (3, 5), (nc - 1, 1), (1, nc - 1), (nc // 2, nc - nc // 2)):
    if c0 + n > nc or c0 < 0:
      continue
    off, data = res.render(c0, n)
    roff, rbytes = bm.render(host[0], host[1], want, c0, n)
    assert off[0] == 0 and np.array_equal(off, roff) and data.tobytes() == rbytes.tobytes(), (c0, n)


def test_plan_golden_articles(tok):
  docs = [[s.encode() for s in d] for d in golden_docs()]
  for tsl in (8, 128):
    res, host = run_aggregate(tok, docs, None, tsl)
    want = check_plan(res, host, [0, len(docs)], tsl)
    off, data = res.render()
    eoff, ebytes = bm.render(host[0], host[1], want)
    assert np.array_equal(off, eoff) and data.tobytes() == ebytes.tobytes()


def test_plan_more_documents_than_one_grid_pass(tok):
  lanes = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 256  # bart.hip lane_grid
  rng = random.Random(5)
  pool = [[sent_of(rng, w) for w in c] for c in ([], [0], [1], [2, 3], [5], [1, 0], [3, 3, 3], [0, 0])]
  docs = [pool[rng.randrange(len(pool))] for _ in range(lanes + 1000)]
  pdo = [0, 17, lanes, len(docs)]
  res, host = run_aggregate(tok, docs, pdo, 8)
  want = check_plan(res, host, pdo, 8)
  c0 = res.n_chunks - 5000
  off, data = res.render(c0, 5000)
  roff, rbytes = bm.render(host[0], host[1], want, c0, 5000)
  assert np.array_equal(off, roff) and data.tobytes() == rbytes.tobytes()


def test_plan_argument_errors(tok):
  docs, pdo = plan_docs()
  sh, host = shard_set(docs, pdo)
  L, h = _lib.lib(), tok.handle
  n_sent, n_doc = sh.n_sent, sh.n_doc
  nw = dev(bm.count_words(host[0], host[1]), np.int32)
  dco = torch.empty(n_doc + 1, dtype=torch.int64, device='cuda')
  tot = (ctypes.c_int64 * 2)()
  call = lambda **k: L.lddl_bart_plan_len(h, k.get('nw', ptr(nw)), ptr(sh.sent_off), k.get('dso', ptr(sh.doc_sent_off)),
                                          k.get('n_doc', n_doc), k.get('n_sent', n_sent), 8, ptr(dco), tot, None)
  assert call(nw=None) == EINVAL and 'null' in last_error()
  assert call(n_doc=-1) == EINVAL and 'negative' in last_error()
  assert call(n_sent=n_sent - 1) == EINVAL and 'n_sent' in last_error()  # doc_sent_off ends beyond n_sent
  assert call(n_doc=n_doc - 1) == EINVAL and 'n_sent' in last_error()   # doc_sent_off[n_doc - 1] != n_sent
  bad = host[2].copy()
  bad[4] = n_sent + 5
  assert call(dso=ptr(dev(bad, np.int64))) == EINVAL
  assert call() == 0, last_error()  # the next call on the ctx is right
  want = bm.plan(bm.count_words(host[0], host[1]), host[1], host[2], 5)
  assert (tot[0], tot[1]) == (len(want['chunk_sent0']), int(want['chunk_off'][-1]))
  assert np.array_equal(dco.cpu().numpy(), want['doc_chunk_off'])
  # the fill pass checks doc_chunk_off / n_chunks against its own walk
  nc = int(tot[0])
  outs = [torch.empty(nc + 1, dtype=t, device='cuda') for t in (torch.int64, torch.int32, torch.int32, torch.int64)]
  fill = lambda d, n: L.lddl_bart_plan(h, ptr(nw), ptr(sh.sent_off), ptr(sh.doc_sent_off), ptr(d), n_doc, n_sent, 8, n,
                                       *[ptr(o) for o in outs], None)
  wrong = want['doc_chunk_off'].copy()
  wrong[5] += 1
  assert fill(dev(wrong, np.int64), nc) == EINVAL and 'lddl_bart_plan_len' in last_error()
  assert fill(dco, nc - 1) == EINVAL
  assert fill(dco, nc) == 0, last_error()
  assert np.array_equal(outs[3].cpu().numpy(), want['chunk_off'])


# ---- render ---------------------------------------------------------------------
def raw_render(tok, res, c0, n, buf=None, at=0, cap=0, sent0=None, nsent=None, coff=None):
  """lddl_bart_render into buf[at:] -> (rc, nbytes, offsets)"""
  sh = res.shards
  off = torch.full((n + 1,), -1, dtype=torch.int64, device='cuda')
  nb = ctypes.c_int64(-1)
  out = ctypes.c_void_p(buf.data_ptr() + at) if buf is not None else ctypes.c_void_p(0)
  rc = _lib.lib().lddl_bart_render(tok.handle, ptr(sh.data), sh.nbytes, ptr(sh.sent_off), sh.n_sent,
                                   ptr(res.chunk_sent0 if sent0 is None else sent0),
                                   ptr(res.chunk_nsent if nsent is None else nsent),
                                   ptr(res.chunk_off if coff is None else coff), res.n_chunks, c0, n, ptr(off), out, cap,
                                   ctypes.byref(nb), None)
  return rc, nb.value, off.cpu().numpy()


@pytest.mark.parametrize('shift', [0, 1])  # the output 16-B aligned, and one byte off
def test_render_guards_capacity_and_refusals(tok, shift):
  docs, pdo = plan_docs()
  res, host = run_aggregate(tok, docs, pdo, 8)
  want = check_plan(res, host, pdo, 8)
  nc = res.n_chunks
  for c0, n in ((0, nc), (4, nc - 9)):
    eoff, ebytes = bm.render(host[0], host[1], want, c0, n)
    total = int(eoff[-1])
    rc, nb, off = raw_render(tok, res, c0, n)  # the size query
    assert (rc, nb) == (0, total) and np.array_equal(off, eoff)
    buf = torch.full((GUARD + shift + total + GUARD,), 0xAA, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    at = GUARD + shift
    rc, nb, _ = raw_render(tok, res, c0, n, buf, at, total - 1)
    assert (rc, nb) == (ECAPACITY, total) and 'out_cap %d' % (total - 1) in last_error()
    assert bool((buf == 0xAA).all())  # nothing written
    rc, nb, off = raw_render(tok, res, c0, n, buf, at, total)  # the next call on the ctx, at the exact capacity
    assert (rc, nb) == (0, total) and np.array_equal(off, eoff)
    got = buf.cpu().numpy()
    assert got[at:at + total].tobytes() == ebytes.tobytes()
    assert (got[:at] == 0xAA).all() and (got[at + total:] == 0xAA).all()

    def refused(bad_chunks, **tables):
      """the call is LDDL_EINVAL naming the lowest refused chunk; those chunks are unwritten, every other
      chunk of the range is right, the guards are intact"""
      buf.fill_(0xAA)
      rc, _, _ = raw_render(tok, res, c0, n, buf, at, total, **tables)
      assert rc == EINVAL and 'chunk %d ' % min(bad_chunks) in last_error(), (rc, last_error())
      got = buf.cpu().numpy()
      exp = np.frombuffer(ebytes.tobytes(), dtype=np.uint8).copy()
      for c in bad_chunks:
        exp[eoff[c - c0]:eoff[c - c0 + 1]] = 0xAA
      assert np.array_equal(got[at:at + total], exp)
      assert (got[:at] == 0xAA).all() and (got[at + total:] == 0xAA).all()

    mid = c0 + n // 2
    for c, d in ((mid, 1), (mid, -1), (c0 + n - 1, 1), (c0, -1)):
      ns = want['chunk_nsent'].copy()
      ns[c] += d
      refused([c], nsent=dev(ns, np.int32))
    for c, d in ((mid, 1), (mid, -1)):  # entry c bounds chunks c - 1 and c
      co = want['chunk_off'].copy()
      co[c] += d
      refused([c - 1, c], coff=dev(co, np.int64))
    s0 = want['chunk_sent0'].copy()
    s0[mid] = -1
    refused([mid], sent0=dev(s0, np.int64))
    s0[mid] = res.shards.n_sent + 1
    refused([mid], sent0=dev(s0, np.int64))
    buf.fill_(0xAA)
    rc, nb, off = raw_render(tok, res, c0, n, buf, at, total)  # and the next call is right
    assert (rc, nb) == (0, total) and buf.cpu().numpy()[at:at + total].tobytes() == ebytes.tobytes()


def test_render_argument_errors(tok):
  docs, pdo = plan_docs()
  res, _ = run_aggregate(tok, docs, pdo, 8)
  nc = res.n_chunks
  for c0, n in ((-1, 1), (0, -1), (nc, 1), (1, nc)):
    off = torch.empty(nc + 2, dtype=torch.int64, device='cuda')
    nb = ctypes.c_int64(0)
    sh = res.shards
    rc = _lib.lib().lddl_bart_render(tok.handle, ptr(sh.data), sh.nbytes, ptr(sh.sent_off), sh.n_sent,
                                     ptr(res.chunk_sent0), ptr(res.chunk_nsent), ptr(res.chunk_off), nc, c0, n,
                                     ptr(off), None, 0, ctypes.byref(nb), None)
    assert rc == EINVAL, (c0, n)
  rc, nb, _ = raw_render(tok, res, 0, nc)
  assert rc == 0 and nb == res.nbytes


# ---- writers and the CLI -----------------------------------------------------------
def test_cli_end_to_end(tok, tmp_path):
  import pyarrow.parquet as pq
  from lddl_amd import preprocess
  src = tmp_path / 'books'
  src.mkdir()
  rng = random.Random(9)
  words = 'the quick brown fox jumps over a lazy dog and runs far away from here today'.split()

  def line(k):
    sents = [' '.join(rng.choice(words) for _ in range(rng.randint(3, 12))).capitalize() + '.'
             for _ in range(rng.randint(1, 9))]
    return 'doc%d ' % k + ' '.join(sents)
  (src / 'a.txt').write_text('\n'.join(line(k) for k in range(40)) + '\n')
  (src / 'b.txt').write_text('\n\n'.join(line(k) for k in range(40, 55)) + '\n')
  common = ['--books', str(src), '--num-blocks', '3', '--sentence-splitter', 'rules', '--target-seq-length', '32']
  args = preprocess.attach_bart_args().parse_args(common + ['--sink', 'x'])
  index, order, pro = preprocess.plan_bart_input(args)
  n_part = len(pro) - 1
  assert n_part >= 3
  want = []
  for p in range(n_part):
    corpus, _ = preprocess.split_chunk(index, order[int(pro[p]):int(pro[p + 1])], False, preprocess._rule_split, True)
    nb = corpus.nbytes
    _, chunks = bm.aggregate(corpus.data[:nb], corpus.sent_off, corpus.doc_sent_off, 32 - 3)
    want.append([c.decode() for c in chunks])
  index.close()
  assert sum(map(len, want)) > 20 and want[0][0].startswith(' doc0 ')  # the id stays in the first sentence
  preprocess.bart_console_script(common + ['--sink', str(tmp_path / 'pq')])
  assert sorted(os.listdir(tmp_path / 'pq')) == sorted('part.%d.parquet' % p for p in range(n_part))
  for p in range(n_part):
    t = pq.read_table(str(tmp_path / 'pq' / ('part.%d.parquet' % p)))
    assert t.schema.names == ['sentences'] and str(t.schema.field('sentences').type) == 'string'
    assert t.column('sentences').to_pylist() == want[p], p
  preprocess.bart_console_script(common + ['--sink', str(tmp_path / 'txt'), '--output-format', 'txt'])
  assert sorted(os.listdir(tmp_path / 'txt')) == sorted('%d.txt' % p for p in range(n_part))
  for p in range(n_part):
    assert (tmp_path / 'txt' / ('%d.txt' % p)).read_bytes() == '\n'.join(want[p]).encode(), p


def test_writers_create_every_partitions_file(tok, tmp_path):
  import pyarrow.parquet as pq
  from lddl_amd import bart
  docs, pdo = plan_docs()
  res, host = run_aggregate(tok, docs, pdo, 8)
  _, chunks = bm.aggregate(host[0], host[1], host[2], 5)
  pco = res.part_chunk_off
  files = bart.write_bart_shards(res, str(tmp_path / 'pq'), part_base=10, batch_rows=40)
  assert [os.path.basename(f) for f in files] == ['part.%d.parquet' % (10 + p) for p in range(len(pdo) - 1)]
  txt = bart.write_bart_txt(res, str(tmp_path / 'txt'), part_base=10, batch_rows=40)
  for p, (f, g) in enumerate(zip(files, txt)):
    rows = [c.decode() for c in chunks[pco[p]:pco[p + 1]]]
    assert pq.read_table(f).column('sentences').to_pylist() == rows
    assert open(g, 'rb').read() == '\n'.join(rows).encode()
  assert pq.read_table(files[0]).num_rows == 0 and os.path.getsize(txt[0]) == 0
