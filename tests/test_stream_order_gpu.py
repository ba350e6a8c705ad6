"""Every GPU entry point on a side stream behind a delayed producer
(tests/stream_cases.py holds the harness, the cases and what they prove).

Checklist: every entry point of include/lddl_amd.h that takes a `stream`, and
the cases (ids of test_side_stream, or a test of this module) that reach it;
test_every_stream_entry_point_has_a_case holds this list to the header.

  lddl_tokenize                       tokenize[ test_two_streams_one_ctx
  lddl_pack_bert                      pack[bert- pack[masked-
  lddl_pack_codebert                  pack[codebert-
  lddl_pack_mlm                       pack[mlm-
  lddl_pack_sop                       pack[sop-
  lddl_materialize                    pack[bert-rows post_pack[rows]
  lddl_row_spans                      pack[bert-spans test_two_streams_one_ctx
  lddl_masked_lm                      pack[masked-rows]
  lddl_masked_lm_spans                pack[masked-spans] post_pack[spans]
  lddl_render_strings                 render[span- render[labels- write_shards[codebert]
  lddl_render_masked                  render_masked[ write_shards[bert] write_txt[bert]
  lddl_render_npy                     render_npy[ write_shards[bert]
  lddl_row_docs                       row_docs write_shards[codebert]
  lddl_bin                            bin_rows
  lddl_collate_seq_len                collate_call[ collate_arrow
  lddl_collate_bert                   collate_call[ collate_arrow
  lddl_mask_tokens                    mask_tokens
  lddl_collate_rows_seq_len           collate_rows[bert-padded-
  lddl_collate_rows                   collate_rows[bert-padded-
  lddl_collate_rows_cu_seqlens        collate_rows[bert-unpadded-
  lddl_collate_rows_unpadded          collate_rows[bert-unpadded-
  lddl_collate_rows_fixed             collate_rows[bert-fixed-
  lddl_collate_code_rows_seq_len      collate_rows[code-padded- collate_rows[mlm-padded-
  lddl_collate_code_rows              collate_rows[code-padded- collate_rows[mlm-padded-
  lddl_collate_code_rows_cu_seqlens   collate_rows[code-unpadded- collate_rows[mlm-unpadded-
  lddl_collate_code_rows_unpadded     collate_rows[code-unpadded- collate_rows[mlm-unpadded-
  lddl_collate_code_rows_fixed        collate_rows[code-fixed- collate_rows[mlm-fixed-
  lddl_mlm_targets                    mlm_targets[
  lddl_rows_from_strings_len          load_rows[bert
  lddl_rows_from_strings              load_rows[bert
  lddl_code_rows_from_strings_len     load_rows[code]
  lddl_code_rows_from_strings         load_rows[code]
  lddl_bart_count                     bart_aggregate
  lddl_bart_plan_len                  bart_aggregate
  lddl_bart_plan                      bart_aggregate
  lddl_bart_render                    bart_render[
  lddl_split_len                      split_device
  lddl_split                          split_device
"""
import contextlib
import os
import re
import types

import numpy as np
import pytest
import torch

import stream_cases as SC

pytestmark = pytest.mark.gpu

SEED = 9091
PACK_KW = dict(target_seq_length=128, bin_size=32, duplicate_factor=2, seed=SEED)
N_BATCH = 24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u16(t, n=None):
  a = t.cpu().numpy()
  return (a if n is None else a[:n]).view(np.uint16)


def _on(s):
  """the current stream for wrappers that take none: s, or the default one"""
  return torch.cuda.stream(s) if s is not None else contextlib.nullcontext()


def _tokenized(pk, sh):
  """the dense ids of sh in buffers that hold every possible total (the rest zeroed), and host copies"""
  ids = torch.zeros(sh.nbytes + 32, dtype=torch.int16, device=sh.data.device)
  ntok = torch.empty(sh.n_sent, dtype=torch.int32, device=sh.data.device)
  toff = torch.empty(sh.n_sent + 1, dtype=torch.int64, device=sh.data.device)
  pk.tok.tokenize_device(sh.data, sh.sent_off, 512, ids, ntok, toff, nbytes=sh.nbytes)
  torch.cuda.synchronize()
  return types.SimpleNamespace(ids=ids, ntok=ntok, toff=toff, ids_a=_u16(ids).copy(), ntok_a=ntok.cpu().numpy().copy())


@pytest.fixture(scope='module')
def env(gpu):
  from lddl_amd import pipeline, synth
  e = types.SimpleNamespace(dev=gpu)
  e.delay, e.delay_ms = SC.calibrate()
  print('stream-order delay: %.1f ms' % e.delay_ms)
  c = synth.make_wiki(250_000, seed=SEED)
  half = c.n_doc // 2
  e.corpus = c
  e.pk = pipeline.Packer(pipeline.VOCAB_BERT, 0, masking=True)  # the module's ctx (and one for the CodeBERT vocabulary)
  e.sh = pipeline.upload(c, [0, half, half, c.n_doc], gpu)
  e.text_a = np.ascontiguousarray(c.data[:c.nbytes]).copy()
  e.t = _tokenized(e.pk, e.sh)
  cc = synth.make_code(300, seed=SEED)
  e.cpk = pipeline.Packer(pipeline.VOCAB_CODEBERT, 0)
  e.csh = pipeline.upload(cc, [0, 150, 150, cc.n_doc], gpu)
  e.ct = _tokenized(e.cpk, e.csh)
  e.meta = {}
  for name, pk in (('bert', e.pk), ('codebert', e.cpk)):
    t = pk.tok
    e.meta[name] = {'vocab': t.vocab_size, 'special': (t.pad_id, t.unk_id, t.cls_id, t.sep_id, t.mask_id), 'range': (1, 129)}
  e.handles = {}
  e.res = {}
  return e


def _meta(e, case):
  return e.meta['codebert' if SC.meta_for(case)['vocab'] == SC.VOCAB_SIZES['codebert'] else 'bert']


def _res(e, key):
  """a pack result with spans in a handle of its own, packed once on the default stream"""
  from lddl_amd import pipeline
  if key not in e.res:
    code = key.startswith('code')
    pk, sh, t = (e.cpk, e.csh, e.ct) if code else (e.pk, e.sh, e.t)
    kw = dict(PACK_KW, spans=key != 'rows', into=pipeline.PackHandle(pk.tok))
    if code:
      kw.update(codebert=True, seed=SEED + (1 if key == 'code2' else 0))
    elif key == 'mlm':
      kw.update(nsp=False)
    else:
      kw.update(masking=True)
    r = pk.pack(sh, t.ids, t.ntok, t.toff, **kw)
    torch.cuda.synchronize()
    assert r.n_pairs > 4 * N_BATCH
    e.res[key] = r
  return e.res[key]


def _live(e, case, names):
  """[(name, role, live tensor, A)] of a case's staged arrays, from the tensors in `names`"""
  return [(n, role, names[n][0], names[n][1]) for n, role in case.staged]


# ---- the kinds -------------------------------------------------------------------
def k_tokenize(e, case):
  from lddl_amd import pipeline, synth
  p = case.p
  if p.get('dense'):  # 60-letter words among empty sentences: every window goes to the serial path (tokenize_fallback.hip)
    c = synth.corpus_from_sentences((['q' * 60] + [''] * 30) * 300, [0, 31 * 300])
    sh, text = pipeline.upload(c, [0, 1], e.dev), c.data[:c.nbytes].copy()
  else:
    sh, text = e.sh, e.text_a
  n = sh.nbytes
  ids = torch.zeros(n + 32, dtype=torch.int16, device=e.dev)  # capacity nbytes + 16: no total can pass it
  ntok = torch.empty(sh.n_sent, dtype=torch.int32, device=e.dev)
  toff = torch.empty(sh.n_sent + 1, dtype=torch.int64, device=e.dev)
  bufs = pipeline.TokBuffers()

  def call(s, which):
    if p.get('packer'):
      i, nt, to = e.pk.tokenize(sh, stream=s, bufs=bufs)
    else:
      e.pk.tok.set_algo(p['algo'])
      try:
        i, nt, to = e.pk.tok.tokenize_device(sh.data, sh.sent_off, 512, ids, ntok, toff, s, nbytes=n)
      finally:
        e.pk.tok.set_algo(5)
    # (ids past the total are not part of the result)
    return {'ntok': nt[:sh.n_sent], 'tok_off': to[:sh.n_sent + 1], 'ids': lambda: i[:int(to[sh.n_sent].item())]}
  return _live(e, case, {'text': (sh.data[:n], text)}), call


def _pack_out(res):
  n = res.n_pairs
  out = {'n_pairs': n, 'n_tokens': res.n_tokens, 'nbins': res.nbins, 'n_masked': res.n_masked,
         'tok_off': res.tok_off[:n + 1], 'len0': res.len0[:n], 'len1': res.len1[:n], 'flags': res.flags[:n],
         'bins': res.bins[:n], 'part': res.part[:n], 'bin_count': res.bin_count}
  if res.spans:
    out.update(src0=res.src0[:n], src1=res.src1[:n])
  else:
    out['tokens'] = res.tokens[:res.n_tokens]
  if res.mlm_off is not None:
    out.update(mlm_off=res.mlm_off[:n + 1], mlm_pos=res.mlm_pos[:res.n_masked], mlm_label=res.mlm_label[:res.n_masked])
  if res.mlm_token is not None:
    out['mlm_token'] = res.mlm_token[:res.n_masked]
  return out


def k_pack(e, case):
  from lddl_amd import pipeline
  p = case.p
  code = p['kind'] == 'codebert'
  pk, sh, t = (e.cpk, e.csh, e.ct) if code else (e.pk, e.sh, e.t)
  kw = dict(PACK_KW, spans=p['spans'], codebert=code, masking=p['kind'] == 'masked', nsp=p['kind'] != 'mlm',
            sop=p['kind'] == 'sop')
  if p.get('into'):
    kw['into'] = e.handles.setdefault('into', pipeline.PackHandle(pk.tok))

  def call(s, which):
    return _pack_out(pk.pack(sh, t.ids, t.ntok, None if p.get('scan') else t.toff, stream=s, **kw))
  return _live(e, case, {'ntok': (t.ntok, t.ntok_a), 'ids': (t.ids, t.ids_a)}), call


def k_post_pack(e, case):
  """lddl_materialize, or lddl_masked_lm_spans, alone behind the producer (neither synchronises; lddl_masked_lm
  masks the rows of a pack in place exactly once, so it runs only inside pack[masked-rows])"""
  from lddl_amd import _lib
  from lddl_amd.tokenizer import _ptr, _stream
  r = _res(e, 'masked' if case.p['spans'] else 'rows')
  L, h, k = _lib.lib(), e.pk.tok.handle, r.pack.handle

  def call(s, which):
    st = _stream(s)
    if r.spans:
      _lib.check(L.lddl_masked_lm_spans(h, k, _ptr(r.ids), _ptr(r.src0), _ptr(r.src1), _ptr(r.len0), _ptr(r.part),
                                        _ptr(r.mlm_off), _ptr(r.mlm_pos), _ptr(r.mlm_label), _ptr(r.mlm_token), st))
    else:
      bc = torch.empty_like(r.bin_count)
      _lib.check(L.lddl_materialize(h, k, _ptr(r.ids), _ptr(r.tokens), _ptr(r.tok_off), _ptr(r.len0), _ptr(r.len1),
                                    _ptr(r.flags), _ptr(r.bins), _ptr(r.part), _ptr(bc), st))
      return {'tokens': r.tokens[:r.n_tokens], 'tok_off': r.tok_off[:r.n_pairs + 1], 'bin_count': bc}
    return _pack_out(r)
  return _live(e, case, {'ids': (e.t.ids, e.t.ids_a)}), call


def k_bin(e, case):
  from lddl_amd import pipeline
  a = np.random.default_rng(SEED).integers(1, 129, 20_000).astype(np.int64)
  t = torch.from_numpy(a).to(e.dev)

  def call(s, which):
    perm, counts = pipeline.bin_rows(e.pk.tok, t, 32, 4, stream=s)
    return {'perm': perm, 'counts': counts}
  return _live(e, case, {'num_tokens': (t, a)}), call


def k_row_docs(e, case):
  from lddl_amd import writer
  rs = {'A': _res(e, 'code'), 'B': _res(e, 'code2')}
  n = min(r.n_pairs for r in rs.values())

  def call(s, which):
    return {'docs': writer.row_docs(e.cpk, rs[which], n, stream=s)}
  return [], call


def _masked_names(e, r):
  return {'ids': (e.t.ids, e.t.ids_a), 'flags': (r.flags[:r.n_pairs], r.flags[:r.n_pairs].cpu().numpy()),
          'mlm_label': (r.mlm_label[:r.n_masked], _u16(r.mlm_label, r.n_masked)),
          'mlm_token': (r.mlm_token[:r.n_masked], _u16(r.mlm_token, r.n_masked)),
          'mlm_pos_values': (r.mlm_pos[:r.n_masked], _u16(r.mlm_pos, r.n_masked))}


def k_render(e, case):
  from lddl_amd import writer
  r = _res(e, 'masked')
  p = case.p
  r0, n = 7, min(r.n_pairs - 7, 2000)

  def call(s, which):
    kw = dict(stream=s, host=p['host'])
    if p['what'] == 'span':
      off, data = writer.render(e.pk, r.ids, r.src1, r0, n, writer.SPAN, len0=r.len1, **kw)
    elif p['what'] == 'labels':
      off, data = writer.render(e.pk, r.mlm_label, r.mlm_off, r0, n, writer.ROW, **kw)
    elif p['what'] == 'masked':
      off, data = writer.render_masked(e.pk, r, r0, n, 0, **kw)
    else:
      off, data = writer.render_npy(e.pk, r, r0, n, **kw)
    return {'off': off, 'data': data}
  return _live(e, case, _masked_names(e, r)), call


def k_write(e, case, tmp_path):
  from lddl_amd import writer
  p = case.p
  if p.get('code'):
    pk, r = e.cpk, _res(e, 'code')
    names = {'ids': (e.ct.ids, e.ct.ids_a)}
    kw = dict(codebert=True, doc_ids=['doc-%d' % i for i in range(e.csh.n_doc)])
  else:
    pk, r = e.pk, _res(e, 'masked')
    names, kw = _masked_names(e, r), dict(masking=True)
  run = [0]

  def call(s, which):
    run[0] += 1
    d = str(tmp_path / ('run%d' % run[0]))
    if p['sink'] == 'txt':
      files = writer.write_txt(pk, r, d, bin_size=32, stream=s, **kw)
      return {os.path.basename(f): open(f, 'rb').read() for f in files}
    files = writer.write_shards(pk, r, d, bin_size=32, batch_rows=1024, stream=s, **kw)
    return {os.path.basename(f): SC.parquet_bytes(f) for f in files}
  return _live(e, case, names), call


def k_bart(e, case):
  from lddl_amd import bart
  p = case.p
  if p['what'] == 'render' and 'bart' not in e.res:
    e.res['bart'] = bart.aggregate(e.sh, target_seq_length=128, tokenizer_or_ctx=e.pk)
    torch.cuda.synchronize()

  def call(s, which):
    if p['what'] == 'render':
      off, data = e.res['bart'].render(3, None, stream=s, host=p['host'])
      return {'off': off, 'data': data}
    b = bart.aggregate(e.sh, target_seq_length=128, tokenizer_or_ctx=e.pk, stream=s)
    return {'n_chunks': b.n_chunks, 'nbytes': b.nbytes, 'nwords': b.nwords, 'doc_chunk_off': b.doc_chunk_off,
            'chunk_sent0': b.chunk_sent0, 'chunk_nsent': b.chunk_nsent, 'num_tokens': b.num_tokens,
            'chunk_off': b.chunk_off, 'part_chunk_off': b.part_chunk_off}
  return _live(e, case, {'text': (e.sh.data[:e.sh.nbytes], e.text_a)}), call


def _records(e):
  """raw records `id text` of the corpus' documents, as one byte string and its offsets"""
  c = e.corpus
  n_doc = c.n_doc
  recs = [('wiki-%d ' % d + ' '.join(c.sentence(i) for i in range(c.doc_sent_off[d], c.doc_sent_off[d + 1]))).encode()
          for d in range(n_doc)]
  from lddl_amd.splitgpu import join_records
  return join_records(recs)


def k_split(e, case):
  from lddl_amd import splitgpu
  buf, rec_off = _records(e)
  bufs = {'A': buf, 'B': SC.rot_text(buf)}
  SC.check_pair('records', 'text', bufs['A'], bufs['B'], e.meta['bert'])
  n_rec = len(rec_off) - 1
  part = [0, n_rec // 3, n_rec // 3, n_rec]

  def call(s, which):
    sh, ids = splitgpu.split_device(e.pk.tok, (bufs[which], rec_off), part_rec_off=part, stream=s)
    return {'data': sh.data, 'sent_off': sh.sent_off, 'doc_sent_off': sh.doc_sent_off, 'part_doc_off': sh.part_doc_off,
            'nbytes': sh.nbytes, 'ids': ids}
  return [], call


def _collate(e, p, **kw):
  from lddl_amd import loader
  cls = {'bert': loader.BertCollate, 'code': loader.CodeCollate, 'mlm': loader.MlmCollate}[p.get('cls', 'bert')]
  pk = e.cpk if p.get('cls') == 'code' else e.pk
  return cls(tokenizer=pk.tok, base_seed=SEED, whole_word_mask=bool(p.get('wwm')),
             span_mask=(3, 0.3) if p.get('span') else None, **kw)


def k_collate(e, case):
  p = case.p
  code = p['cls'] == 'code'
  r = _res(e, {'bert': 'masked', 'code': 'code', 'mlm': 'mlm'}[p['cls']])
  t = e.ct if code else e.t
  rows = torch.arange(5, 5 + 3 * N_BATCH, 3, device=e.dev)  # fixed: in [0, n_total), never staged
  names = {'ids': (t.ids, t.ids_a)}
  if p['mode'] == 1:
    names.update(_masked_names(e, r))

  def call(s, which):
    col = _collate(e, p)  # (sets the ctx's masking switches; seed and counter fixed: the draws repeat)
    try:
      with _on(s):
        if p['route'] == 'padded':
          return col.collate_rows(r, rows, mode=p['mode'])
        if p['route'] == 'unpadded':
          return col.collate_rows_unpadded(r, rows, mode=p['mode'])
        return col.collate_rows_fixed(r, rows, mode=p['mode'], max_tokens=N_BATCH * 128, max_seqs=2 * N_BATCH + 2,
                                      max_seqlen=128)
    finally:
      _collate(e, {'cls': p['cls']})  # (switches off again)
  return _live(e, case, names), call


def _samples(e, static, n=N_BATCH):
  """the reference's samples of the first rows of the masked pack result, A (as packed) and B (letters rotated)"""
  from lddl_amd import writer
  r = _res(e, 'masked')
  cols = [writer.render_masked(e.pk, r, 0, n, seg) for seg in (0, 1)]
  cols.append(writer.render(e.pk, r.mlm_label, r.mlm_off, 0, n, writer.ROW))
  pos_off, pos = writer.render_npy(e.pk, r, 0, n)
  rn = (r.flags[:n].cpu().numpy() & 1).astype(bool)
  out = {}
  for which in 'AB':
    strs = []
    for off, data in cols:
      SC.check_pair('samples', 'text', data, SC.rot_text(data), e.meta['bert'])
      d = (data if which == 'A' else SC.rot_text(data)).tobytes()
      strs.append([d[off[i]:off[i + 1]].decode() for i in range(n)])
    posb = [pos[pos_off[i]:pos_off[i + 1]].tobytes() for i in range(n)]
    out[which] = [(strs[0][i], strs[1][i], bool(rn[i])) + ((posb[i], strs[2][i]) if static else ()) for i in range(n)]
  return out


def k_strings(e, case):
  import pyarrow as pa
  p = case.p
  what = p['what']
  if what == 'load_code':
    from lddl_amd import writer
    r = _res(e, 'code')
    n = 4 * N_BATCH
    cols = [writer.render(e.cpk, r.ids, src, 0, n, writer.SPAN, len0=ln) for src, ln in ((r.src0, r.len0), (r.src1, r.len1))]
    nt = np.diff(r.tok_off[:n + 1].cpu().numpy()).astype(np.uint16)
    tabs = {}
    for which in 'AB':
      strs = []
      for off, data in cols:
        SC.check_pair('samples', 'text', data, SC.rot_text(data), e.meta['codebert'])
        d = (data if which == 'A' else SC.rot_text(data)).tobytes()
        strs.append([d[off[i]:off[i + 1]].decode() for i in range(n)])
      tabs[which] = pa.table({'doc': strs[0], 'code': strs[1], 'num_tokens': pa.array(nt, pa.uint16())})
    col = _collate(e, {'cls': 'code'})

    def call(s, which):
      with _on(s):
        r = col.load_rows(tabs[which])
        return dict(_pack_out(r), ids=r.ids)
    return [], call
  sam = _samples(e, bool(p.get('static')), 4 * N_BATCH if what == 'load' else N_BATCH)
  col = _collate(e, {})

  def call(s, which):
    col.counter = 0
    b = sam[which]
    with _on(s):
      if what == 'load':
        r = col.load_rows(b)
        return dict(_pack_out(r), ids=r.ids)
      if what == 'call':
        return col(b)
      if what == 'encoded':
        return col.to_encoded_inputs(b)
      return col.collate_arrow(pa.table({'A': [x[0] for x in b], 'B': [x[1] for x in b],
                                         'is_random_next': [x[2] for x in b]}))
  return [], call


def k_mask_tokens(e, case):
  col = _collate(e, {})
  b = col.collate_rows(_res(e, 'masked'), row0=11, n_rows=N_BATCH, mode=0)
  torch.cuda.synchronize()
  inputs, sp = b['input_ids'].clone(), b['special_tokens_mask'].clone()
  a = inputs.cpu().numpy().copy()

  def call(s, which):
    with _on(s):
      ids, labels = col.mask_tokens(inputs, sp, counter=5)  # (in place: the harness refills `inputs` before every call)
    return {'input_ids': ids.clone() if s is None else ids, 'labels': labels}
  return _live(e, case, {'inputs': (inputs, a)}), call


def k_mlm_targets(e, case):
  col = _collate(e, {})
  r = _res(e, 'masked')
  if case.p['cu']:
    b = col.collate_rows_unpadded(r, row0=11, n_rows=N_BATCH, mode=2)
  else:
    b = col.collate_rows(r, row0=11, n_rows=N_BATCH, mode=2)
  torch.cuda.synchronize()
  labels, cu = b['labels'].clone(), b.get('cu_seqlens')
  a = labels.cpu().numpy().copy()

  def call(s, which):
    with _on(s):
      pos, lab, off = col.mlm_targets(labels, cu)
    return {'positions': pos, 'labels': lab, 'offsets': off}
  return _live(e, case, {'labels': (labels, a)}), call


KINDS = {'tokenize': k_tokenize, 'pack': k_pack, 'post_pack': k_post_pack, 'bin': k_bin, 'row_docs': k_row_docs,
         'render': k_render, 'write': k_write, 'bart': k_bart, 'split': k_split, 'collate': k_collate,
         'strings': k_strings, 'mask_tokens': k_mask_tokens, 'mlm_targets': k_mlm_targets}


@pytest.mark.parametrize('case', SC.CASES, ids=[c.id for c in SC.CASES])
def test_side_stream(env, case, tmp_path):
  staged, call = KINDS[case.kind](env, case, tmp_path) if case.kind == 'write' else KINDS[case.kind](env, case)
  assert case.host == (not staged)
  base_a, base_b, got = SC.run_delayed(case, staged, call, env.delay, _meta(env, case))
  SC.assert_same(case, base_a, base_b, got)


def test_two_streams_one_ctx(env):
  """the overlapped recipe at toy size: step k tokenizes on one stream into
  alternating buffer sets and packs on another, joined by events, the pack
  stream behind a delay; every step's rows are those of the same step run
  serially on the default stream"""
  from lddl_amd import pipeline, synth
  e = env
  c2 = synth.make_wiki(200_000, seed=SEED + 1)
  shs = [e.sh, pipeline.upload(c2, [0, c2.n_doc // 3, c2.n_doc // 3, c2.n_doc], e.dev)]
  kw = dict(PACK_KW, spans=True)
  serial = []
  for k in range(3):
    sh = shs[k % 2]
    serial.append(SC.snapshot(_pack_out(e.pk.pack(sh, *e.pk.tokenize(sh), **kw))))
    torch.cuda.synchronize()
  assert serial[0] != serial[1]
  st_tok, st_pack = torch.cuda.Stream(), torch.cuda.Stream()
  tbufs = [pipeline.TokBuffers(), pipeline.TokBuffers()]
  handles = [pipeline.PackHandle(e.pk.tok) for _ in range(3)]
  packed, results = [None, None], []
  for k in range(2):  # (grow every buffer and workspace first: an allocation would drain the delay)
    e.pk.pack(shs[k], *e.pk.tokenize(shs[k], bufs=tbufs[k]), into=handles[k], **kw)
  e.pk.pack(shs[0], *e.pk.tokenize(shs[0], bufs=tbufs[0]), into=handles[2], **kw)
  for t in tbufs:
    for b in t._out.values():
      b.zero_()
  torch.cuda.synchronize()
  with torch.cuda.stream(st_pack):
    e.delay()
  assert not st_pack.query()
  for k in range(3):
    i, sh = k % 2, shs[k % 2]
    with torch.cuda.stream(st_tok):
      if packed[i] is not None:
        st_tok.wait_event(packed[i])  # (the pack that last read set i)
      ids, ntok, toff = e.pk.tokenize(sh, stream=st_tok, bufs=tbufs[i])
      done_tok = torch.cuda.Event()
      done_tok.record(st_tok)
    with torch.cuda.stream(st_pack):
      st_pack.wait_event(done_tok)
      results.append(e.pk.pack(sh, ids, ntok, toff, stream=st_pack, into=handles[k], **kw))
      packed[i] = torch.cuda.Event()
      packed[i].record(st_pack)
  st_tok.synchronize()
  st_pack.synchronize()
  for k in range(3):
    got = SC.snapshot(_pack_out(results[k]))
    bad = [n for n in serial[k] if got[n] != serial[k][n]]
    assert not bad, (k, bad)


def test_every_stream_entry_point_has_a_case():
  """a new entry point with a `stream` parameter fails here until the checklist above maps it to a case"""
  text = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  header = {name for name, args in re.findall(r'\bint\s+(lddl_\w+)\s*\(([^;{]*)\)\s*;', text) if re.search(r'void\s*\*\s*stream', args)}
  listed = dict(re.findall(r'^  (lddl_\w+) +(\S.*)$', __doc__, flags=re.M))
  assert header and set(listed) == header, (sorted(header - set(listed)), sorted(set(listed) - header))
  names = [c.id for c in SC.CASES] + ['test_two_streams_one_ctx']
  for entry, prefixes in listed.items():
    for pre in prefixes.split():
      assert any(n.startswith(pre) for n in names), '%s: no case %s*' % (entry, pre)
