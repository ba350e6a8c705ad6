"""The refusals of the C API as a table, shared by tests/test_capi_errors_gpu.py
(replays it against the working tree's library) and
tools/gen_golden_capi_errors.py (records tests/golden/capi_errors.json from
the parent commit's library).  Plain helper module: no fixtures, no tests.

run_all() yields (call, case, rc, message) in a fixed order.  Every case
takes a valid tiny call -- real device tensors of 3 rows, a 4-sentence
tokenizer input, 2 partitions -- and changes the arguments named in the case
so that exactly one refusal fires before anything is launched; a refusal that
failed to fire would run the valid call.  The state refusals run on ctxs
brought into the state they name.  Left out: "pack result of another device"
(needs two GPUs) and lddl_collate_rows_cu_seqlens' n_rows > INT32_MAX / 3
(no valid call has that many rows; tests/test_collate_unpadded_gpu.py covers it).
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_vocab as sv  # noqa: E402
from lddl_amd import _lib  # noqa: E402

NAN = float('nan')
SENTS = [b'a b c', b'the of a', b'b c', b'of the in a']


def T(a, dtype):
  a = np.asarray(a)
  if dtype == 'u16':
    return torch.from_numpy(a.astype(np.uint16).view(np.int16)).cuda()
  return torch.from_numpy(a.astype(dtype)).cuda()


def Z(n, dtype):
  return T(np.zeros(n, np.int64), dtype)


class Env:
  """tensors of the valid calls; ctxs in the states the cases need"""

  def __init__(self):
    from lddl_amd.tokenizer import Tokenizer
    from lddl_amd import writer
    self.L = _lib.lib()
    self.path = sv.vocab_path('tiny64')
    self.keep = []
    self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    # tokenizer input and outputs
    self.bytes = T(np.frombuffer(b''.join(SENTS) + b'\0' * 16, np.uint8), np.uint8)
    self.nbytes = sum(map(len, SENTS))
    self.sent_off = T(np.concatenate([[0], np.cumsum([len(s) for s in SENTS])]), np.int64)
    self.ids, self.ntok, self.tok_off = Z(64, 'u16'), Z(4, np.int32), Z(5, np.int64)
    self.doc_sent_off, self.part_doc_off = T([0, 2, 4], np.int64), T([0, 1, 2], np.int64)
    self.nseg = T([1, 1], np.int32)
    self.totals = (ctypes.c_int64 * 4)()
    # outputs of the post-pack calls: room for 64 rows of 16 tokens
    self.o_tokens, self.o_off = Z(1024, 'u16'), Z(65, np.int64)
    self.o_len0, self.o_len1, self.o_flags, self.o_bin = Z(64, 'u16'), Z(64, 'u16'), Z(64, np.uint8), Z(64, np.uint8)
    self.o_part, self.o_bc, self.o_src0, self.o_src1 = Z(64, np.int64), Z(64, np.int64), Z(64, np.int64), Z(64, np.int64)
    self.o_moff, self.o_mpos, self.o_mlab, self.o_mtok = Z(65, np.int64), Z(1024, 'u16'), Z(1024, 'u16'), Z(1024, 'u16')
    self.o_doc = Z(64, np.int64)
    # 3 rows with segment lengths (1, 1), (0, 5), (7, 2): materialized rows and spans over 18 dense ids
    segs = ((1, 1), (0, 5), (7, 2))
    lens = [a + b + 3 for a, b in segs]
    self.n = 3
    self.total = sum(lens)
    self.r_ids = T(np.concatenate([6 + np.arange(18), np.zeros(16, np.int64)]), 'u16')
    self.r_src0, self.r_src1 = T([1, 3, 9], np.int64), T([2, 3, 16], np.int64)
    self.r_len0, self.r_len1 = T([a for a, _ in segs], 'u16'), T([b for _, b in segs], 'u16')
    self.r_flags = T([2, 3, 2], np.uint8)
    rows = [[2] + list(range(10, 10 + a)) + [3] + list(range(30, 30 + b)) + [3] for a, b in segs]
    self.r_tokens = T([x for r in rows for x in r] + [0] * 16, 'u16')
    self.r_tok_off = T(np.concatenate([[0], np.cumsum(lens)]), np.int64)
    self.r_rows = T([2, 0, 1], np.int64)
    self.m_off, self.m_pos = T([0, 1, 2, 3], np.int64), T([1, 2, 3], 'u16')
    self.m_lab, self.m_tok = T([30, 31, 32], 'u16'), T([4, 33, 4], 'u16')
    self.cu = T(np.concatenate([[0], np.cumsum([lens[g] for g in (2, 0, 1)])]), np.int32)
    self.out_off, self.nb, self.i64a, self.i64b = Z(4, np.int64), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    self.pad = [torch.zeros((3, 12), dtype=torch.int64, device='cuda') for _ in range(5)]
    self.flat = [torch.zeros(self.total, dtype=torch.int64, device='cuda') for _ in range(4)]
    self.nsl = Z(3, np.int64)
    self.lens5, self.perm, self.counts = T([3, 9, 5, 12, 7], np.int64), Z(5, np.int64), Z(2, np.int64)
    self.hdr, self.hlen, self.kmax = writer.npy_header_table(torch.device('cuda', 0), 1024)
    # string columns of lddl_collate_seq_len / lddl_collate_bert
    A, B = [b'a', b'', b'a b c d e f g'], [b'b', b'a b c d e', b'the of']
    col = lambda v: (T(np.frombuffer(b''.join(v) + b'\0' * 16, np.uint8), np.uint8),  # noqa: E731
                     T(np.concatenate([[0], np.cumsum([len(x) for x in v])]), np.int64))
    (self.a, self.a_off), (self.b, self.b_off) = col(A), col(B)
    self.rn = T([0, 1, 0], np.uint8)
    # masked_lm_positions as np.save bytes, masked_lm_labels as words
    npy = [bytes(writer._npy_header(1).tobytes()) + np.asarray([p], np.uint16).tobytes() for p in (1, 2, 3)]
    (self.pos, self.pos_off), (self.lab, self.lab_off) = col(npy), col([b'a', b'b', b'c'])
    self.vbuf = ctypes.create_string_buffer(64)
    self.sp = (ctypes.c_int32 * 5)()
    self.stats = (ctypes.c_double * 6)()
    self.algo = ctypes.c_int()
    self.newpk = ctypes.c_void_p()
    self.tok = Tokenizer  # (the class: new ctxs below)
    self.c0 = self.ctx()   # never packs
    self.c = self.ctx()    # unmasked pack
    self.cm = self.ctx()   # masked pack
    self.big = self.ctx(sv.vocab_path('v65536'))  # 65 536 entries: masking is refused
    for c in (self.c, self.cm):
      assert self.call('lddl_tokenize', self.tokenize(c)) == 0, self.L.lddl_last_error()
    assert self.call('lddl_pack_bert', self.pack_bert(self.c)) == 0, self.L.lddl_last_error()
    assert self.call('lddl_pack_bert', self.pack_bert(self.cm, masking=1, ratio=0.5)) == 0, self.L.lddl_last_error()
    assert self.totals[0] > 0 and self.totals[3] > 0, list(self.totals)

  def ctx(self, path=None):
    t = self.tok(path or self.path, 0)
    self.keep.append(t)
    return t.handle

  def call(self, name, args):
    return getattr(self.L, name)(*args.values())

  # ---- the valid calls, as ordered name -> value ---------------------------------
  def tokenize(self, c):
    return dict(c=c, bytes=self.bytes.data_ptr(), nbytes=self.nbytes, sent_off=self.sent_off.data_ptr(), n_sent=4,
                max_tok=16, out_ids=self.ids.data_ptr(), out_cap=48, out_ntok=self.ntok.data_ptr(),
                out_tok_off=self.tok_off.data_ptr(), stream=self.st)

  def pack_bert(self, c, masking=0, ratio=0.15):
    return dict(c=c, pk=None, ids=self.ids.data_ptr(), ntok=self.ntok.data_ptr(), tok_off=self.tok_off.data_ptr(),
                sent_off=self.sent_off.data_ptr(), n_sent=4, doc_sent_off=self.doc_sent_off.data_ptr(), n_doc=2,
                part_doc_off=self.part_doc_off.data_ptr(), n_part=2, seq=16, ssp=0.1, dup=1, masking=masking, ratio=ratio,
                seed=1, bin_size=0, totals=self.totals, stream=self.st)

  def pack_codebert(self, c):
    return dict(c=c, pk=None, ntok=self.ntok.data_ptr(), tok_off=self.tok_off.data_ptr(),
                sent_off=self.sent_off.data_ptr(), n_sent=4, doc_sent_off=self.doc_sent_off.data_ptr(),
                nseg=self.nseg.data_ptr(), n_doc=2, part_doc_off=self.part_doc_off.data_ptr(), n_part=2, seq=16, ssp=0.1,
                dup=1, seed=1, bin_size=0, totals=self.totals, stream=self.st)

  def _row_outs(self):
    return dict(tok_off=self.o_off.data_ptr(), len0=self.o_len0.data_ptr(), len1=self.o_len1.data_ptr(),
                flags=self.o_flags.data_ptr(), bin=self.o_bin.data_ptr(), part=self.o_part.data_ptr(),
                bin_count=self.o_bc.data_ptr(), stream=self.st)

  def materialize(self, c):
    return dict(c=c, pk=None, ids=self.ids.data_ptr(), tokens=self.o_tokens.data_ptr(), **self._row_outs())

  def row_spans(self, c):
    return dict(c=c, pk=None, src0=self.o_src0.data_ptr(), src1=self.o_src1.data_ptr(), **self._row_outs())

  def masked_lm(self, c):
    return dict(c=c, pk=None, off=self.o_moff.data_ptr(), pos=self.o_mpos.data_ptr(), label=self.o_mlab.data_ptr(),
                stream=self.st)

  def masked_lm_spans(self, c):
    return dict(c=c, pk=None, ids=self.ids.data_ptr(), src0=self.o_src0.data_ptr(), src1=self.o_src1.data_ptr(),
                len0=self.o_len0.data_ptr(), part=self.o_part.data_ptr(), off=self.o_moff.data_ptr(),
                pos=self.o_mpos.data_ptr(), label=self.o_mlab.data_ptr(), token=self.o_mtok.data_ptr(), stream=self.st)

  def row_docs(self, c):
    return dict(c=c, pk=None, doc=self.o_doc.data_ptr(), stream=self.st)

  def bin(self, c):
    return dict(c=c, num_tokens=self.lens5.data_ptr(), n=5, bin_size=8, nbins=2, perm=self.perm.data_ptr(),
                counts=self.counts.data_ptr(), stream=self.st)

  def _render_out(self):
    return dict(out_off=self.out_off.data_ptr(), out_bytes=None, out_cap=0, nbytes=ctypes.byref(self.nb), stream=self.st)

  def render_strings(self, c):
    return dict(c=c, tokens=self.r_tokens.data_ptr(), row_off=self.r_tok_off.data_ptr(), len0=self.r_len0.data_ptr(),
                len1=self.r_len1.data_ptr(), flags=self.r_flags.data_ptr(), row0=0, n_rows=3, segment=1, codebert=1,
                **self._render_out())

  def render_npy(self, c):
    return dict(c=c, mlm_off=self.m_off.data_ptr(), mlm_pos=self.m_pos.data_ptr(), row0=0, n_rows=3,
                hdr=self.hdr.data_ptr(), hdr_len=self.hlen, kmax=self.kmax, **self._render_out())

  def render_masked(self, c):
    return dict(c=c, ids=self.r_ids.data_ptr(), src=self.r_src0.data_ptr(), len=self.r_len0.data_ptr(),
                len0=self.r_len0.data_ptr(), segment=0, mlm_off=self.m_off.data_ptr(), mlm_pos=self.m_pos.data_ptr(),
                mlm_token=self.m_tok.data_ptr(), row0=0, n_rows=3, **self._render_out())

  def _cols(self):
    return dict(a=self.a.data_ptr(), a_off=self.a_off.data_ptr(), b=self.b.data_ptr(), b_off=self.b_off.data_ptr())

  def collate_seq_len(self, c):
    return dict(c=c, **self._cols(), n_rows=3, seq_align=1, out=ctypes.byref(self.i64a), stream=self.st)

  def _model_outs(self, bufs, third):
    return dict(input_ids=bufs[0].data_ptr(), token_type_ids=bufs[1].data_ptr(), **{third: bufs[2].data_ptr()},
                labels=bufs[3].data_ptr(), nsl=self.nsl.data_ptr(), stream=self.st)

  def collate_bert(self, c):
    return dict(c=c, **self._cols(), rn=self.rn.data_ptr(), pos=self.pos.data_ptr(), pos_off=self.pos_off.data_ptr(),
                lab=self.lab.data_ptr(), lab_off=self.lab_off.data_ptr(), n_rows=3, seq_len=12, mode=1, ignore_index=-1,
                prob=0.15, seed=1, counter=0, **self._model_outs(self.pad, 'attention_mask'))

  def mask_tokens(self, c):
    return dict(c=c, inputs=self.pad[0].data_ptr(), special=self.pad[1].data_ptr(), labels=self.pad[3].data_ptr(),
                n_rows=3, seq_len=12, prob=0.15, ignore_index=-1, seed=1, counter=0, stream=self.st)

  def _sel(self):
    return dict(len0=self.r_len0.data_ptr(), len1=self.r_len1.data_ptr(), rows=self.r_rows.data_ptr(), row0=0, n_rows=3,
                n_total=3)

  def collate_rows_seq_len(self, c):
    return dict(c=c, **self._sel(), seq_align=1, out=ctypes.byref(self.i64a), stream=self.st)

  def _spans(self):
    sel = self._sel()
    return dict(ids=self.r_ids.data_ptr(), src0=self.r_src0.data_ptr(), src1=self.r_src1.data_ptr(), len0=sel.pop('len0'),
                len1=sel.pop('len1'), flags=self.r_flags.data_ptr(), **sel, mlm_off=self.m_off.data_ptr(),
                mlm_pos=self.m_pos.data_ptr(), mlm_label=self.m_lab.data_ptr(), mlm_token=self.m_tok.data_ptr())

  def collate_rows(self, c):
    return dict(c=c, **self._spans(), seq_len=12, mode=1, ignore_index=-1, prob=0.15, seed=1, counter=0,
                **self._model_outs(self.pad, 'attention_mask'))

  def cu_seqlens(self, c):
    return dict(c=c, **self._sel(), cu=self.cu.data_ptr(), total=ctypes.byref(self.i64a),
                longest=ctypes.byref(self.i64b), stream=self.st)

  def collate_rows_unpadded(self, c):
    return dict(c=c, **self._spans(), cu=self.cu.data_ptr(), total=self.total, mode=1, ignore_index=-1, prob=0.15, seed=1,
                counter=0, **self._model_outs(self.flat, 'position_ids'))


def null(*names):
  return {n: None for n in names}


# call -> (builder, [(case, overrides)]): argument validation on a ctx that has packed (unmasked)
def validation(E):
  model_ptrs = ['input_ids', 'token_type_ids', 'labels', 'nsl']
  span_ptrs = ['ids', 'src0', 'src1', 'len0', 'len1', 'flags']
  mlm_ptrs = ['mlm_off', 'mlm_pos', 'mlm_label', 'mlm_token']
  each = lambda names, tag='null': [('%s %s' % (tag, n), null(n)) for n in names]  # noqa: E731
  sizes = lambda *names: [('%s -1' % n, {n: -1}) for n in names]  # noqa: E731
  modes = [('mode -1', dict(mode=-1)), ('mode 3', dict(mode=3))]
  probs = [('prob 1.5', dict(prob=1.5)), ('prob -0.1', dict(prob=-0.1)), ('prob nan', dict(prob=NAN))]
  pack_common = ([('n_part 0', dict(n_part=0))] + sizes('n_doc', 'n_sent') +
                 each(['ntok', 'tok_off', 'sent_off', 'doc_sent_off', 'part_doc_off', 'totals']) + [
                     ('seq 4', dict(seq=4)), ('seq 32769', dict(seq=32769)), ('dup 0', dict(dup=0)),
                     ('bin_size 32', dict(bin_size=32)), ('bin_size 5', dict(bin_size=5)),
                     ('more than 255 bins', dict(seq=512, bin_size=1))])
  rows_common = (sizes('n_rows', 'n_total') + modes + probs + each(span_ptrs + model_ptrs) +
                 each(mlm_ptrs, 'static null'))
  return [
      ('lddl_tokenize', E.tokenize, sizes('n_sent', 'nbytes', 'out_cap') + [
          ('max_tok 0', dict(max_tok=0)), ('max_tok 65535', dict(max_tok=65535))] +
       each(['out_tok_off', 'bytes', 'sent_off', 'out_ids', 'out_ntok']) + [
           ('n_sent 0 null out_tok_off', dict(n_sent=0, out_tok_off=None))]),
      ('lddl_pack_bert', E.pack_bert, [
          ('masking null ids', dict(masking=1, ids=None)), ('masking seq 1025', dict(masking=1, seq=1025)),
          ('masking ratio 1.5', dict(masking=1, ratio=1.5)), ('masking ratio nan', dict(masking=1, ratio=NAN)),
          ] + pack_common),
      ('lddl_pack_codebert', E.pack_codebert, pack_common + each(['nseg'])),
      ('lddl_materialize', E.materialize, each(['ids', 'tokens', 'tok_off', 'len0', 'len1', 'flags', 'bin', 'part'])),
      ('lddl_row_spans', E.row_spans, each(['src0', 'src1', 'len0', 'len1', 'flags', 'bin', 'part'])),
      ('lddl_row_docs', E.row_docs, each(['doc'])),
      ('lddl_bin', E.bin, sizes('n') + [('bin_size 0', dict(bin_size=0)), ('nbins 0', dict(nbins=0)),
                                        ('nbins 1025', dict(nbins=1025))] + each(['counts', 'num_tokens', 'perm'])),
      ('lddl_render_strings', E.render_strings, [('segment -1', dict(segment=-1)), ('segment 4', dict(segment=4))] +
       sizes('row0', 'n_rows') + each(['tokens', 'row_off', 'out_off', 'nbytes']) + [
           ('seg0 null len0', dict(segment=0, len0=None)), ('seg1 null len1', dict(len1=None)),
           ('seg1 codebert null flags', dict(flags=None)), ('span null len0', dict(segment=3, len0=None)),
           ('seg0 null len0, no codebert', dict(segment=0, len0=None, codebert=0)),
           ('seg1 null len1, no codebert', dict(len1=None, codebert=0))]),
      ('lddl_render_npy', E.render_npy, sizes('row0', 'n_rows') + [
          ('hdr_len 0', dict(hdr_len=0)), ('hdr_len odd', dict(hdr_len=E.hlen + 1)), ('kmax -1', dict(kmax=-1))] +
       each(['out_off', 'nbytes', 'mlm_off', 'hdr'])),
      ('lddl_render_masked', E.render_masked, [('segment 2', dict(segment=2)), ('segment -1', dict(segment=-1))] +
       sizes('row0', 'n_rows') +
       each(['ids', 'src', 'len', 'len0', 'mlm_off', 'mlm_pos', 'mlm_token', 'out_off', 'nbytes'])),
      ('lddl_collate_seq_len', E.collate_seq_len, sizes('n_rows') + [('seq_align 0', dict(seq_align=0))] +
       each(['out', 'a', 'a_off', 'b', 'b_off']) + [('n_rows 0', dict(n_rows=0))]),
      ('lddl_collate_bert', E.collate_bert, sizes('n_rows') + modes + [
          ('seq_len 2', dict(seq_len=2)), ('seq_len 2049', dict(seq_len=2049)),
          ('ignore_index 2^31', dict(ignore_index=2**31)), ('ignore_index -2^31 - 1', dict(ignore_index=-2**31 - 1))] +
       probs + each(['a', 'a_off', 'b', 'b_off', 'rn', 'attention_mask'] + model_ptrs) +
       each(['pos', 'pos_off', 'lab', 'lab_off'], 'static null')),
      ('lddl_mask_tokens', E.mask_tokens, sizes('n_rows', 'seq_len') + [('seq_len 2^20', dict(seq_len=1 << 20))] + probs +
       each(['inputs', 'special', 'labels'])),
      ('lddl_collate_rows_seq_len', E.collate_rows_seq_len, sizes('n_rows', 'n_total') + [
          ('seq_align 0', dict(seq_align=0)), ('null out', null('out')), ('n_rows 0', dict(n_rows=0))] +
       each(['len0', 'len1'])),
      ('lddl_collate_rows', E.collate_rows, [('seq_len 2', dict(seq_len=2)), ('seq_len 2049', dict(seq_len=2049))] +
       rows_common + each(['attention_mask'])),
      ('lddl_collate_rows_cu_seqlens', E.cu_seqlens, sizes('n_rows', 'n_total') + each(['total', 'longest']) + [
          ('n_rows 0', dict(n_rows=0))] + each(['len0', 'len1', 'cu'])),
      ('lddl_collate_rows_unpadded', E.collate_rows_unpadded, [('total -1', dict(total=-1)),
                                                               ('total 2^31', dict(total=2**31))] +
       rows_common + each(['cu', 'position_ids'])),
  ]


def run_all():
  """yields (call, case, rc, message)"""
  E = Env()
  L = E.L

  def rec(call, case, rc):
    return call, case, int(rc), L.lddl_last_error().decode(errors='replace')

  for call, build, cases in validation(E):
    yield rec(call, 'null ctx', E.call(call, {**build(E.c), 'c': None}))
    for case, over in cases:
      args = build(E.c)
      assert set(over) <= set(args), (call, case)
      yield rec(call, case, E.call(call, {**args, **over}))
  # masking over a vocabulary whose ids do not fit 16 bits (the ids of the 64-entry one are valid in it)
  yield rec('lddl_pack_bert', 'masking vocab 65536', E.call('lddl_pack_bert', E.pack_bert(E.big, masking=1)))
  # the ctx-only calls
  yield rec('lddl_vocab_size', 'null ctx', L.lddl_vocab_size(None))
  yield rec('lddl_special_ids', 'null ctx', L.lddl_special_ids(None, E.sp))
  yield rec('lddl_special_ids', 'null out', L.lddl_special_ids(E.c, None))
  yield rec('lddl_vocab_token', 'null ctx', L.lddl_vocab_token(None, 5, E.vbuf, 64))
  yield rec('lddl_vocab_token', 'null buf', L.lddl_vocab_token(E.c, 5, None, 64))
  yield rec('lddl_vocab_token', 'id -1', L.lddl_vocab_token(E.c, -1, E.vbuf, 64))
  yield rec('lddl_vocab_token', 'id V', L.lddl_vocab_token(E.c, sv.vocab_size('tiny64'), E.vbuf, 64))
  yield rec('lddl_vocab_token', 'cap 1', L.lddl_vocab_token(E.c, 40, E.vbuf, 1))
  yield rec('lddl_set_special_flags', 'null ctx', L.lddl_set_special_flags(None, 1))
  yield rec('lddl_set_tokenize_algo', 'null ctx', L.lddl_set_tokenize_algo(None, 5, ctypes.byref(E.algo)))
  yield rec('lddl_set_tokenize_algo', 'algo 3', L.lddl_set_tokenize_algo(E.c, 3, ctypes.byref(E.algo)))
  yield rec('lddl_set_timing', 'null ctx', L.lddl_set_timing(None, 1))
  yield rec('lddl_tokenize_stats', 'null ctx', L.lddl_tokenize_stats(None, E.stats, 6))
  yield rec('lddl_tokenize_stats', 'null out', L.lddl_tokenize_stats(E.c, None, 6))
  yield rec('lddl_tokenize_stats', 'n 5', L.lddl_tokenize_stats(E.c, E.stats, 5))
  yield rec('lddl_tokenize_stats', 'timing off', L.lddl_tokenize_stats(E.c0, E.stats, 6))
  yield rec('lddl_pack_new', 'null ctx', L.lddl_pack_new(None, ctypes.byref(E.newpk)))
  yield rec('lddl_pack_new', 'null out', L.lddl_pack_new(E.c, None))
  # the state refusals
  for call, build in (('lddl_materialize', E.materialize), ('lddl_row_spans', E.row_spans), ('lddl_row_docs', E.row_docs)):
    yield rec(call, 'before any pack', E.call(call, build(E.c0)))
  yield rec('lddl_masked_lm', 'after an unmasked pack', E.call('lddl_masked_lm', E.masked_lm(E.c)))
  yield rec('lddl_masked_lm_spans', 'after an unmasked pack', E.call('lddl_masked_lm_spans', E.masked_lm_spans(E.c)))
  yield rec('lddl_masked_lm', 'null ctx', E.call('lddl_masked_lm', {**E.masked_lm(E.cm), 'c': None}))
  yield rec('lddl_masked_lm_spans', 'null ctx', E.call('lddl_masked_lm_spans', {**E.masked_lm_spans(E.cm), 'c': None}))
  yield rec('lddl_masked_lm', 'before lddl_materialize', E.call('lddl_masked_lm', E.masked_lm(E.cm)))
  assert E.call('lddl_row_spans', E.row_spans(E.cm)) == 0, L.lddl_last_error()
  for n in ('off', 'ids', 'src0', 'src1', 'len0', 'part', 'pos', 'label', 'token'):
    yield rec('lddl_masked_lm_spans', 'null %s' % n, E.call('lddl_masked_lm_spans', {**E.masked_lm_spans(E.cm), n: None}))
  assert E.call('lddl_materialize', E.materialize(E.cm)) == 0, L.lddl_last_error()
  for n in ('off', 'pos', 'label'):
    yield rec('lddl_masked_lm', 'null %s' % n, E.call('lddl_masked_lm', {**E.masked_lm(E.cm), n: None}))
  assert E.call('lddl_masked_lm', E.masked_lm(E.cm)) == 0, L.lddl_last_error()
  yield rec('lddl_masked_lm', 'called twice', E.call('lddl_masked_lm', E.masked_lm(E.cm)))
  torch.cuda.synchronize()
