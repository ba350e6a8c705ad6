"""What lddl_set_split_props / lddl_split_len / lddl_split refuse, each with
its code and message: NULL pointers, negative counts, a mode other than 0 or
1, a missing property table, 2^31 bytes, record offsets that do not start at
0, run backwards or end off nbytes, invalid UTF-8 of every kind (with the
lowest bad record named, also when several pieces hold one), and in
lddl_split an n_sent, out_bytes or d_doc_sent_off that is not the length
call's -- with the output buffers and the canary bytes behind them untouched.
Every case is an argument error the library must refuse; none is meant to
fault."""
import ctypes

import numpy as np
import pytest
import torch

import split_model as M
from lddl_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, EFORMAT, ECAPACITY = -1, -3, -6
CANARY = 0xAB


@pytest.fixture(scope='module')
def tok(gpu):
  from lddl_amd import splitgpu
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer()
  splitgpu.set_props(t)
  yield t
  t.close()


def dev(a, dtype):
  a = np.array(a, dtype=dtype)
  return torch.from_numpy(a).cuda() if a.size else torch.empty(0, dtype=getattr(torch, np.dtype(dtype).name), device='cuda')


def ptr(t):
  return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def last_error():
  return _lib.lib().lddl_last_error().decode()


class Case:
  """one input on the device, the length call's outputs and the fill call's buffers (with canaries)"""

  def __init__(self, raws, mode=0):
    self.buf, self.rec_off = M.join(raws)
    self.n_rec, self.nbytes, self.mode = len(raws), len(self.buf), mode
    self.d_buf = dev(np.frombuffer(self.buf, np.uint8), np.uint8)
    self.d_rec = dev(self.rec_off, np.int64)
    self.dso = torch.full((self.n_rec + 1,), -5, dtype=torch.int64, device='cuda')
    self.id_end = torch.full((max(self.n_rec, 1),), -5, dtype=torch.int64, device='cuda')
    self.tot = (ctypes.c_int64 * 2)(-9, -9)
    self.bad = ctypes.c_int64(-9)

  def len_args(self, h):
    return [h, ptr(self.d_buf), self.nbytes, ptr(self.d_rec), self.n_rec, self.mode, ptr(self.dso), ptr(self.id_end),
            self.tot, ctypes.byref(self.bad), None]

  def length(self, h, **over):
    a = self.len_args(h)
    for k, v in over.items():
      a[int(k[1:])] = v
    return _lib.lib().lddl_split_len(*a)

  def fill_buffers(self):
    n_sent, out_bytes = int(self.tot[0]), int(self.tot[1])
    self.data = torch.full((out_bytes + 16 + 64,), CANARY, dtype=torch.uint8, device='cuda')
    self.so = torch.full((n_sent + 1 + 8,), -77, dtype=torch.int64, device='cuda')

  def fill(self, h, **over):
    a = [h, ptr(self.d_buf), self.nbytes, ptr(self.d_rec), self.n_rec, self.mode, ptr(self.dso), int(self.tot[0]),
         int(self.tot[1]), ptr(self.data), ptr(self.so), None]
    for k, v in over.items():
      a[int(k[1:])] = v
    rc = _lib.lib().lddl_split(*a)
    torch.cuda.synchronize()
    return rc

  def untouched(self):
    return bool((self.data == CANARY).all()) and bool((self.so == -77).all())


RECS = [b'id One. Two. Three', b'x A b. C', b'', b'id2 Mr. Smith went. He left.']


def refused(rc, code, *words):
  assert rc == code, (rc, last_error())
  msg = last_error()
  for w in words:
    assert w in msg, msg


def test_props_refusals(tok):
  L = _lib.lib()
  tab = np.zeros(0x110000, np.uint8)
  p = ctypes.c_void_p(tab.ctypes.data)
  refused(L.lddl_set_split_props(None, p, tab.size), EINVAL, 'null ctx')
  refused(L.lddl_set_split_props(tok.handle, None, tab.size), EINVAL, 'null pointer')
  refused(L.lddl_set_split_props(tok.handle, p, 0x10FFFF), EINVAL, 'lddl_set_split_props', '1114111')
  refused(L.lddl_set_split_props(tok.handle, p, 0), EINVAL, 'lddl_set_split_props')


def test_props_not_set(gpu):
  from lddl_amd.tokenizer import Tokenizer
  t = Tokenizer()
  try:
    c = Case(RECS)
    refused(c.length(t.handle), EINVAL, 'lddl_split_len', 'lddl_set_split_props')
    c.tot[0] = c.tot[1] = 0
    c.fill_buffers()
    refused(c.fill(t.handle), EINVAL, 'lddl_split:', 'lddl_set_split_props')
    assert c.untouched()
  finally:
    t.close()


def test_len_argument_refusals(tok):
  h = tok.handle
  c = Case(RECS)
  refused(c.length(None), EINVAL, 'null ctx')
  for k in ('a1', 'a3', 'a6', 'a7', 'a8', 'a9'):  # d_buf, d_rec_off, d_out_doc_sent_off, d_out_id_end, totals, bad
    refused(c.length(h, **{k: None}), EINVAL, 'null pointer')
  refused(c.length(h, a2=-1), EINVAL, 'negative count')
  refused(c.length(h, a4=-1), EINVAL, 'negative count')
  for m in (2, -1):
    refused(c.length(h, a5=m), EINVAL, 'lddl_split_len', 'mode %d' % m)
  refused(c.length(h, a2=1 << 31), ECAPACITY, 'lddl_split_len', '2^31')
  # d_out_id_end may be NULL in mode 1 only
  c1 = Case(RECS, mode=1)
  assert c1.length(h, a7=None) == 0, last_error()
  assert c.length(h) == 0, last_error()
  assert c.bad.value == -1


@pytest.mark.parametrize('rec_off, nbytes', [([1, 4, 8], 8), ([0, 6, 4, 8], 8), ([0, 4, 7], 8), ([0, 4, 9], 8),
                                             ([0, -3, 8], 8), ([0, 100, 8], 8), ([0], 8), ([3], 0)])
def test_record_offsets_refused(tok, rec_off, nbytes):
  c = Case([b'id A. B.'])
  c.d_rec = dev(rec_off, np.int64)
  c.n_rec = len(rec_off) - 1
  c.nbytes = nbytes
  c.dso = torch.zeros(c.n_rec + 1, dtype=torch.int64, device='cuda')
  c.id_end = torch.zeros(max(c.n_rec, 1), dtype=torch.int64, device='cuda')
  refused(c.length(tok.handle), EINVAL, 'lddl_split_len', 'd_rec_off')
  c.tot[0] = c.tot[1] = 0
  c.fill_buffers()
  refused(c.fill(tok.handle), EINVAL, 'lddl_split:', 'd_rec_off')
  assert c.untouched()


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('raw', M.INVALID)
def test_invalid_utf8(tok, raw, mode):
  for raws, low in (([raw], 0), ([b'ok A. B.', b'', raw, b'fine. C', raw], 2)):
    c = Case(raws, mode)
    refused(c.length(tok.handle), EFORMAT, 'lddl_split_len', 'record %d' % low, 'UTF-8')
    assert c.bad.value == low
    c.tot[0] = c.tot[1] = 1
    c.fill_buffers()
    refused(c.fill(tok.handle), EFORMAT, 'lddl_split:', 'record %d' % low)
    assert c.untouched()


def test_truncated_then_continuation(tok):
  """the buffer as a whole decodes; the record cut inside a sequence is the lowest bad one"""
  c = Case([b'ok. Fine', b'id trunc \xe2\x82', b'', b'\xac rest. A', b'id good'])
  refused(c.length(tok.handle), EFORMAT, 'record 1')
  assert c.bad.value == 1
  c = Case([b'\xac rest. A'])
  refused(c.length(tok.handle), EFORMAT, 'record 0')
  assert c.bad.value == 0


def test_lowest_bad_record_over_many_pieces(tok):
  """bad records in pieces 2, 5 and 9 (and a clean start): the lowest is named whichever wave finds its own"""
  good = ('id ' + 'Some words here. ' * 60).encode()  # ~1 KB
  raws = [good] * 40
  for r in (9, 21, 37):
    raws[r] = good[:500] + M.INVALID[r % len(M.INVALID)] + good[500:]
  c = Case(raws)
  assert c.rec_off[9] // M.PIECE != c.rec_off[21] // M.PIECE != c.rec_off[37] // M.PIECE
  refused(c.length(tok.handle), EFORMAT, 'record 9')
  assert c.bad.value == 9
  raws[9] = good
  c = Case(raws)
  refused(c.length(tok.handle), EFORMAT, 'record 21')
  assert c.bad.value == 21


def test_fill_argument_refusals(tok):
  h = tok.handle
  c = Case(RECS)
  assert c.length(h) == 0, last_error()
  c.fill_buffers()
  refused(c.fill(None), EINVAL, 'null ctx')
  for k in ('a1', 'a3', 'a6', 'a9', 'a10'):  # d_buf, d_rec_off, d_doc_sent_off, d_out_data, d_out_sent_off
    refused(c.fill(h, **{k: None}), EINVAL, 'null pointer')
  for k in ('a2', 'a4', 'a7', 'a8'):
    refused(c.fill(h, **{k: -1}), EINVAL, 'negative count')
  refused(c.fill(h, a5=2), EINVAL, 'lddl_split:', 'mode 2')
  refused(c.fill(h, a2=1 << 31), ECAPACITY, 'lddl_split:', '2^31')
  assert c.untouched()


@pytest.mark.parametrize('mode', [0, 1])
def test_fill_refuses_what_the_length_call_did_not_give(tok, mode):
  h = tok.handle
  recs = [r.encode('utf-8') for r in M.adversarial(1, 200)]
  c = Case(recs, mode)
  assert c.length(h) == 0, last_error()
  n_sent, out_bytes = int(c.tot[0]), int(c.tot[1])
  assert n_sent > 100 and out_bytes > 1000
  c.fill_buffers()
  for d in (-1, 1):
    refused(c.fill(h, a7=n_sent + d), EINVAL, 'lddl_split:', 'n_sent')
    assert c.untouched()
    refused(c.fill(h, a8=out_bytes + d), EINVAL, 'lddl_split:', 'out_bytes')
    assert c.untouched()
  refused(c.fill(h, a7=c.nbytes + 1), EINVAL, 'lddl_split:', 'n_sent')
  good = c.dso.clone()
  for i, d in ((0, 1), (1, -1), (c.n_rec // 2, 1), (c.n_rec, -1), (c.n_rec - 1, 1 << 40)):
    c.dso = good.clone()
    c.dso[i] += d
    if i == c.n_rec:  # (its last entry is n_sent: both are then altered together)
      refused(c.fill(h, a7=n_sent + d), EINVAL, 'lddl_split:')
    else:
      refused(c.fill(h), EINVAL, 'lddl_split:', 'd_doc_sent_off')
    assert c.untouched()
  # and the untouched values fill: the canaries behind both outputs stay
  c.dso = good
  assert c.fill(h) == 0, last_error()
  data, so = c.data.cpu().numpy(), c.so.cpu().numpy()
  edata, eso, _, _ = M.reference([r.decode('utf-8') for r in recs], bool(mode))
  assert data[:out_bytes].tobytes() == edata and not data[out_bytes:out_bytes + 16].any()
  assert (data[out_bytes + 16:] == CANARY).all()
  assert np.array_equal(so[:n_sent + 1], eso) and (so[n_sent + 1:] == -77).all()
