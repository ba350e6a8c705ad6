"""lddl_set_mask_budget, the switch itself: what it refuses, that a refused value
leaves it as it was, span masking beside it, and off again."""
import ctypes

import numpy as np
import pytest
import torch

import budget_model as bm
import mask_model as mm
import synth_vocab as sv
from lddl_amd import _lib

pytestmark = pytest.mark.gpu
EINVAL, SEED, COUNTER = -1, 31, 9


def run(tok, ids, sp):
  """lddl_mask_tokens on the ctx as it stands (p 0.5, ignore_index -1): rc, input_ids, labels"""
  x, s = torch.from_numpy(ids).cuda(), torch.from_numpy(sp).cuda()
  lab = torch.full_like(x, 7)
  ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
  rc = _lib.lib().lddl_mask_tokens(tok.handle, ptr(x), ptr(s), ptr(lab), ids.shape[0], ids.shape[1], 0.5, -1, SEED, COUNTER,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  return rc, x.cpu().numpy(), lab.cpu().numpy()


def test_switch(gpu):
  from lddl_amd.loader import BertCollate
  from lddl_amd.tokenizer import Tokenizer
  L, tok = _lib.lib(), Tokenizer(sv.vocab_path('tiny64'), 0)
  ids = np.random.default_rng(1).integers(5, 31, (5, 70)).astype(np.int64)
  sp = (np.arange(350).reshape(5, 70) % 9 == 0).astype(np.int64)
  never = run(tok, ids, sp)
  off = mm.mask(ids, sp, SEED, COUNTER, 0.5, tok.mask_id, 64, -1)
  assert never[0] == 0 and np.array_equal(never[1], off.input_ids) and np.array_equal(never[2], off.labels)
  assert L.lddl_set_mask_budget(None, 5) == EINVAL and L.lddl_last_error() == b'null ctx'
  assert L.lddl_set_mask_budget(tok.handle, 5) == 0
  assert L.lddl_set_mask_budget(tok.handle, -1) == EINVAL and L.lddl_set_mask_budget(tok.handle, -(1 << 31)) == EINVAL
  on = bm.mask(ids, sp, None, SEED, COUNTER, 0.5, 5, tok.mask_id, 64, -1)  # still 5
  got = run(tok, ids, sp)
  assert got[0] == 0 and np.array_equal(got[1], on.input_ids) and np.array_equal(got[2], on.labels)
  assert (on.select.sum(1) == 5).all() and not np.array_equal(on.labels, off.labels)
  # span masking beside it: the dynamic call is refused and writes nothing; the constructor refuses before any ctx
  assert L.lddl_set_span_mask(tok.handle, 3, 0.5) == 0
  rc, x, lab = run(tok, ids, sp)
  assert rc == EINVAL and b'span' in L.lddl_last_error() and np.array_equal(x, ids) and (lab == 7).all()
  with pytest.raises(ValueError, match='span_mask'):
    BertCollate(vocab_file='/nonexistent', span_mask=True, max_predictions=5)
  # off again: the bits of the ctx that never had it on
  assert L.lddl_set_span_mask(tok.handle, 0, 0.0) == 0 and L.lddl_set_mask_budget(tok.handle, 0) == 0
  again = run(tok, ids, sp)
  assert again[0] == 0 and np.array_equal(again[1], never[1]) and np.array_equal(again[2], never[2])
