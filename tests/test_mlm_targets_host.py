"""Compact MLM targets without a GPU: the numpy definition
(tests/mlm_targets_model.py) on hand-written cases, the registration of
lddl_mlm_targets (header, lddl_amd/_lib.py:SIGNATURES, the built library) and
the constructor argument of the two collates."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mlm_targets_model as tm
from conftest import ROOT

I = -1


def test_model_padded_rows():
  labels = [[I, 7, I, 9], [I, I, I, I], [5, I, I, 6]]
  t = tm.targets(labels, I)
  assert t.positions.tolist() == [1, 3, 8, 11]
  assert t.target_labels.tolist() == [7, 9, 5, 6]
  assert t.offsets.tolist() == [0, 2, 2, 4] and t.offsets.dtype == np.int32
  assert t.count == 4 and t.positions.dtype == t.target_labels.dtype == np.int64


def test_model_empty_result():
  t = tm.targets(np.full((2, 3), -100), -100)
  assert t.count == 0 and t.positions.size == 0 and t.target_labels.size == 0
  assert t.offsets.tolist() == [0, 0, 0]
  t = tm.targets(np.full((2, 3), -100), -100, capacity=2)
  assert t.positions.tolist() == [0, 0] and t.target_labels.tolist() == [-100, -100]


def test_model_padded_tail():
  t = tm.targets([[I, 4], [3, I]], I, capacity=5)
  assert t.count == 2
  assert t.positions.tolist() == [1, 2, 0, 0, 0]
  assert t.target_labels.tolist() == [4, 3, I, I, I]
  assert t.offsets.tolist() == [0, 1, 2]
  with pytest.raises(AssertionError):
    tm.targets([[1, 2]], I, capacity=1)


def test_model_offsets_layout_with_a_row_of_zero_length_and_an_ignored_tail():
  labels = np.asarray([8, I, 2, 1 << 40, I, 6, 7], np.int64)
  # row 1 is empty; tokens 5 and 6 lie in no row; ignore_index -1 keeps the label 0 apart
  labels[2] = 0
  t = tm.targets(labels, I, cu_seqlens=[0, 2, 2, 5])
  assert t.positions.tolist() == [0, 2, 3]
  assert t.target_labels.tolist() == [8, 0, 1 << 40]
  assert t.offsets.tolist() == [0, 1, 1, 3]
  # the same labels as rows that tile the tensor: both layouts agree
  a = tm.targets(labels[:6].reshape(2, 3), I)
  b = tm.targets(labels[:6], I, cu_seqlens=[0, 3, 6])
  assert a.positions.tolist() == b.positions.tolist() and a.offsets.tolist() == b.offsets.tolist()


def test_entry_is_registered_declared_and_exported():
  from lddl_amd import _lib, build
  assert 'lddl_mlm_targets' in _lib.SIGNATURES
  res, args = _lib.SIGNATURES['lddl_mlm_targets']
  assert res is ctypes.c_int and len(args) == 13
  src = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
  m = re.search(r'\bint\s+lddl_mlm_targets\s*\(([^;]*?)\)\s*;', src, flags=re.S)
  assert m, 'include/lddl_amd.h does not declare lddl_mlm_targets'
  assert len(m.group(1).split(',')) == len(args)
  build.build_hip()
  assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'lddl_mlm_targets')


@pytest.mark.parametrize('name', ['BertCollate', 'CodeCollate'])
def test_constructor_takes_compact_mlm_and_refuses_a_label_as_ignore_index(name):
  from lddl_amd import loader
  cls = getattr(loader, name)
  p = inspect.signature(cls.__init__).parameters
  assert 'compact_mlm' in p and p['compact_mlm'].default is False
  assert 'capacity' in inspect.signature(cls.mlm_targets).parameters
  # refused before anything touches a GPU or a vocabulary file
  for compact in (True, 64):
    for ignore in (0, 5):
      with pytest.raises(ValueError, match='ignore_index'):
        cls(vocab_file='/nonexistent/vocab.txt', ignore_index=ignore, compact_mlm=compact)
  with pytest.raises(ValueError, match='compact_mlm'):
    cls(vocab_file='/nonexistent/vocab.txt', compact_mlm=-1)
