"""No GPU: the file ordering and the bin / partition parsing of
loader.load_shards (loader.shard_files, a pure function over file names, after
lddl/utils.py:47-75; the preprocessor's part.<p> and the load balancer's
shard-<k> names), and the two entry points behind it in the header and in
_lib.SIGNATURES."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from lddl_amd import _lib
from lddl_amd.loader import shard_files


def test_binned_directory_in_partition_bin_order():
  names = ['d/part.10.parquet_1', 'd/part.2.parquet_0', 'd/_SUCCESS', 'd/part.2.parquet_1', 'd/part.10.parquet_0',
           'd/part.2.parquet_2', 'd/part.10.parquet_2', 'd/.part.2.parquet_0.crc']
  got = shard_files(names)
  assert got == [('d/part.2.parquet_0', 2, 0), ('d/part.2.parquet_1', 2, 1), ('d/part.2.parquet_2', 2, 2),
                 ('d/part.10.parquet_0', 10, 0), ('d/part.10.parquet_1', 10, 1), ('d/part.10.parquet_2', 10, 2)]
  assert shard_files(reversed(names)) == got  # numeric, not lexicographic, and independent of the listing order


def test_two_digit_bins_sort_numerically():
  names = ['part.0.parquet_%d' % b for b in (10, 9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11)]
  assert [b for _, _, b in shard_files(names)] == list(range(12))


def test_unbinned_directory():
  got = shard_files(['/x/part.1.parquet', '/x/part.0.parquet', '/x/part.11.parquet', '/x/README'])
  assert got == [('/x/part.0.parquet', 0, None), ('/x/part.1.parquet', 1, None), ('/x/part.11.parquet', 11, None)]
  assert shard_files(['notes.txt', 'vocab.txt']) == []


def test_balanced_directory():
  """the load balancer's output: shard-<k>.parquet[_<b>] next to .num_samples.json, k as the partition"""
  names = ['b/shard-10.parquet_1', 'b/.num_samples.json', 'b/shard-2.parquet_0', 'b/shard-2.parquet_1',
           'b/shard-10.parquet_0']
  assert shard_files(names) == [('b/shard-2.parquet_0', 2, 0), ('b/shard-2.parquet_1', 2, 1),
                                ('b/shard-10.parquet_0', 10, 0), ('b/shard-10.parquet_1', 10, 1)]
  assert shard_files(['shard-1.parquet', 'shard-0.parquet']) == [('shard-0.parquet', 0, None), ('shard-1.parquet', 1, None)]


def test_other_stems_are_numbered_in_sorted_order():
  assert shard_files(['x/wiki.parquet', 'x/books.parquet']) == [('x/books.parquet', 0, None), ('x/wiki.parquet', 1, None)]
  assert shard_files(['x/b.parquet_1', 'x/a.parquet_1', 'x/a.parquet_0', 'x/b.parquet_0']) == [
      ('x/a.parquet_0', 0, 0), ('x/a.parquet_1', 0, 1), ('x/b.parquet_0', 1, 0), ('x/b.parquet_1', 1, 1)]
  # part.* and shard-* together: their numbers would collide, so neither is taken
  assert shard_files(['part.0.parquet', 'shard-0.parquet']) == [('part.0.parquet', 0, None), ('shard-0.parquet', 1, None)]
  assert shard_files(['part.1x.parquet']) == [('part.1x.parquet', 0, None)]


def test_refused_names():
  with pytest.raises(ValueError, match='bin suffixes'):  # the rule of lddl/utils.py:64-66
    shard_files(['part.0.parquet_0', 'part.0.parquet_2'])
  with pytest.raises(ValueError, match='bin suffixes'):
    shard_files(['part.0.parquet_1'])
  with pytest.raises(ValueError, match='binned and unbinned'):
    shard_files(['part.0.parquet', 'part.1.parquet_0'])


def _declared():
  src = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
  return {m.group(1): ' '.join(m.group(2).split()).split(',')
          for m in re.finditer(r'\b(lddl_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S)}


def test_entry_points_declared_and_bound():
  decl = _declared()
  for name, n_args in (('lddl_rows_from_strings_len', 18), ('lddl_rows_from_strings', 24)):
    assert name in decl and len(decl[name]) == n_args, name
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == n_args
    for c_param, t in zip(decl[name], args):
      pointer = '*' in c_param or '[' in c_param
      assert pointer == (t is ctypes.c_void_p or issubclass(t, ctypes._Pointer)), (name, c_param)
      if not pointer:
        assert t is ctypes.c_int64 and 'int64_t' in c_param, (name, c_param)


def test_header_cites_the_reference_seam():
  src = open(os.path.join(ROOT, 'include', 'lddl_amd.h')).read()
  for name in ('lddl_rows_from_strings_len', 'lddl_rows_from_strings'):
    end = src.index('int %s(' % name)
    comment = src[src.rindex('/*', 0, end):end]
    assert 'bert.py' in comment and ':83-89' in comment and ':109-124' in comment, name
