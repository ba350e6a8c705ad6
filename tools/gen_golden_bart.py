#!/usr/bin/env python3
"""Golden vectors for the BART sentence aggregation, produced by the
REFERENCE's own code (run where a checkout of the reference is at hand:
LDDL_REFERENCE names it; it is read, never copied).

lddl.dask.bart.pretrain imports once dask / nltk are stubbed, as
tools/gen_golden_pack.py does for the BERT module.  The stub
``db.concat([]).map(f)`` captures the closure ``_generate_sequences`` that
``_get_sequences(target_seq_length=...)`` builds (pretrain.py:130-133), and
``nltk.tokenize.sent_tokenize`` is a split on '\\x01' (not whitespace to
Python), so an article is its raw sentences joined by '\\x01' and the
reference's own ``_segment`` (strip, drop empty) and ``_aggregate_sentences``
run on them unchanged.

Writes tests/golden/bart_chunks.json.gz (data only): the articles and, per
target_seq_length, the dictionaries the closure returned.
"""
import gzip
import json
import os
import random
import sys
import unittest.mock as mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'bart_chunks.json.gz')
TARGETS = [3, 4, 8, 128, 512]

# every character str.isspace() accepts (what str.split() splits on; lddl_amd/csrc/collate_dev.h py_space)
PY_SPACE = [chr(c) for c in list(range(9, 14)) + list(range(0x1c, 0x21)) + [0x85, 0xa0, 0x1680] +
            list(range(0x2000, 0x200b)) + [0x2028, 0x2029, 0x202f, 0x205f, 0x3000]]
WORDS = ('the of and to in a is was for on as by with he that at from his it an were are which this be or had '
         'first one their has not but new also its two they who been other when time she there all into more '
         'naïve café über straße 東京 大阪府 日本語 '
         '中文 \U0001f600 x y z 1999 3.14 e.g. U.S. co-op').split(' ')


def load_reference():
  captured = {}

  class Bag:
    def map(self, f):
      captured['f'] = f
      return mock.MagicMock()

  mods = {m: mock.MagicMock() for m in ['dask', 'dask.bag', 'dask.distributed', 'dask.highlevelgraph', 'dask.base',
                                        'dask.bag.core', 'dask.delayed', 'dask.utils', 'dask.dataframe',
                                        'dask.dataframe.core', 'dask.dataframe.io', 'dask.dataframe.io.parquet',
                                        'dask.dataframe.io.parquet.core', 'dask.dataframe.io.parquet.arrow',
                                        'dask.bytes', 'tlz', 'nltk', 'nltk.tokenize', 'dask_mpi']}
  mods['dask'].bag = mods['dask.bag']
  mods['dask.bag'].concat = lambda bags: Bag()
  mods['nltk'].tokenize = mods['nltk.tokenize']
  mods['nltk.tokenize'].sent_tokenize = lambda article: article.split('\x01')
  sys.modules.update(mods)
  sys.path.insert(0, os.environ['LDDL_REFERENCE'])
  import lddl.dask.bart.pretrain as ref

  def closure(target_seq_length):
    ref._get_sequences(target_seq_length=target_seq_length)
    return captured.pop('f')
  return closure


def sentence(rng, n, sep=' '):
  return sep.join(rng.choice(WORDS) for _ in range(n))


def articles():
  rng = random.Random(20261020)
  arts = []
  # hand-made edges
  arts.append('\x01'.join(['  leading and trailing  ', '', '   ', '\t\n', 'single', 'two words', ' 　 ', 'x']))
  arts.append('\x01'.join(w + ' after' for w in PY_SPACE))                 # a piece that begins with each space
  arts.append('\x01'.join('a' + w + 'b' + w + w + 'c' for w in PY_SPACE))  # each space inside, single and doubled
  arts.append(('one' + ' ' * 70 + 'two' + ' ' * 200 + 'three') + '\x01' + 'tail')     # long runs of spaces
  arts.append('\x01'.join(['w'] * 40))                                    # single-word sentences
  arts.append(sentence(rng, 700) + '\x01' + 'short one' + '\x01' + sentence(rng, 3))  # one sentence longer than any T
  arts.append('東京は日本の首都です。\x01大阪 京都　'
              '奈良\x01中文没有空格')                 # CJK, with U+3000 between words
  arts.append('')                                                         # nothing
  arts.append('\x01'.join(['', ' ', ' ']))                           # only empty / whitespace pieces
  arts.append('id12345 The id stays in the first sentence.\x01Second sentence here.')
  for n in (1, 2, 4, 5, 6, 124, 125, 126):                                # counts around T = 0, 1, 5, 125
    arts.append(sentence(rng, n))
    arts.append(sentence(rng, n) + '\x01' + sentence(rng, 1))
  while len(arts) < 240:
    pieces = []
    for _ in range(rng.randint(1, 14)):
      r = rng.random()
      if r < 0.06:
        pieces.append(rng.choice(['', ' ', '\t', rng.choice(PY_SPACE) * rng.randint(1, 3)]))
        continue
      s = sentence(rng, rng.choice([1, 1, 2, 3, 5, 8, 13, 21, 34]), sep=' ' if r < 0.8 else rng.choice(PY_SPACE))
      if r > 0.9:
        s = rng.choice(PY_SPACE) * rng.randint(1, 2) + s + rng.choice(PY_SPACE)
      pieces.append(s)
    arts.append('\x01'.join(pieces))
  return arts


def build():
  closure = load_reference()
  arts = articles()
  results = {}
  for t in TARGETS:
    f = closure(t)
    results[str(t)] = [[[r['sentences'], r['num_tokens'], r['target_length']] for r in f(a)] for a in arts]
  return {'generator': 'tools/gen_golden_bart.py', 'reference': 'lddl/dask/bart/pretrain.py:82-133',
          'sent_tokenize': "split on '\\x01'", 'row': ['sentences', 'num_tokens', 'target_length'],
          'articles': arts, 'results': results}


def main():
  doc = build()
  with gzip.GzipFile(OUT, 'wb', mtime=0) as f:
    f.write(json.dumps(doc, ensure_ascii=True, sort_keys=True).encode())
  print(OUT, os.path.getsize(OUT), 'bytes;', len(doc['articles']), 'articles;',
        {t: sum(len(r) for r in rs) for t, rs in doc['results'].items()}, 'chunks')


if __name__ == '__main__':
  if '--check' in sys.argv:  # the committed golden is what the reference gives now
    with gzip.open(OUT, 'rt') as f:
      assert json.load(f) == json.loads(json.dumps(build())), 'golden differs'
    print('golden reproduced')
  else:
    main()
