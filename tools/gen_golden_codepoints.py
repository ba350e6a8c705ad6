#!/usr/bin/env python3
"""Golden digests of the code-point sweep (run where HF tokenizers is
installed; needs transformers and tokenizers, like gen_golden_tokenizer.py).

Every family of tests/codepoint_sweep.py goes through
``BertTokenizerFast(vocab).backend_tokenizer.encode_batch(...,
add_special_tokens=False)`` and ``[:512]``, the calling pattern of
tools/gen_golden_tokenizer.py.  Stored per vocabulary and family: the digest
and the token total of every block of 512 sentences and the corpus digest;
also the markpairs / len100 / markwords code-point selections (chosen with
this Python's unicodedata and the reference normalizer) and the tokenizers
version.  No ids.

Writes tests/golden/tok_codepoints.npz.
"""
import os
import sys
import time

import numpy as np
import transformers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import codepoint_sweep as cs  # noqa: E402

VOCABS = {
    'bert': os.path.join(ROOT, 'lddl_amd', 'data', 'bert_vocab.txt'),
    'codebert': os.path.join(ROOT, 'lddl_amd', 'data', 'codebert_52000_vocab.txt'),
}
CHUNK = 1 << 16  # sentences per encode_batch call


def main():
  import unicodedata
  norm = transformers.BertTokenizerFast(VOCABS['bert']).backend_tokenizer.normalizer
  sel = cs.select(norm.normalize_str)
  out = {'sel_marks': sel['marks'], 'sel_len100': sel['len100'], 'sel_kept': sel['kept'],
         'sel_kept_class': sel['kept_class'],
         'tokenizers': np.array(__import__('tokenizers').__version__),
         'unidata': np.array(unicodedata.unidata_version)}
  print('marks', len(sel['marks']), 'len100 code points', len(sel['len100']), 'kept marks', len(sel['kept']))
  for name, path in VOCABS.items():
    bt = transformers.BertTokenizerFast(path).backend_tokenizer
    for fam in cs.GOLDEN_FAMILIES[name]:
      t0 = time.time()
      sents = cs.sentences(fam, sel)
      data, sent_off = cs.corpus(fam, sel)
      assert len(sents) == len(sent_off) - 1 == cs.n_sentences(fam, sel)
      ntok = np.zeros(len(sents), np.int32)
      parts = []
      for i in range(0, len(sents), CHUNK):
        enc = bt.encode_batch(sents[i:i + CHUNK], add_special_tokens=False)
        ids = [e.ids[:512] for e in enc]
        ntok[i:i + CHUNK] = [len(x) for x in ids]
        parts.append(np.fromiter((x for s in ids for x in s), dtype=np.int32))
      dig, tot = cs.digest_blocks(np.concatenate(parts), ntok)
      out[cs.golden_key(name, fam, 'dig')] = dig
      out[cs.golden_key(name, fam, 'tot')] = tot.astype(np.int32)
      out[cs.golden_key(name, fam, 'corpus')] = np.array(cs.corpus_digest(data, sent_off), np.uint64)
      print('%-8s %-9s %8d sentences %9d bytes %9d tokens %5d blocks %.1f s' %
            (name, fam, len(sents), len(data), int(tot.sum()), len(dig), time.time() - t0))
  path = os.path.join(ROOT, 'tests', 'golden', cs.GOLDEN_FILE)
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), 'bytes; tok_bert.npz',
        os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'tok_bert.npz')))


if __name__ == '__main__':
  main()
