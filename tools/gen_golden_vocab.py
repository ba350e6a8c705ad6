#!/usr/bin/env python3
"""Golden vectors for the synthetic vocabularies of tests/synth_vocab.py (run
on the development machine only; needs HF tokenizers + transformers).

For every vocabulary: ``transformers.BertTokenizerFast(vocab_file)`` as
tools/gen_golden_tokenizer.py builds it, ``backend_tokenizer.encode_batch(...,
add_special_tokens=False)``, each result cut to 512.

Writes
  tests/golden/vocabs/<name>.txt        the small vocabularies
  tests/golden/tok_synth_common.npz     the sentences every corpus ends with
  tests/golden/tok_synth_<name>.npz     the vocabulary's targeted sentences
                                        (data, sent_off) and the ids / counts
                                        of targeted + common sentences
  tests/golden/vocab_lines_hf.json      what HF makes of CRLF lines, trailing
                                        blanks, duplicate lines and specials on
                                        two lines: its token -> id map and
                                        its special ids for those vocabularies
"""
import json
import os
import sys

import numpy as np
import tokenizers
import transformers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from lddl_amd import synth  # noqa: E402
import synth_vocab as sv  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
  os.makedirs(sv.VOCAB_DIR, exist_ok=True)
  for name in sv.SMALL:
    with open(os.path.join(sv.VOCAB_DIR, name + '.txt'), 'wb') as f:
      f.write(sv.vocab_bytes(name))
  common = sv.common_sentences()
  cc = synth.corpus_from_sentences(common, [0, len(common)])
  np.savez_compressed(os.path.join(GOLDEN, 'tok_synth_common.npz'), data=cc.data, sent_off=cc.sent_off)
  lines = {'tokenizers': tokenizers.__version__, 'transformers': transformers.__version__}
  for name in sv.NAMES:
    tok = transformers.BertTokenizerFast(sv.vocab_path(name))
    bt = tok.backend_tokenizer
    tgt = sv.targeted(name)
    enc = bt.encode_batch(tgt + common, add_special_tokens=False)
    ids = [e.ids[:512] for e in enc]
    c = synth.corpus_from_sentences(tgt, [0, len(tgt)])
    cnt = np.array([len(i) for i in ids], dtype=np.int32)
    flat = np.array([x for i in ids for x in i], dtype=np.int32)
    assert flat.max() < sv.vocab_size(name)
    out = os.path.join(GOLDEN, 'tok_synth_%s.npz' % name)
    np.savez_compressed(out, data=c.data, sent_off=c.sent_off, ids=flat.astype(np.uint16), ntok=cnt,
                        tokenizers=np.array(tokenizers.__version__))
    unk = tok.unk_token_id
    print(name, sv.vocab_size(name), 'entries', len(tgt), '+', len(common), 'sentences', flat.size, 'tokens',
          '%.1f %% [UNK]' % (100.0 * (flat == unk).mean()), 'max id', int(flat.max()), os.path.getsize(out), 'file bytes')
    if name in sv.LINE_VOCABS:
      lines[name] = bt.get_vocab()
      lines[name + ':special_ids'] = [tok.pad_token_id, tok.unk_token_id, tok.cls_token_id, tok.sep_token_id,
                                      tok.mask_token_id]
  with open(os.path.join(GOLDEN, 'vocab_lines_hf.json'), 'w') as f:
    json.dump(lines, f, indent=0, sort_keys=True, ensure_ascii=True)
    f.write('\n')


if __name__ == '__main__':
  main()
