"""Host model of the BART sentence aggregation (lddl_bart_count / _plan_len /
_plan / _render), written for this project from the rule the reference states
(lddl/dask/bart/pretrain.py:88-128) and pinned to the reference's own output
by tests/test_bart_host.py.

Input: a sentence table (data bytes, sent_off [n_sent + 1], doc_sent_off
[n_doc + 1]) and T = target_seq_length - 3.  Unlike the reference's front end
it accepts sentences of 0 words (empty or whitespace only): they add
" " + bytes to the chunk text and nothing to the count; a remainder whose
count is 0 is dropped with its text.
"""
import numpy as np


def count_words(data, sent_off):
  """len(sentence.split()) per sentence, as int32"""
  raw = bytes(data)
  return np.array([len(raw[int(a):int(b)].decode('utf-8').split()) for a, b in zip(sent_off[:-1], sent_off[1:])],
                  dtype=np.int32).reshape(-1)


def plan(nwords, sent_off, doc_sent_off, T):
  """The chunk tables: dict of doc_chunk_off int64 [n_doc + 1], chunk_sent0
  int64, chunk_nsent / chunk_num_tokens int32, chunk_off int64 [n_chunks + 1]"""
  sent0, nsent, ntok, lens, dco = [], [], [], [], [0]
  for d in range(len(doc_sent_off) - 1):
    cnt, first = 0, int(doc_sent_off[d])
    for s in range(int(doc_sent_off[d]), int(doc_sent_off[d + 1])):
      cnt += int(nwords[s])
      if cnt >= T:
        sent0.append(first)
        nsent.append(s + 1 - first)
        ntok.append(cnt)
        cnt, first = 0, s + 1
    if cnt > 0:
      sent0.append(first)
      nsent.append(int(doc_sent_off[d + 1]) - first)
      ntok.append(cnt)
    dco.append(len(sent0))
  so = np.asarray(sent_off, dtype=np.int64)
  sent0 = np.array(sent0, dtype=np.int64).reshape(-1)
  nsent = np.array(nsent, dtype=np.int32).reshape(-1)
  lens = so[sent0 + nsent] - so[sent0] + nsent if len(sent0) else np.zeros(0, np.int64)
  off = np.zeros(len(sent0) + 1, dtype=np.int64)
  np.cumsum(lens, out=off[1:])
  return {'doc_chunk_off': np.array(dco, dtype=np.int64), 'chunk_sent0': sent0, 'chunk_nsent': nsent,
          'chunk_num_tokens': np.array(ntok, dtype=np.int32).reshape(-1), 'chunk_off': off}


def render(data, sent_off, pl, c0=0, n=None):
  """(offsets from 0, bytes) of chunks [c0, c0 + n): every sentence with one space in front"""
  raw = bytes(data)
  n = len(pl['chunk_sent0']) - c0 if n is None else n
  out = []
  for c in range(c0, c0 + n):
    s0, ns = int(pl['chunk_sent0'][c]), int(pl['chunk_nsent'][c])
    out.append(b''.join(b' ' + raw[int(sent_off[s]):int(sent_off[s + 1])] for s in range(s0, s0 + ns)))
  off = np.zeros(n + 1, dtype=np.int64)
  np.cumsum([len(b) for b in out], out=off[1:])
  return off, np.frombuffer(b''.join(out), dtype=np.uint8)


def aggregate(data, sent_off, doc_sent_off, T):
  """plan + every chunk's bytes: (tables, list of bytes per chunk)"""
  pl = plan(count_words(data, sent_off), sent_off, doc_sent_off, T)
  off, b = render(data, sent_off, pl)
  raw = b.tobytes()
  return pl, [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def table(docs):
  """documents (lists of sentence bytes / str) -> (data uint8, sent_off, doc_sent_off)"""
  sents = [s.encode('utf-8') if isinstance(s, str) else s for d in docs for s in d]
  so = np.zeros(len(sents) + 1, dtype=np.int64)
  np.cumsum([len(s) for s in sents], out=so[1:])
  dso = np.zeros(len(docs) + 1, dtype=np.int64)
  np.cumsum([len(d) for d in docs], out=dso[1:])
  return np.frombuffer(b''.join(sents), dtype=np.uint8), so, dso
