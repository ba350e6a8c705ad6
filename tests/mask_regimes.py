"""The regimes of the static-masking packer's create_masked_lm_predictions
block (lddl_amd/csrc/pack_wave.hip, pack_bert_wave_kernel<MASK = 1 | 2>), as
a corpus that reaches them and a host-side classification of the oracle's
rows.  Host only: nothing here touches a GPU.

Per pair the kernel chooses
  * implicit or explicit candidates (expl: a sentence of the pair holds a
    literal [CLS] / [SEP] id; the explicit list lives in global scratch),
  * the split trace (nm < m and nm8 + nm <= MCAP: the swaps q >= nm become
    successor chains F, built in 64-swap chunks) or the unsplit one (the
    trace covers [1, (m + 7) & ~7)),
  * ceil(nm / 64) pick passes,
and per launch the MASK = 1 (lists of 512 / 256) or MASK = 2 (1024 / 1024)
instantiation.  classify() restates those formulas over the oracle's rows.
"""
import functools
import random

from oracle import pack_oracle as po

CLS, SEP, MASK_ID, N_VOCAB = 101, 102, 103, 30522  # bert-base-uncased
DUP = 3
PACK_SEED = 7  # partition p packs after random.seed(PACK_SEED + p)
# corpus seeds under which the oracle alone reaches required(seq, ratio):
# every candidate count m = 2 .. 125 at seq 128 takes its own pair
CORPUS_SEED = 5
CORPUS_SEEDS = {(128, 0.15): 7}
N_PART = 4

# the constants of the kernel and its launch, each stated once
MLM_PICKS_1 = 256    # pack_wave.hip:63
MLM_MAX_SEQ = 1024   # pack.h:77
MLM_CHUNK = 1024     # pack.h:76
MCAP = {1: 512, 2: MLM_MAX_SEQ}  # pack_wave.hip:971

# (seq, ratio) of every configuration under test
CONFIGS = [(128, 0.15), (128, 0.0), (128, 1.0), (512, 0.5), (512, 1.0), (1024, 0.6), (1024, 1.0), (1024, 0.15)]


def corpus(seq, seed=CORPUS_SEED):
  """-> (docs, part_doc_off): pre-tokenised documents (lists of id lists).
  One two-sentence document for every total length 2 .. seq - 3 + 40, cut at
  random, and a dozen documents of [CLS] / [SEP] ids alone or beside one
  ordinary id (pairs of m == 0 and m == 1 candidates; as a random next they
  make long explicit pairs); shuffled, in N_PART partitions."""
  rnd = random.Random(seed)
  docs = []
  for total in range(2, seq - 3 + 40 + 1):
    cut = rnd.randint(1, total - 1)
    ids = [rnd.randint(999, 29999) for _ in range(total)]
    docs.append([ids[:cut], ids[cut:]])
  sp = lambda n: [rnd.choice((CLS, SEP)) for _ in range(n)]  # noqa: E731
  for k in range(12):
    a, b = sp(rnd.randint(1, 4)), sp(rnd.randint(1, 4))
    if k % 3 == 1:  # one ordinary id in the document
      a[rnd.randrange(len(a))] = rnd.randint(999, 29999)
    if k % 3 == 2:  # one ordinary id per sentence
      a[rnd.randrange(len(a))] = rnd.randint(999, 29999)
      b[rnd.randrange(len(b))] = rnd.randint(999, 29999)
    docs.append([a, b])
  rnd.shuffle(docs)
  n = len(docs)
  return docs, [n * p // N_PART for p in range(N_PART + 1)]


@functools.lru_cache(maxsize=None)
def oracle_rows(seq, ratio, seed=None):
  """-> (docs, part_doc_off, rows per partition): the oracle's rows
  (A', B', is_random_next, num_tokens, positions, labels, expl) of
  corpus(seq, seed) at duplicate factor DUP, bin size seq // 4, in the binned
  output order.  expl is what the kernel's any_spec sees: whether any
  sentence the pair draws from holds a [CLS] / [SEP] id (the truncation may
  have cut the id itself away).  Computed once per configuration and shared;
  not modified."""
  docs, pdo = corpus(seq, CORPUS_SEEDS.get((seq, ratio), CORPUS_SEED) if seed is None else seed)
  masking = (ratio, N_VOCAB, CLS, SEP, MASK_ID)
  out = []
  for p in range(N_PART):
    D = docs[pdo[p]:pdo[p + 1]]
    spec = [[CLS in s or SEP in s for s in d] for d in D]
    prs = po.partition_pairs(D, PACK_SEED + p, lambda X, di, r: po.bert_pairs(X, di, seq, 0.1, r, masking), DUP)
    rr = []
    for pr in prs:
      a, b, rn = po.pair_tokens(D, pr)
      ma, mb, pos, lab = pr[5]
      expl = any(spec[d][s] for (d, s) in pr[0] + pr[1])
      rr.append((ma, mb, rn, len(a) + len(b) + 3, pos, lab, expl))
    order, _ = po.binned_order([r[3] for r in rr], seq // 4, 4)
    out.append([rr[i] for i in order])
  return docs, pdo, out


def instantiation(seq, ratio):
  """the MASK template argument launch_pack_bert_wave picks (pack_wave.hip:1227)"""
  return 1 if seq <= 512 and max(1, int(round(seq * ratio))) <= MLM_PICKS_1 else 2


def pair_regime(row, seq, ratio):
  """one row -> dict of the masked block's per-pair quantities (pack_wave.hip:912-974)"""
  ma, mb, _, n, pos, lab, expl = row
  tok = [CLS] + list(ma) + [SEP] + list(mb) + [SEP]
  for q, l in zip(pos, lab):  # the tokens before masking
    tok[q] = l
  assert len(tok) == n
  m = sum(1 for t in tok if t != CLS and t != SEP)
  assert expl or m == n - 3
  ntp = max(1, int(round(n * ratio)))  # :913 (round() and rint() both round half to even)
  nm = min(ntp, m)  # :952
  assert nm == len(pos)
  nm8 = (nm + 7) & ~7  # :972
  split = nm < m and nm8 + nm <= MCAP[instantiation(seq, ratio)]  # :973
  tr8 = nm8 if split else (m + 7) & ~7  # :974
  chunks = ((m - nm - 1) >> 6) + 1 if split else 0  # :983, F-build passes
  return dict(n=n, m=m, expl=expl, ntp=ntp, nm=nm, nm8=nm8, split=split, tr8=tr8, chunks=chunks)


def classify(rows, seq, ratio):
  """rows: oracle_rows' partitions -> the set of regimes reached, as tuples
    ('zero',)                      m == 0
    ('full', expl, m)              nm == m >= 1 (unsplit, every candidate picked)
    ('split', expl, chunks)        split trace with that many F-build chunks
    ('split_nm', nm)  ('split_m', m)  ('split_nm_m', nm, m) for nm == 1
    ('unsplit', expl)              unsplit with nm < m
    ('unsplit_nm', nm)
    ('tr8', tr8)  ('nm', nm)  ('passes', ceil(nm / 64))"""
  out = set()
  for part in rows:
    for row in part:
      r = pair_regime(row, seq, ratio)
      out.add(('nm', r['nm']))
      out.add(('tr8', r['tr8']))
      out.add(('passes', (r['nm'] + 63) // 64))
      if r['m'] == 0:
        out.add(('zero',))
      elif r['nm'] == r['m']:
        out.add(('full', r['expl'], r['m']))
      elif r['split']:
        out.add(('split', r['expl'], r['chunks']))
        out.add(('split_nm', r['nm']))
        out.add(('split_m', r['m']))
        if r['nm'] == 1:
          out.add(('split_nm_m', 1, r['m']))
      else:
        out.add(('unsplit', r['expl']))
        out.add(('unsplit_nm', r['nm']))
  return out


def required(seq, ratio):
  """-> (instantiation, the regimes a run of (seq, ratio) must reach).  From
  the formulas alone: a pair has n = m + 3 tokens when implicit, m <= seq - 3."""
  mm = seq - 3
  both = lambda *t: {t[:1] + (e,) + t[1:] for e in (False, True)}  # noqa: E731
  if (seq, ratio) == (128, 0.15):
    return 1, (both('split', 1) | both('split', 2) | {('split_m', m) for m in range(2, mm + 1)} |
               {('zero',), ('full', True, 1)})
  if (seq, ratio) == (128, 0.0):  # ntp = max(1, 0): one pick whatever the length
    return 1, {('split_nm_m', 1, m) for m in range(2, mm + 1)} | {('zero',), ('full', True, 1)}
  if (seq, ratio) == (128, 1.0):  # every m, so every multiple of 8 and of 64 and its neighbours
    return 1, {('full', False, m) for m in range(2, mm + 1)} | {('full', True, 1), ('full', True, 2), ('zero',)}
  if (seq, ratio) == (512, 0.5):  # short rows: ntp = rint(n / 2) reaches m = n - 3 for n <= 7
    return 1, ({('split_nm', MLM_PICKS_1), ('passes', 4)} | {('split', False, c) for c in (1, 2, 3, 4)} |
               {('full', False, 2), ('full', False, 3), ('full', False, 4), ('zero',)})
  if (seq, ratio) == (512, 1.0):
    return 2, ({('full', False, mm), ('full', True, 1), ('zero',), ('passes', 8)} |
               {('tr8', t) for t in range(8, 513, 8)})
  if (seq, ratio) == (1024, 0.6):  # nm = 512: 512 + 512 <= 1024 splits; nm = 513: 520 + 513 does not
    return 2, (both('unsplit') | both('split', 1) | {('split_nm', 512), ('unsplit_nm', 513), ('unsplit_nm', 614)} |
               {('split', False, c) for c in range(1, 7)} | {('zero',)})
  if (seq, ratio) == (1024, 1.0):
    return 2, ({('full', False, mm), ('full', True, 1), ('zero',), ('passes', 16)} |
               {('tr8', t) for t in range(8, 1025, 8)})
  if (seq, ratio) == (1024, 0.15):  # m - nm up to 1021 - 154: (866 >> 6) + 1 = 14 chunks
    return 2, {('split', False, c) for c in range(1, 15)} | both('split', 1) | {('zero',)}
  raise KeyError((seq, ratio))


def default_arena(n_sent):
  """lddl_pack_bert's first masked-LM arena (capi_pack.hip:184)"""
  return N_PART * 4 * MLM_CHUNK + DUP * n_sent * 4
