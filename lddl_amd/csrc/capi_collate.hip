// C-ABI, host side of the training-time collate (kernels: collate.hip,
// collate_rows.hip, collate_unpadded.hip, collate_fixed.hip, rows_from_strings.hip, mlm_targets.hip).
#include "capi_ctx.h"

#include <math.h>

static int collate_vocab(lddl_ctx* c, CollateVocab* V) {
  if (!c->d_ctab) {
    const size_t n = c->vocab.size();
    uint32_t sz = 1024;
    while (sz < 4 * n) sz <<= 1;
    std::vector<uint2> tab(sz, make_uint2(0u, 0xFFFFFFFFu));
    for (size_t i = 0; i < n; ++i) {
      const std::string& w = c->vocab[i];
      const uint32_t h = collate_hash_host((const uint8_t*)w.data(), (int)w.size());
      for (uint32_t s = h & (sz - 1);; s = (s + 1) & (sz - 1)) {
        if (tab[s].y == 0xFFFFFFFFu) {
          tab[s] = make_uint2(h, (uint32_t)i);
          break;
        }
        if (tab[s].x == h && c->vocab[tab[s].y] == w) {  // duplicate line: last id wins
          tab[s].y = (uint32_t)i;
          break;
        }
      }
    }
    int rc;
    if ((rc = upload(&c->d_ctab, tab.data(), tab.size() * sizeof(uint2)))) return rc;
    c->ctab_mask = sz - 1;
  }
  V->slots = c->d_ctab;
  V->mask = c->ctab_mask;
  V->vinfo = c->d_rinfo;
  V->vpool = c->d_rpool;
  V->unk = (int32_t)c->special[1];
  V->cls = (int32_t)c->special[2];
  V->sep = (int32_t)c->special[3];
  V->mask_id = (int32_t)c->special[4];
  V->n_random = c->vocab_size;
  return 0;
}

// ---------------------------------------------------------------- span masking --
extern "C" int lddl_span_params(int32_t max_span, double geo_p, double mlm_probability, double* out_q,
                                double out_cdf[16]) {
  if (!out_q || !out_cdf) return set_err(LDDL_EINVAL, "null output pointer");
  if (max_span < 1 || max_span > 16) return set_err(LDDL_EINVAL, "max_span %d not in [1, 16]", max_span);
  if (!(geo_p > 0.0 && geo_p <= 1.0)) return set_err(LDDL_EINVAL, "geo_p not in (0, 1]");
  if (!(mlm_probability >= 0.0 && mlm_probability <= 1.0)) return set_err(LDDL_EINVAL, "mlm_probability not in [0, 1]");
  const int L = max_span;
  const double p = mlm_probability;
  // 1 - (1 - g)^t = -expm1(t * log1p(-g)): no cancellation for a small g, and 1 for g = 1
  const double lg = log1p(-geo_p), all = -expm1(L * lg);
  for (int t = 1; t <= 16; ++t) out_cdf[t - 1] = t < L ? std::min(-expm1(t * lg) / all, 1.0) : 1.0;
  if (L == 1) {
    *out_q = p;
    return 0;
  }
  // 1 - prod (1 - q * S_t), S_0 = 1, S_t = 1 - cdf[t], is 0 at 0, >= p at p and monotone.  Compared as the product
  // against 1 - p, which stays exact near p = 1.  64 halvings of [0, p] keep missed(lo) > 1 - p >= missed(hi);
  // q = hi, which is exactly 0 for p = 0 and exactly 1 for p = 1.
  const auto missed = [&](double q) {
    double keep = 1.0 - q;
    for (int t = 1; t < L; ++t) keep *= 1.0 - q * (1.0 - out_cdf[t - 1]);
    return keep;
  };
  double lo = 0.0, hi = p;
  for (int it = 0; it < 64; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (missed(mid) > 1.0 - p) lo = mid;
    else hi = mid;
  }
  *out_q = hi;
  return 0;
}

// the span law of a dynamic call over c, from its own mlm_probability; L = 0 while the switch is off
static int span_law(const lddl_ctx* c, double mlm_probability, SpanLaw* S) {
  *S = SpanLaw{};
  if (!c->span_max) return 0;
  S->L = c->span_max;
  return lddl_span_params(c->span_max, c->span_geo, mlm_probability, &S->q, S->cdf);
}

// the longest row m rounded up to a multiple of sequence_length_alignment (bert.py:94-97)
static int64_t aligned_seq_len(int64_t m, int32_t seq_align) { return ((m - 1) / seq_align + 1) * seq_align; }

extern "C" int lddl_collate_seq_len(lddl_ctx* c, const uint8_t* d_a, const int64_t* d_a_off, const uint8_t* d_b,
                                    const int64_t* d_b_off, int64_t n_rows, int32_t seq_align, int64_t* out_seq_len,
                                    void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0 || seq_align < 1 || !out_seq_len) return set_err(LDDL_EINVAL, "bad n_rows / seq_align / out");
  if (n_rows > 0 && (!d_a || !d_a_off || !d_b || !d_b_off)) return set_err(LDDL_EINVAL, "null column pointer");
  if (n_rows == 0) return set_err(LDDL_EINVAL, "empty batch (max() of an empty sequence)");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CollateParams P{};
  int rc;
  if ((rc = collate_vocab(c, &P.V))) return rc;
  P.C = StringColumns{d_a, d_a_off, d_b, d_b_off, nullptr, nullptr, nullptr, nullptr};
  P.n_rows = n_rows;
  if ((rc = ws_get(c, CW_SHARED_META, 1, &P.max_len))) return rc;
  HIP_TRY(hipMemsetAsync(P.max_len, 0, 4, st));
  HIP_TRY(launch_collate_len(P, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_MAX_LEN, P.max_len, 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  *out_seq_len = aligned_seq_len(*(const int32_t*)&c->h_tot[HW_MAX_LEN], seq_align);
  return 0;
}

extern "C" int lddl_collate_bert(lddl_ctx* c, const uint8_t* d_a, const int64_t* d_a_off, const uint8_t* d_b,
                                 const int64_t* d_b_off, const uint8_t* d_is_random_next, const uint8_t* d_pos,
                                 const int64_t* d_pos_off, const uint8_t* d_lab, const int64_t* d_lab_off,
                                 int64_t n_rows, int64_t seq_len, int32_t mode, int64_t ignore_index,
                                 double mlm_probability, uint64_t seed, uint64_t counter, int64_t* d_input_ids,
                                 int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
                                 int64_t* d_next_sentence_labels, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0) return set_err(LDDL_EINVAL, "negative n_rows");
  if (mode < COLLATE_SPECIAL_MASK || mode > COLLATE_DYNAMIC) return set_err(LDDL_EINVAL, "mode %d not in 0..2", mode);
  if (seq_len < 3 || seq_len > COLLATE_MAX_LEN)
    return set_err(LDDL_ECAPACITY, "seq_len %lld not in [3, %d]", (long long)seq_len, COLLATE_MAX_LEN);
  if (ignore_index < INT32_MIN || ignore_index > INT32_MAX) return set_err(LDDL_EINVAL, "ignore_index out of int32");
  if (!(mlm_probability >= 0.0 && mlm_probability <= 1.0)) return set_err(LDDL_EINVAL, "mlm_probability not in [0, 1]");
  if (n_rows > 0 && (!d_a || !d_a_off || !d_b || !d_b_off || !d_is_random_next || !d_input_ids ||
                     !d_token_type_ids || !d_attention_mask || !d_labels || !d_next_sentence_labels))
    return set_err(LDDL_EINVAL, "null pointer");
  if (mode == COLLATE_STATIC && n_rows > 0 && (!d_pos || !d_pos_off || !d_lab || !d_lab_off))
    return set_err(LDDL_EINVAL, "static masking needs positions and labels");
  if (n_rows == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CollateParams P{};
  int rc;
  if ((rc = collate_vocab(c, &P.V))) return rc;
  P.C = StringColumns{d_a, d_a_off, d_b, d_b_off, d_pos, d_pos_off, d_lab, d_lab_off};
  P.is_random_next = d_is_random_next;
  P.n_rows = n_rows;
  P.seq_len = (int32_t)seq_len;
  P.mode = mode;
  P.ignore_index = ignore_index;
  P.mlm_probability = mlm_probability;
  P.seed = seed;
  P.counter = counter;
  P.cont = c->whole_word || c->span_max ? c->d_cont : nullptr;  // picks the whole-word or the span instantiation of mode 2
  if (mode == COLLATE_DYNAMIC && (rc = span_law(c, mlm_probability, &P.span))) return rc;
  P.input_ids = d_input_ids;
  P.token_type_ids = d_token_type_ids;
  P.attention_mask = d_attention_mask;
  P.labels = d_labels;
  P.next_sentence_labels = d_next_sentence_labels;
  uint32_t e;
  if ((rc = ws_get(c, CW_COLLATE_ERR, 1, &P.err))) return rc;
  HIP_TRY(hipMemsetAsync(P.err, 0, 4, st));
  HIP_TRY(launch_collate_fill(P, c->n_cu, st));
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) {
    const unsigned long long row = e >> 4;
    switch (e & 15u) {
      case CERR_LONG: return set_err(LDDL_ECAPACITY, "row %llu longer than seq_len %lld", row, (long long)seq_len);
      case CERR_POS_RANGE:
        return set_err(LDDL_EINDEX, "row %llu: masked_lm_positions index out of range for seq_len %lld", row,
                       (long long)seq_len);
      case CERR_NPY: return set_err(LDDL_EFORMAT, "row %llu: masked_lm_positions is not np.save bytes", row);
      default:
        return set_err(LDDL_EFORMAT, "row %llu: masked_lm_positions and masked_lm_labels differ in length", row);
    }
  }
  return 0;
}

extern "C" int lddl_mask_tokens(lddl_ctx* c, int64_t* d_inputs, const int64_t* d_special_tokens_mask,
                                int64_t* d_labels, int64_t n_rows, int64_t seq_len, double mlm_probability,
                                int64_t ignore_index, uint64_t seed, uint64_t counter, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0 || seq_len < 0 || seq_len >= (1 << 20)) return set_err(LDDL_EINVAL, "bad shape");
  if (!(mlm_probability >= 0.0 && mlm_probability <= 1.0)) return set_err(LDDL_EINVAL, "mlm_probability not in [0, 1]");
  if (n_rows * seq_len > 0 && (!d_inputs || !d_special_tokens_mask || !d_labels))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  MaskParams M{};
  M.inputs = d_inputs;
  M.special = d_special_tokens_mask;
  M.labels = d_labels;
  M.n_rows = n_rows;
  M.seq_len = (int32_t)seq_len;
  M.mask_id = (int32_t)c->special[4];
  M.n_random = c->vocab_size;
  M.ignore_index = ignore_index;
  M.mlm_probability = mlm_probability;
  M.seed = seed;
  M.counter = counter;
  M.cont = c->whole_word || c->span_max ? c->d_cont : nullptr;  // picks the wave-per-row kernel
  int rc;
  if ((rc = span_law(c, mlm_probability, &M.span))) return rc;
  HIP_TRY(launch_mask_tokens(M, c->n_cu, (hipStream_t)stream));
  return 0;
}

// ---------------------------------------------- collate from a pack result --
static int collate_rows_error(uint32_t e, int64_t seq_len) {
  const unsigned long long row = e >> 4;
  switch (e & 15u) {
    case CERR_ROW_INDEX: return set_err(LDDL_EINDEX, "batch row %llu: row index out of range", row);
    case CERR_LONG: return set_err(LDDL_ECAPACITY, "batch row %llu longer than seq_len %lld", row, (long long)seq_len);
    case CERR_POS_RANGE:
      return set_err(LDDL_EINDEX, "batch row %llu: masked position out of range for seq_len %lld", row,
                     (long long)seq_len);
    case CERR_CU_SEQLENS:
      return set_err(LDDL_EINVAL, "batch row %llu: cu_seqlens do not hold the row's tokens within [0, total)", row);
    case CERR_CODE_ROW:
      return set_err(LDDL_EINVAL, "batch row %llu has doc tokens and no [SEP] after them (flags bit 1 clear, len0 > 0)", row);
    default:
      return set_err(LDDL_EINVAL,
                     "batch row %llu has no [SEP] after its first segment (a CodeBERT row: lddl_collate_code_rows takes it)",
                     row);
  }
}

// collate_rows_error with the unpadded calls' wording where seq_len has no meaning (max_len: the bound of a row, the
// fixed calls' max_seqlen)
static int collate_unpadded_error(uint32_t e, int64_t max_len = COLLATE_MAX_LEN) {
  const unsigned long long row = e >> 4;
  switch (e & 15u) {
    case CERR_LONG: return set_err(LDDL_ECAPACITY, "batch row %llu longer than %lld tokens", row, (long long)max_len);
    case CERR_POS_RANGE: return set_err(LDDL_EINDEX, "batch row %llu: masked position beyond the row's tokens", row);
    default: return collate_rows_error(e, 0);
  }
}

// the row selection that every lddl_collate_rows* / lddl_collate_code_rows* call takes (d_flags: the CodeBERT
// calls, whose row lengths depend on it, and the fill calls)
static void collate_rows_index(CollateRowsParams* P, const uint16_t* d_len0, const uint16_t* d_len1,
                               const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                               int64_t n_total) {
  P->len0 = d_len0;
  P->len1 = d_len1;
  P->flags = d_flags;
  P->rows = d_rows;
  P->row0 = row0;
  P->n_rows = n_rows;
  P->n_total = n_total;
}

// lddl_collate_rows_seq_len (code 0: d_flags NULL) and lddl_collate_code_rows_seq_len (code 1)
static int collate_rows_seq_len_common(lddl_ctx* c, int code, const uint16_t* d_len0, const uint16_t* d_len1,
                                       const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                                       int64_t n_total, int32_t seq_align, int64_t* out_seq_len, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0 || n_total < 0 || seq_align < 1 || !out_seq_len)
    return set_err(LDDL_EINVAL, "bad n_rows / n_total / seq_align / out");
  if (n_rows == 0) return set_err(LDDL_EINVAL, "empty batch (max() of an empty sequence)");
  if (!d_len0 || !d_len1 || (code && !d_flags)) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CollateRowsParams P{};
  collate_rows_index(&P, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total);
  int rc;
  uint32_t e;
  if ((rc = ws_get(c, CW_SHARED_META, 1, &P.max_len)) || (rc = ws_get(c, CW_COLLATE_ERR, 1, &P.err))) return rc;
  HIP_TRY(hipMemsetAsync(P.max_len, 0, 4, st));
  HIP_TRY(hipMemsetAsync(P.err, 0, 4, st));
  HIP_TRY(launch_collate_rows_len(P, code != 0, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_MAX_LEN, P.max_len, 4, st));
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return collate_rows_error(e, 0);
  *out_seq_len = aligned_seq_len(*(const int32_t*)&c->h_tot[HW_MAX_LEN], seq_align);
  return 0;
}

extern "C" int lddl_collate_rows_seq_len(lddl_ctx* c, const uint16_t* d_len0, const uint16_t* d_len1,
                                         const int64_t* d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                         int32_t seq_align, int64_t* out_seq_len, void* stream) {
  return collate_rows_seq_len_common(c, 0, d_len0, d_len1, nullptr, d_rows, row0, n_rows, n_total, seq_align, out_seq_len,
                                     stream);
}

// what lddl_collate[_code]_rows_fixed take beyond the unpadded fill call's arguments
struct CollateFixedArgs {
  int64_t tok_cap, seq_cap, max_seqlen;
  int32_t* d_status;
  int64_t *out_total, *out_n_rows, *out_n_seqs;
};

// the pad sequences that the slack of a fixed batch is cut into
static int64_t fixed_pad_seqs(int64_t total, const CollateFixedArgs& F) {
  return total < F.tok_cap ? (F.tok_cap - total + F.max_seqlen - 1) / F.max_seqlen : 0;
}

// collate_unpadded_error with the two refusals of the fixed calls
static int collate_fixed_error(uint32_t e, int64_t total, int64_t n_rows, const CollateFixedArgs& F) {
  switch (e & 15u) {
    case CERR_TOK_CAP:
      return set_err(LDDL_ECAPACITY, "the batch holds %lld tokens, tok_cap %lld", (long long)total, (long long)F.tok_cap);
    case CERR_SEQ_CAP:
      return set_err(LDDL_ECAPACITY, "%lld rows and %lld pad sequences of max_seqlen %lld, seq_cap %lld", (long long)n_rows,
                     (long long)fixed_pad_seqs(total, F), (long long)F.max_seqlen, (long long)F.seq_cap);
    default: return collate_unpadded_error(e, F.max_seqlen);
  }
}

// lddl_collate_rows (unpadded 0: seq_len, d_attention_mask) and lddl_collate_rows_unpadded (1: d_cu_seqlens,
// total, d_position_ids) validate their arguments and fill CollateRowsParams here, once.  The range check
// between the mode and the probability checks, the launch and the wording of the device's errors are each
// call's own; the arguments of the other call arrive as 0 / NULL and are passed on as that.  code 1: the
// lddl_collate_code_rows[_unpadded] twins, CodeBERT rows: modes 0 and 2, no static arrays, no
// d_next_sentence_labels, a row of two tokens at least, and an empty batch is refused.  F: the
// lddl_collate[_code]_rows_fixed calls, unpadded 1 with total = tok_cap and seq_len = max_seqlen, both range
// checks, d_cu_seqlens an output, the capacities' own checks and one launch that also makes the offsets.
static int collate_rows_common(lddl_ctx* c, int unpadded, int code, const uint16_t* d_ids, const int64_t* d_src0,
                               const int64_t* d_src1, const uint16_t* d_len0, const uint16_t* d_len1,
                               const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                               int64_t n_total, const int64_t* d_mlm_off, const uint16_t* d_mlm_pos,
                               const uint16_t* d_mlm_label, const uint16_t* d_mlm_token, int64_t seq_len,
                               const int32_t* d_cu_seqlens, int64_t total, int32_t mode, int64_t ignore_index,
                               double mlm_probability, uint64_t seed, uint64_t counter, int64_t* d_input_ids,
                               int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_position_ids,
                               int64_t* d_labels, int64_t* d_next_sentence_labels, void* stream,
                               const CollateFixedArgs* F = nullptr) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0 || n_total < 0) return set_err(LDDL_EINVAL, "negative n_rows / n_total");
  if ((code || F) && n_rows == 0) return set_err(LDDL_EINVAL, "empty batch");
  if (code && mode != COLLATE_SPECIAL_MASK && mode != COLLATE_DYNAMIC)
    return set_err(LDDL_EINVAL, "mode %d: CodeBERT rows have no static masks, the modes are 0 and 2", mode);
  if (mode < COLLATE_SPECIAL_MASK || mode > COLLATE_DYNAMIC) return set_err(LDDL_EINVAL, "mode %d not in 0..2", mode);
  const int min_len = code ? 2 : 3;
  if ((!unpadded || F) && (seq_len < min_len || seq_len > COLLATE_MAX_LEN))
    return set_err(LDDL_ECAPACITY, "%s %lld not in [%d, %d]", F ? "max_seqlen" : "seq_len", (long long)seq_len, min_len,
                   COLLATE_MAX_LEN);
  if (unpadded && total < 0) return set_err(LDDL_EINVAL, "negative %s", F ? "tok_cap" : "total");
  if (unpadded && total > INT32_MAX)
    return set_err(LDDL_ECAPACITY, "%s %lld: cu_seqlens are int32", F ? "tok_cap" : "total", (long long)total);
  if (F) {
    if (!F->d_status || !F->out_total || !F->out_n_rows || !F->out_n_seqs) return set_err(LDDL_EINVAL, "null pointer");
    if (F->seq_cap < 1 || F->seq_cap > (1 << 20))
      return set_err(LDDL_ECAPACITY, "seq_cap %lld not in [1, 2^20]", (long long)F->seq_cap);
    if (n_rows > F->seq_cap)
      return set_err(LDDL_ECAPACITY, "%lld rows, seq_cap %lld", (long long)n_rows, (long long)F->seq_cap);
  }
  if (!(mlm_probability >= 0.0 && mlm_probability <= 1.0)) return set_err(LDDL_EINVAL, "mlm_probability not in [0, 1]");
  if (n_rows > 0 && (!d_ids || !d_src0 || !d_src1 || !d_len0 || !d_len1 || !d_flags || !d_input_ids || !d_token_type_ids ||
                     (unpadded ? !d_cu_seqlens || !d_position_ids : !d_attention_mask) || !d_labels ||
                     (!code && !d_next_sentence_labels)))
    return set_err(LDDL_EINVAL, "null pointer");
  if (mode == COLLATE_STATIC && n_rows > 0 && (!d_mlm_off || !d_mlm_pos || !d_mlm_label || !d_mlm_token))
    return set_err(LDDL_EINVAL, "static masking needs lddl_masked_lm_spans' arrays");
  if (n_rows == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CollateUnpaddedParams U{};
  CollateRowsParams& P = U.R;
  int rc;
  collate_rows_index(&P, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total);
  P.ids = d_ids;
  P.src0 = d_src0;
  P.src1 = d_src1;
  P.mlm_off = d_mlm_off;
  P.mlm_pos = d_mlm_pos;
  P.mlm_label = d_mlm_label;
  P.mlm_token = d_mlm_token;
  P.cls = (int32_t)c->special[2];
  P.sep = (int32_t)c->special[3];
  P.mask_id = (int32_t)c->special[4];
  P.n_random = c->vocab_size;
  P.seq_len = (int32_t)seq_len;
  P.ignore_index = ignore_index;
  P.mlm_probability = mlm_probability;
  P.seed = seed;
  P.counter = counter;
  P.cont = c->whole_word || c->span_max ? c->d_cont : nullptr;  // picks the whole-word or the span instantiation of mode 2
  if (mode == COLLATE_DYNAMIC && (rc = span_law(c, mlm_probability, &P.span))) return rc;
  P.input_ids = d_input_ids;
  P.token_type_ids = d_token_type_ids;
  P.attention_mask = d_attention_mask;
  P.labels = d_labels;
  P.next_sentence_labels = d_next_sentence_labels;
  U.cu_seqlens = const_cast<int32_t*>(d_cu_seqlens);  // read only by the fill pass
  U.position_ids = d_position_ids;
  U.total = total;
  uint32_t e;
  if (F) {
    // one buffer, one memset, one copy: total, then the rows' error word and the capacities' (the layout of
    // HW_CU_TOTAL, HW_MAX_LEN); a row's error is reported first
    CollateFixedParams X{};
    int64_t* meta;
    if ((rc = ws_get(c, CW_SHARED_META, 2, &meta))) return rc;
    P.err = (uint32_t*)(meta + 1);
    X.R = P;
    X.cu_seqlens = U.cu_seqlens;
    X.position_ids = d_position_ids;
    X.tok_cap = F->tok_cap;
    X.seq_cap = F->seq_cap;
    X.status = F->d_status;
    X.total_out = meta;
    HIP_TRY(hipMemsetAsync(meta, 0, 16, st));
    HIP_TRY(launch_collate_fixed(X, code != 0, mode, c->n_cu, st));
    HIP_TRY(fetch_word(c, HW_CU_TOTAL, meta, 16, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t batch = c->h_tot[HW_CU_TOTAL];
    e = (uint32_t)(c->h_tot[HW_MAX_LEN] & 0xFFFFFFFF);
    if (!e) e = (uint32_t)((uint64_t)c->h_tot[HW_MAX_LEN] >> 32);
    *F->out_total = batch;
    *F->out_n_rows = n_rows;
    *F->out_n_seqs = n_rows + fixed_pad_seqs(batch, *F);
    return e ? collate_fixed_error(e, batch, n_rows, *F) : 0;
  }
  if ((rc = ws_get(c, CW_COLLATE_ERR, 1, &P.err))) return rc;
  HIP_TRY(hipMemsetAsync(P.err, 0, 4, st));
  HIP_TRY(unpadded ? launch_collate_unpadded(U, code != 0, mode, c->n_cu, st)
                   : launch_collate_rows(P, code != 0, mode, c->n_cu, st));
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return unpadded ? collate_unpadded_error(e) : collate_rows_error(e, seq_len);
  return 0;
}

extern "C" int lddl_collate_rows(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0, const int64_t* d_src1,
                                 const uint16_t* d_len0, const uint16_t* d_len1, const uint8_t* d_flags,
                                 const int64_t* d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                 const int64_t* d_mlm_off, const uint16_t* d_mlm_pos, const uint16_t* d_mlm_label,
                                 const uint16_t* d_mlm_token, int64_t seq_len, int32_t mode, int64_t ignore_index,
                                 double mlm_probability, uint64_t seed, uint64_t counter, int64_t* d_input_ids,
                                 int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
                                 int64_t* d_next_sentence_labels, void* stream) {
  return collate_rows_common(c, 0, 0, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, d_mlm_off,
                             d_mlm_pos, d_mlm_label, d_mlm_token, seq_len, nullptr, 0, mode, ignore_index, mlm_probability,
                             seed, counter, d_input_ids, d_token_type_ids, d_attention_mask, nullptr, d_labels,
                             d_next_sentence_labels, stream);
}

// ------------------------------------- padding-free collate from a pack result --
// lddl_collate_rows_cu_seqlens (code 0: d_flags NULL) and lddl_collate_code_rows_cu_seqlens (code 1)
static int collate_cu_seqlens_common(lddl_ctx* c, int code, const uint16_t* d_len0, const uint16_t* d_len1,
                                     const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                                     int64_t n_total, int32_t* d_cu_seqlens, int64_t* out_total, int64_t* out_max_seqlen,
                                     void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows < 0 || n_total < 0 || !out_total || !out_max_seqlen)
    return set_err(LDDL_EINVAL, "bad n_rows / n_total / out");
  if (n_rows == 0) return set_err(LDDL_EINVAL, "empty batch (max() of an empty sequence)");
  if (!d_len0 || !d_len1 || !d_cu_seqlens || (code && !d_flags)) return set_err(LDDL_EINVAL, "null pointer");
  // every row has its special tokens at least: three, or the two of a CodeBERT row without docstring
  if (n_rows > INT32_MAX / (code ? 2 : 3))
    return set_err(LDDL_ECAPACITY, "%lld rows hold 2^31 tokens or more", (long long)n_rows);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  CollateUnpaddedParams P{};
  collate_rows_index(&P.R, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total);
  P.cu_seqlens = d_cu_seqlens;
  P.n_chunks = collate_chunks(n_rows);
  int rc;
  uint32_t e;
  int64_t* meta;  // total, then max_len in the low half of meta[1]: the layout of HW_CU_TOTAL, HW_MAX_LEN
  if ((rc = ws_get(c, CW_SHARED_META, 2, &meta)) || (rc = ws_get(c, CW_SHARED_BSUM, (size_t)P.n_chunks, &P.chunk_sum)) ||
      (rc = ws_get(c, CW_COLLATE_ERR, 1, &P.R.err)))
    return rc;
  P.total_out = meta;
  P.R.max_len = (int32_t*)(meta + 1);
  HIP_TRY(hipMemsetAsync(meta, 0, 16, st));
  HIP_TRY(hipMemsetAsync(P.R.err, 0, 4, st));
  HIP_TRY(launch_collate_cu_seqlens(P, code != 0, st));
  HIP_TRY(fetch_word(c, HW_CU_TOTAL, meta, 16, st));
  if ((rc = read_err(c, P.R.err, st, &e))) return rc;
  if (e) return collate_unpadded_error(e);
  const int64_t total = c->h_tot[HW_CU_TOTAL];
  if (total > INT32_MAX)
    return set_err(LDDL_ECAPACITY, "the batch holds %lld tokens: cu_seqlens are int32", (long long)total);
  *out_total = total;
  *out_max_seqlen = *(const int32_t*)&c->h_tot[HW_MAX_LEN];
  return 0;
}

extern "C" int lddl_collate_rows_cu_seqlens(lddl_ctx* c, const uint16_t* d_len0, const uint16_t* d_len1,
                                            const int64_t* d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                            int32_t* d_cu_seqlens, int64_t* out_total, int64_t* out_max_seqlen,
                                            void* stream) {
  return collate_cu_seqlens_common(c, 0, d_len0, d_len1, nullptr, d_rows, row0, n_rows, n_total, d_cu_seqlens, out_total,
                                   out_max_seqlen, stream);
}

extern "C" int lddl_collate_rows_unpadded(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0,
                                          const int64_t* d_src1, const uint16_t* d_len0, const uint16_t* d_len1,
                                          const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                                          int64_t n_total, const int64_t* d_mlm_off, const uint16_t* d_mlm_pos,
                                          const uint16_t* d_mlm_label, const uint16_t* d_mlm_token,
                                          const int32_t* d_cu_seqlens, int64_t total, int32_t mode,
                                          int64_t ignore_index, double mlm_probability, uint64_t seed, uint64_t counter,
                                          int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_position_ids,
                                          int64_t* d_labels, int64_t* d_next_sentence_labels, void* stream) {
  return collate_rows_common(c, 1, 0, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, d_mlm_off,
                             d_mlm_pos, d_mlm_label, d_mlm_token, 0, d_cu_seqlens, total, mode, ignore_index,
                             mlm_probability, seed, counter, d_input_ids, d_token_type_ids, nullptr, d_position_ids,
                             d_labels, d_next_sentence_labels, stream);
}

// ------------------------------- fixed-shape padding-free collate from a pack result --
extern "C" int lddl_collate_rows_fixed(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0, const int64_t* d_src1,
                                       const uint16_t* d_len0, const uint16_t* d_len1, const uint8_t* d_flags,
                                       const int64_t* d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                       const int64_t* d_mlm_off, const uint16_t* d_mlm_pos, const uint16_t* d_mlm_label,
                                       const uint16_t* d_mlm_token, int32_t* d_cu_seqlens, int64_t tok_cap,
                                       int64_t seq_cap, int64_t max_seqlen, int32_t mode, int64_t ignore_index,
                                       double mlm_probability, uint64_t seed, uint64_t counter, int64_t* d_input_ids,
                                       int64_t* d_token_type_ids, int64_t* d_position_ids, int64_t* d_labels,
                                       int64_t* d_next_sentence_labels, int32_t* d_status, int64_t* out_total,
                                       int64_t* out_n_rows, int64_t* out_n_seqs, void* stream) {
  const CollateFixedArgs F{tok_cap, seq_cap, max_seqlen, d_status, out_total, out_n_rows, out_n_seqs};
  return collate_rows_common(c, 1, 0, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, d_mlm_off,
                             d_mlm_pos, d_mlm_label, d_mlm_token, max_seqlen, d_cu_seqlens, tok_cap, mode, ignore_index,
                             mlm_probability, seed, counter, d_input_ids, d_token_type_ids, nullptr, d_position_ids,
                             d_labels, d_next_sentence_labels, stream, &F);
}

// ------------------------------------------------- the same for CodeBERT rows --
extern "C" int lddl_collate_code_rows_seq_len(lddl_ctx* c, const uint16_t* d_len0, const uint16_t* d_len1,
                                              const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                                              int64_t n_total, int32_t seq_align, int64_t* out_seq_len, void* stream) {
  return collate_rows_seq_len_common(c, 1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, seq_align, out_seq_len,
                                     stream);
}

extern "C" int lddl_collate_code_rows(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0, const int64_t* d_src1,
                                      const uint16_t* d_len0, const uint16_t* d_len1, const uint8_t* d_flags,
                                      const int64_t* d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                      int64_t seq_len, int32_t mode, int64_t ignore_index, double mlm_probability,
                                      uint64_t seed, uint64_t counter, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                      int64_t* d_attention_mask, int64_t* d_labels, void* stream) {
  return collate_rows_common(c, 0, 1, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, nullptr,
                             nullptr, nullptr, nullptr, seq_len, nullptr, 0, mode, ignore_index, mlm_probability, seed,
                             counter, d_input_ids, d_token_type_ids, d_attention_mask, nullptr, d_labels, nullptr, stream);
}

extern "C" int lddl_collate_code_rows_cu_seqlens(lddl_ctx* c, const uint16_t* d_len0, const uint16_t* d_len1,
                                                 const uint8_t* d_flags, const int64_t* d_rows, int64_t row0,
                                                 int64_t n_rows, int64_t n_total, int32_t* d_cu_seqlens,
                                                 int64_t* out_total, int64_t* out_max_seqlen, void* stream) {
  return collate_cu_seqlens_common(c, 1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, d_cu_seqlens, out_total,
                                   out_max_seqlen, stream);
}

extern "C" int lddl_collate_code_rows_unpadded(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0,
                                               const int64_t* d_src1, const uint16_t* d_len0, const uint16_t* d_len1,
                                               const uint8_t* d_flags, const int64_t* d_rows, int64_t row0,
                                               int64_t n_rows, int64_t n_total, const int32_t* d_cu_seqlens,
                                               int64_t total, int32_t mode, int64_t ignore_index, double mlm_probability,
                                               uint64_t seed, uint64_t counter, int64_t* d_input_ids,
                                               int64_t* d_token_type_ids, int64_t* d_position_ids, int64_t* d_labels,
                                               void* stream) {
  return collate_rows_common(c, 1, 1, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, nullptr,
                             nullptr, nullptr, nullptr, 0, d_cu_seqlens, total, mode, ignore_index, mlm_probability, seed,
                             counter, d_input_ids, d_token_type_ids, nullptr, d_position_ids, d_labels, nullptr, stream);
}

extern "C" int lddl_collate_code_rows_fixed(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src0,
                                            const int64_t* d_src1, const uint16_t* d_len0, const uint16_t* d_len1,
                                            const uint8_t* d_flags, const int64_t* d_rows, int64_t row0, int64_t n_rows,
                                            int64_t n_total, int32_t* d_cu_seqlens, int64_t tok_cap, int64_t seq_cap,
                                            int64_t max_seqlen, int32_t mode, int64_t ignore_index, double mlm_probability,
                                            uint64_t seed, uint64_t counter, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                            int64_t* d_position_ids, int64_t* d_labels, int32_t* d_status, int64_t* out_total,
                                            int64_t* out_n_rows, int64_t* out_n_seqs, void* stream) {
  const CollateFixedArgs F{tok_cap, seq_cap, max_seqlen, d_status, out_total, out_n_rows, out_n_seqs};
  return collate_rows_common(c, 1, 1, d_ids, d_src0, d_src1, d_len0, d_len1, d_flags, d_rows, row0, n_rows, n_total, nullptr,
                             nullptr, nullptr, nullptr, max_seqlen, d_cu_seqlens, tok_cap, mode, ignore_index, mlm_probability,
                             seed, counter, d_input_ids, d_token_type_ids, nullptr, d_position_ids, d_labels, nullptr, stream,
                             &F);
}

// ------------------------------------------------------ compact MLM targets --
extern "C" int lddl_mlm_targets(lddl_ctx* c, const int64_t* d_labels, int64_t n_rows, int64_t seq_len,
                                const int32_t* d_cu_seqlens, int64_t total, int64_t ignore_index, int64_t capacity,
                                int64_t* d_positions, int64_t* d_target_labels, int32_t* d_offsets, int64_t* out_count,
                                void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (!d_positions || !d_target_labels || !d_offsets || !out_count) return set_err(LDDL_EINVAL, "null output pointer");
  if (n_rows <= 0) return set_err(LDDL_EINVAL, "n_rows %lld: a batch has one row at least", (long long)n_rows);
  if (ignore_index >= 0)
    return set_err(LDDL_EINVAL, "ignore_index %lld could be a label: it must be negative", (long long)ignore_index);
  if (total < 0 || capacity < 0) return set_err(LDDL_EINVAL, "negative total / capacity");
  if (total > 0 && !d_labels) return set_err(LDDL_EINVAL, "null labels");
  // total / n_rows == seq_len without a product that could overflow
  if (!d_cu_seqlens && (seq_len < 1 || total % n_rows != 0 || total / n_rows != seq_len))
    return set_err(LDDL_EINVAL, "a padded batch of %lld rows of %lld columns does not hold %lld labels", (long long)n_rows,
                   (long long)seq_len, (long long)total);
  if (total > INT32_MAX || n_rows > INT32_MAX)
    return set_err(LDDL_ECAPACITY, "total %lld / n_rows %lld: offsets are int32", (long long)total, (long long)n_rows);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  MlmTargetsParams P{};
  P.labels = d_labels;
  P.cu_seqlens = d_cu_seqlens;
  P.n_rows = n_rows;
  P.seq_len = seq_len;
  P.total = total;
  P.ignore_index = ignore_index;
  P.capacity = capacity;
  P.positions = d_positions;
  P.target_labels = d_target_labels;
  P.offsets = d_offsets;
  P.n_chunks = collate_chunks(n_rows);
  // one buffer, one memset: M, the error word (the layout of HW_CU_TOTAL, HW_MAX_LEN), then the chunk sums
  unsigned long long* words;
  int rc;
  if ((rc = ws_get(c, CW_SHARED_BSUM, (size_t)P.n_chunks + 2, &words))) return rc;
  P.count_out = (int64_t*)words;
  P.err = (uint32_t*)(words + 1);
  P.chunk_sum = words + 2;
  HIP_TRY(hipMemsetAsync(words, 0, ((size_t)P.n_chunks + 2) * sizeof(*words), st));
  HIP_TRY(launch_mlm_targets(P, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_CU_TOTAL, words, 16, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t count = c->h_tot[HW_CU_TOTAL];
  const uint32_t e = (uint32_t)(c->h_tot[HW_MAX_LEN] & 0xFFFFFFFF);
  *out_count = count;
  if (e)
    return set_err(LDDL_EINVAL, "row %llu: cu_seqlens do not hold a row within [0, total %lld)", (unsigned long long)(e >> 4),
                   (long long)total);
  if (count > capacity)
    return set_err(LDDL_ECAPACITY, "%lld masked positions, capacity %lld", (long long)count, (long long)capacity);
  return 0;
}

// ------------------------------------------- a row table from a shard's strings --
static int rows_from_strings_error(uint32_t e) {
  const unsigned long long row = e >> 4;
  switch (e & 15u) {
    case CERR_LONG: return set_err(LDDL_ECAPACITY, "row %llu: a segment of more than 65535 tokens", row);
    case CERR_NMASK: return set_err(LDDL_ECAPACITY, "row %llu: more masked_lm_positions than a row has tokens", row);
    case CERR_TABLE_CAP: return set_err(LDDL_ECAPACITY, "the table's ids or masked entries exceed ids_cap / mlm_cap");
    case CERR_POS_RANGE: return set_err(LDDL_EINDEX, "row %llu: masked_lm_positions index beyond the row's tokens", row);
    case CERR_NPY: return set_err(LDDL_EFORMAT, "row %llu: masked_lm_positions is not np.save bytes", row);
    case CERR_NLAB:
      return set_err(LDDL_EFORMAT, "row %llu: masked_lm_positions and masked_lm_labels differ in length", row);
    case CERR_CODE_ROW:
      return set_err(LDDL_EFORMAT,
                     "row %llu: num_tokens is neither doc + code + 3 nor, with an empty doc, code + 2 (tokens by split())", row);
    default:
      return set_err(LDDL_EINVAL, "row %llu: len0 / len1 / src0 / src1 / mlm_off are not what its strings give", row);
  }
}

// lddl_rows_from_strings_len (fill 0: the outputs d_len0 .. d_mlm_off, d_tok_off, out_totals) and
// lddl_rows_from_strings (fill 1: the same arrays as inputs, d_is_random_next and the table) validate their
// arguments and fill RowsFromStringsParams here, once; the arguments of the other call arrive as 0 / NULL.
// code 1: the lddl_code_rows_from_strings[_len] twins over doc / code with d_num_tokens in place of
// d_is_random_next and the static columns; out_totals is then {ids, row tokens}.
static int rows_from_strings_common(lddl_ctx* c, int fill, int code, const uint8_t* d_a, const int64_t* d_a_off,
                                    const uint8_t* d_b, const int64_t* d_b_off, const uint8_t* d_pos,
                                    const int64_t* d_pos_off, const uint8_t* d_lab, const int64_t* d_lab_off,
                                    const uint8_t* d_is_random_next, const uint16_t* d_num_tokens, int64_t n_rows, uint16_t* d_len0, uint16_t* d_len1,
                                    int64_t* d_src0, int64_t* d_src1, int64_t* d_tok_off, int64_t* d_mlm_off,
                                    int64_t* out_totals, uint16_t* d_ids, int64_t ids_cap, uint8_t* d_flags,
                                    uint16_t* d_mlm_pos, uint16_t* d_mlm_label, uint16_t* d_mlm_token, int64_t mlm_cap,
                                    void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_rows <= 0) return set_err(LDDL_EINVAL, "n_rows %lld: a table has one row at least", (long long)n_rows);
  if (!d_a || !d_a_off || !d_b || !d_b_off) return set_err(LDDL_EINVAL, "null column pointer");
  if (!d_len0 || !d_len1 || !d_src0 || !d_src1 || (code ? !d_num_tokens : fill && !d_is_random_next) ||
      (fill ? !d_ids || !d_flags : !out_totals))
    return set_err(LDDL_EINVAL, "null pointer");
  const int n_static = (d_pos != nullptr) + (d_pos_off != nullptr) + (d_lab != nullptr) + (d_lab_off != nullptr);
  if (n_static != 0 && n_static != 4)
    return set_err(LDDL_EINVAL, "static masking needs positions and labels, all four pointers or none");
  const int n_out = (d_mlm_off != nullptr) + (fill ? (d_mlm_pos != nullptr) + (d_mlm_label != nullptr) + (d_mlm_token != nullptr) : 0);
  if (n_out != (n_static ? (fill ? 4 : 1) : 0))
    return set_err(LDDL_EINVAL, n_static ? "static inputs without the static outputs" : "static outputs without static inputs");
  if (fill && (ids_cap < 0 || mlm_cap < 0)) return set_err(LDDL_EINVAL, "negative capacity");
  if (c->vocab_size > 65536) return set_err(LDDL_EINVAL, "a vocabulary of %d entries: an id would not fit 16 bits", c->vocab_size);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  RowsFromStringsParams P{};
  int rc;
  if (fill && (rc = collate_vocab(c, &P.V))) return rc;
  P.C = StringColumns{d_a, d_a_off, d_b, d_b_off, d_pos, d_pos_off, d_lab, d_lab_off};
  P.is_random_next = d_is_random_next;
  P.num_tokens = d_num_tokens;
  P.n_rows = n_rows;
  P.len0 = d_len0;
  P.len1 = d_len1;
  P.src0 = d_src0;
  P.src1 = d_src1;
  P.tok_off = d_tok_off;
  P.mlm_off = d_mlm_off;
  P.ids = d_ids;
  P.ids_cap = ids_cap;
  P.flags = d_flags;
  P.mlm_pos = d_mlm_pos;
  P.mlm_label = d_mlm_label;
  P.mlm_token = d_mlm_token;
  P.mlm_cap = mlm_cap;
  uint32_t e;
  if ((rc = ws_get(c, CW_COLLATE_ERR, 1, &P.err))) return rc;
  HIP_TRY(hipMemsetAsync(P.err, 0, 4, st));
  if (fill) {
    HIP_TRY(launch_rows_from_strings(P, c->n_cu, st));
    if ((rc = read_err(c, P.err, st, &e))) return rc;
    return e ? rows_from_strings_error(e) : 0;
  }
  P.n_chunks = collate_chunks(n_rows);
  if ((rc = ws_get(c, CW_SHARED_META, 3, &P.totals)) || (rc = ws_get(c, CW_SHARED_BSUM, (size_t)P.n_chunks, &P.chunk_sum)))
    return rc;
  HIP_TRY(hipMemsetAsync(P.chunk_sum, 0, (size_t)P.n_chunks * sizeof(*P.chunk_sum), st));
  HIP_TRY(launch_rows_from_strings_len(P, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_NTOK, P.totals, 24, st));  // ids, row tokens, masked: HW_NTOK, HW_PACK_ERR, HW_NMASK
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return rows_from_strings_error(e);
  out_totals[0] = c->h_tot[HW_NTOK];
  if (code) {
    out_totals[1] = c->h_tot[HW_PACK_ERR];
    return 0;
  }
  out_totals[1] = c->h_tot[HW_NMASK];
  out_totals[2] = c->h_tot[HW_PACK_ERR];
  return 0;
}

extern "C" int lddl_rows_from_strings_len(lddl_ctx* c, const uint8_t* d_a, const int64_t* d_a_off, const uint8_t* d_b,
                                          const int64_t* d_b_off, const uint8_t* d_pos, const int64_t* d_pos_off,
                                          const uint8_t* d_lab, const int64_t* d_lab_off, int64_t n_rows,
                                          uint16_t* d_out_len0, uint16_t* d_out_len1, int64_t* d_out_src0,
                                          int64_t* d_out_src1, int64_t* d_out_tok_off, int64_t* d_out_mlm_off,
                                          int64_t out_totals[3], void* stream) {
  return rows_from_strings_common(c, 0, 0, d_a, d_a_off, d_b, d_b_off, d_pos, d_pos_off, d_lab, d_lab_off, nullptr, nullptr,
                                  n_rows,
                                  d_out_len0, d_out_len1, d_out_src0, d_out_src1, d_out_tok_off, d_out_mlm_off, out_totals,
                                  nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int lddl_rows_from_strings(lddl_ctx* c, const uint8_t* d_a, const int64_t* d_a_off, const uint8_t* d_b,
                                      const int64_t* d_b_off, const uint8_t* d_pos, const int64_t* d_pos_off,
                                      const uint8_t* d_lab, const int64_t* d_lab_off, const uint8_t* d_is_random_next,
                                      int64_t n_rows, const uint16_t* d_len0, const uint16_t* d_len1,
                                      const int64_t* d_src0, const int64_t* d_src1, const int64_t* d_mlm_off,
                                      uint16_t* d_out_ids, int64_t ids_cap, uint8_t* d_out_flags, uint16_t* d_out_mlm_pos,
                                      uint16_t* d_out_mlm_label, uint16_t* d_out_mlm_token, int64_t mlm_cap, void* stream) {
  // read only by the fill pass
  return rows_from_strings_common(c, 1, 0, d_a, d_a_off, d_b, d_b_off, d_pos, d_pos_off, d_lab, d_lab_off, d_is_random_next,
                                  nullptr, n_rows, const_cast<uint16_t*>(d_len0), const_cast<uint16_t*>(d_len1),
                                  const_cast<int64_t*>(d_src0), const_cast<int64_t*>(d_src1), nullptr,
                                  const_cast<int64_t*>(d_mlm_off), nullptr, d_out_ids, ids_cap, d_out_flags, d_out_mlm_pos,
                                  d_out_mlm_label, d_out_mlm_token, mlm_cap, stream);
}

// --------------------------------------- the same from a CodeBERT shard's strings --
extern "C" int lddl_code_rows_from_strings_len(lddl_ctx* c, const uint8_t* d_doc, const int64_t* d_doc_off,
                                               const uint8_t* d_code, const int64_t* d_code_off,
                                               const uint16_t* d_num_tokens, int64_t n_rows, uint16_t* d_out_len0,
                                               uint16_t* d_out_len1, int64_t* d_out_src0, int64_t* d_out_src1,
                                               int64_t* d_out_tok_off, int64_t out_totals[2], void* stream) {
  return rows_from_strings_common(c, 0, 1, d_doc, d_doc_off, d_code, d_code_off, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  d_num_tokens, n_rows, d_out_len0, d_out_len1, d_out_src0, d_out_src1, d_out_tok_off,
                                  nullptr, out_totals, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int lddl_code_rows_from_strings(lddl_ctx* c, const uint8_t* d_doc, const int64_t* d_doc_off,
                                           const uint8_t* d_code, const int64_t* d_code_off, const uint16_t* d_num_tokens,
                                           int64_t n_rows, const uint16_t* d_len0, const uint16_t* d_len1,
                                           const int64_t* d_src0, const int64_t* d_src1, uint16_t* d_out_ids,
                                           int64_t ids_cap, uint8_t* d_out_flags, void* stream) {
  // read only by the fill pass
  return rows_from_strings_common(c, 1, 1, d_doc, d_doc_off, d_code, d_code_off, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  d_num_tokens, n_rows, const_cast<uint16_t*>(d_len0), const_cast<uint16_t*>(d_len1),
                                  const_cast<int64_t*>(d_src0), const_cast<int64_t*>(d_src1), nullptr, nullptr, nullptr,
                                  d_out_ids, ids_cap, d_out_flags, nullptr, nullptr, nullptr, 0, stream);
}
