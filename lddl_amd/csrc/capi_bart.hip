// C-ABI, host side of the BART sentence aggregation (kernels: bart.hip).
#include "bart.h"
#include "capi_ctx.h"

// the device words of the lddl_bart_* calls, int64 slots of CW_SHARED_META
enum BartMeta { BM_BYTES, BM_BAD, BM_ERR, BM_COUNT };

static int bart_err(uint32_t e, const char* call) {
  switch (e & 0xF) {
    case BART_E_SENT:
      return set_err(LDDL_EINVAL, "%s: a sentence's offsets run backwards or leave [0, nbytes]", call);
    case BART_E_DOC:
      return set_err(LDDL_EINVAL, "%s: a document's sentences run backwards or leave [0, n_sent]", call);
    case BART_E_BYTES:
      return set_err(LDDL_ECAPACITY, "%s: a chunk of 2^31 bytes or more", call);
    default:
      return set_err(LDDL_EINVAL, "%s: d_doc_chunk_off / n_chunks are not what lddl_bart_plan_len gives", call);
  }
}

extern "C" int lddl_bart_count(lddl_ctx* c, const uint8_t* d_data, int64_t nbytes, const int64_t* d_sent_off,
                               int64_t n_sent, int32_t* d_out_nwords, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (nbytes < 0 || n_sent < 0) return set_err(LDDL_EINVAL, "negative count");
  if (!d_sent_off || (n_sent > 0 && !d_out_nwords) || (nbytes > 0 && !d_data)) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int64_t* meta;
  int rc;
  if ((rc = ws_get(c, CW_SHARED_META, BM_COUNT, &meta))) return rc;
  BartCountParams P{};
  P.data = d_data;
  P.nbytes = nbytes;
  P.sent_off = d_sent_off;
  P.n_sent = n_sent;
  P.nwords = d_out_nwords;
  P.err = (uint32_t*)(meta + BM_ERR);
  HIP_TRY(hipMemsetAsync(P.err, 0, 4, st));
  HIP_TRY(launch_bart_count(P, c->n_cu, st));
  uint32_t e;
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return bart_err(e, "lddl_bart_count");
  return 0;
}

static int plan_args(lddl_ctx* c, const int32_t* d_nwords, const int64_t* d_sent_off, const int64_t* d_doc_sent_off,
                     int64_t n_doc, int64_t n_sent) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_doc < 0 || n_sent < 0) return set_err(LDDL_EINVAL, "negative count");
  if (!d_sent_off || !d_doc_sent_off || (n_sent > 0 && !d_nwords)) return set_err(LDDL_EINVAL, "null pointer");
  return 0;
}

extern "C" int lddl_bart_plan_len(lddl_ctx* c, const int32_t* d_nwords, const int64_t* d_sent_off,
                                  const int64_t* d_doc_sent_off, int64_t n_doc, int64_t n_sent,
                                  int32_t target_seq_length, int64_t* d_out_doc_chunk_off, int64_t out_totals[2],
                                  void* stream) {
  int rc;
  if ((rc = plan_args(c, d_nwords, d_sent_off, d_doc_sent_off, n_doc, n_sent))) return rc;
  if (!d_out_doc_chunk_off || !out_totals) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int64_t *meta, *bsum;
  BartPlanParams P{};
  if ((rc = ws_get(c, CW_SHARED_META, BM_COUNT, &meta)) || (rc = ws_get(c, CW_SHARED_ROWS, (size_t)n_doc, &P.doc_nchunks)) ||
      (rc = ws_get(c, CW_SHARED_BSUM, (size_t)scan_blocks(n_doc) + 1, &bsum)))
    return rc;
  P.nwords = d_nwords;
  P.sent_off = d_sent_off;
  P.doc_sent_off = d_doc_sent_off;
  P.n_doc = n_doc;
  P.n_sent = n_sent;
  P.target = (int64_t)target_seq_length - 3;
  P.total_bytes = (unsigned long long*)(meta + BM_BYTES);
  P.err = (uint32_t*)(meta + BM_ERR);
  HIP_TRY(hipMemsetAsync(meta, 0, BM_COUNT * sizeof(int64_t), st));
  HIP_TRY(launch_bart_plan_len(P, c->n_cu, st));
  HIP_TRY(launch_scan_ntok(P.doc_nchunks, n_doc, d_out_doc_chunk_off, bsum, st));
  HIP_TRY(fetch_word(c, HW_BART_LO, d_out_doc_chunk_off + n_doc, 8, st));
  HIP_TRY(fetch_word(c, HW_BART_HI, meta + BM_BYTES, 8, st));
  // the last entry of doc_sent_off against n_sent, under the same synchronize
  HIP_TRY(fetch_word(c, HW_BART_NSENT, d_doc_sent_off + n_doc, 8, st));
  uint32_t e;
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return bart_err(e, "lddl_bart_plan_len");
  if (c->h_tot[HW_BART_NSENT] != n_sent)
    return set_err(LDDL_EINVAL, "lddl_bart_plan_len: d_doc_sent_off ends at %lld, n_sent is %lld",
                   (long long)c->h_tot[HW_BART_NSENT], (long long)n_sent);
  out_totals[0] = c->h_tot[HW_BART_LO];
  out_totals[1] = c->h_tot[HW_BART_HI];
  return 0;
}

extern "C" int lddl_bart_plan(lddl_ctx* c, const int32_t* d_nwords, const int64_t* d_sent_off,
                              const int64_t* d_doc_sent_off, const int64_t* d_doc_chunk_off, int64_t n_doc,
                              int64_t n_sent, int32_t target_seq_length, int64_t n_chunks, int64_t* d_out_chunk_sent0,
                              int32_t* d_out_chunk_nsent, int32_t* d_out_chunk_num_tokens, int64_t* d_out_chunk_off,
                              void* stream) {
  int rc;
  if ((rc = plan_args(c, d_nwords, d_sent_off, d_doc_sent_off, n_doc, n_sent))) return rc;
  if (n_chunks < 0) return set_err(LDDL_EINVAL, "negative count");
  if (!d_doc_chunk_off || !d_out_chunk_off ||
      (n_chunks > 0 && (!d_out_chunk_sent0 || !d_out_chunk_nsent || !d_out_chunk_num_tokens)))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int64_t *meta, *bsum;
  BartPlanParams P{};
  if ((rc = ws_get(c, CW_SHARED_META, BM_COUNT, &meta)) || (rc = ws_get(c, CW_SHARED_ROWS, (size_t)n_chunks, &P.chunk_len)) ||
      (rc = ws_get(c, CW_SHARED_BSUM, (size_t)scan_blocks(n_chunks) + 1, &bsum)))
    return rc;
  P.nwords = d_nwords;
  P.sent_off = d_sent_off;
  P.doc_sent_off = d_doc_sent_off;
  P.n_doc = n_doc;
  P.n_sent = n_sent;
  P.target = (int64_t)target_seq_length - 3;
  P.err = (uint32_t*)(meta + BM_ERR);
  P.doc_chunk_off = d_doc_chunk_off;
  P.n_chunks = n_chunks;
  P.chunk_sent0 = d_out_chunk_sent0;
  P.chunk_nsent = d_out_chunk_nsent;
  P.chunk_num_tokens = d_out_chunk_num_tokens;
  HIP_TRY(hipMemsetAsync(meta, 0, BM_COUNT * sizeof(int64_t), st));
  // the lengths start at 0 (the slot is shared and holds an earlier call's values): after a refused plan the
  // scan sums only what this call's walk stored
  if (n_chunks > 0) {
    HIP_TRY(hipMemsetAsync(P.chunk_len, 0, (size_t)n_chunks * sizeof(int32_t), st));
  }
  HIP_TRY(launch_bart_plan_fill(P, c->n_cu, st));
  HIP_TRY(launch_scan_ntok(P.chunk_len, n_chunks, d_out_chunk_off, bsum, st));
  HIP_TRY(fetch_word(c, HW_BART_LO, d_doc_chunk_off + n_doc, 8, st));
  uint32_t e;
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e) return bart_err(e, "lddl_bart_plan");
  if (c->h_tot[HW_BART_LO] != n_chunks)
    return set_err(LDDL_EINVAL, "lddl_bart_plan: d_doc_chunk_off ends at %lld, n_chunks is %lld",
                   (long long)c->h_tot[HW_BART_LO], (long long)n_chunks);
  return 0;
}

extern "C" int lddl_bart_render(lddl_ctx* c, const uint8_t* d_data, int64_t nbytes, const int64_t* d_sent_off,
                                int64_t n_sent, const int64_t* d_chunk_sent0, const int32_t* d_chunk_nsent,
                                const int64_t* d_chunk_off, int64_t n_chunks, int64_t c0, int64_t n, int64_t* d_out_off,
                                uint8_t* d_out_bytes, int64_t out_cap, int64_t* out_nbytes, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (nbytes < 0 || n_sent < 0 || n_chunks < 0 || c0 < 0 || n < 0) return set_err(LDDL_EINVAL, "negative count");
  if (c0 > n_chunks || n > n_chunks - c0)
    return set_err(LDDL_EINVAL, "chunks [%lld, %lld + %lld) leave the %lld of the plan", (long long)c0, (long long)c0,
                   (long long)n, (long long)n_chunks);
  if (!d_sent_off || !d_chunk_off || !d_out_off || !out_nbytes || (nbytes > 0 && !d_data) ||
      (n > 0 && (!d_chunk_sent0 || !d_chunk_nsent)))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int64_t* meta;
  int rc;
  if ((rc = ws_get(c, CW_SHARED_META, BM_COUNT, &meta))) return rc;
  BartRenderParams R{};
  R.data = d_data;
  R.nbytes = nbytes;
  R.sent_off = d_sent_off;
  R.n_sent = n_sent;
  R.chunk_sent0 = d_chunk_sent0;
  R.chunk_nsent = d_chunk_nsent;
  R.chunk_off = d_chunk_off;
  R.c0 = c0;
  R.n = n;
  R.out_off = d_out_off;
  R.bad = (unsigned long long*)(meta + BM_BAD);
  // size pass: the offsets rebased to 0 and the range's two ends read back
  HIP_TRY(launch_bart_rebase(R, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_BART_LO, d_chunk_off + c0, 8, st));
  HIP_TRY(fetch_word(c, HW_BART_HI, d_chunk_off + c0 + n, 8, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t lo = c->h_tot[HW_BART_LO], hi = c->h_tot[HW_BART_HI];
  if (lo < 0 || hi < lo)
    return set_err(LDDL_EINVAL, "lddl_bart_render: d_chunk_off runs from %lld to %lld over chunks [%lld, %lld)",
                   (long long)lo, (long long)hi, (long long)c0, (long long)(c0 + n));
  const int64_t total = hi - lo;
  *out_nbytes = total;
  if (!d_out_bytes) return 0;  // size query
  if (out_cap < total)
    return set_err(LDDL_ECAPACITY, "render needs %lld bytes, out_cap %lld", (long long)total, (long long)out_cap);
  if (n == 0) return 0;
  R.out = d_out_bytes;
  R.out_cap = out_cap;
  HIP_TRY(hipMemsetAsync(R.bad, 0xFF, 8, st));
  HIP_TRY(launch_bart_render(R, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_BART_HI, R.bad, 8, st));
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned long long bad = (unsigned long long)c->h_tot[HW_BART_HI];
  if (bad != BART_NO_CHUNK)
    return set_err(LDDL_EINVAL, "lddl_bart_render: chunk %llu is not what its sentences give (sentence range, "
                   "byte count or output span); it is left unwritten", bad);
  return 0;
}
