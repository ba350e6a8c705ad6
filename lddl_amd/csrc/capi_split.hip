// C-ABI, host side of the sentence split (kernels: split.hip).
#include "capi_ctx.h"
#include "split.h"

extern "C" int lddl_set_split_props(lddl_ctx* c, const uint8_t* host_tab, int64_t n) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (!host_tab) return set_err(LDDL_EINVAL, "null pointer");
  if (n != SPLIT_PROPS_N)
    return set_err(LDDL_EINVAL, "lddl_set_split_props: the table has %lld entries, one per code point (%lld) is needed",
                   (long long)n, (long long)SPLIT_PROPS_N);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->d_split_props) HIP_TRY(hipMalloc((void**)&c->d_split_props, (size_t)SPLIT_PROPS_N));
  HIP_TRY(hipMemcpy(c->d_split_props, host_tab, (size_t)SPLIT_PROPS_N, hipMemcpyHostToDevice));
  return 0;
}

static int split_args(lddl_ctx* c, const uint8_t* d_buf, int64_t nbytes, const int64_t* d_rec_off, int64_t n_rec,
                      int32_t mode, const char* call) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (nbytes < 0 || n_rec < 0) return set_err(LDDL_EINVAL, "negative count");
  if (mode != 0 && mode != 1) return set_err(LDDL_EINVAL, "%s: mode %d is neither 0 (id + body) nor 1 (whole line)", call, (int)mode);
  if (!d_rec_off || (nbytes > 0 && !d_buf)) return set_err(LDDL_EINVAL, "null pointer");
  if (!c->d_split_props) return set_err(LDDL_EINVAL, "%s: lddl_set_split_props has not been called on this ctx", call);
  if (nbytes >= 0x7FFFFFFFll) return set_err(LDDL_ECAPACITY, "%s: a buffer of 2^31 bytes or more", call);
  return 0;
}

// The passes both calls run: head, count and the scan of the records' sentence counts into d_dso [n_rec + 1].
// fill: the first-sentence bitmap and the per-piece counts with their scan as well.  Everything is queued on st.
static int split_count_passes(lddl_ctx* c, SentSplitParams& P, int64_t* d_dso, bool fill, int64_t n_sent_hint,
                              int64_t** meta_out, int64_t** bsum_out, hipStream_t st) {
  int rc;
  int64_t *meta, *bsum, *rec, *piece = nullptr;
  const int64_t n_rec = P.n_rec, n_pieces = split_pieces(P.nbytes);
  const int64_t scan_n = std::max(std::max(n_rec, n_pieces), n_sent_hint);
  if ((rc = ws_get(c, CW_SHARED_META, SM_COUNT, &meta)) ||
      (rc = ws_get(c, CW_SHARED_BSUM, (size_t)scan_blocks(scan_n) + 1, &bsum)) ||
      (rc = ws_get(c, CW_SPLIT_REC, (size_t)(n_rec + 1) + (size_t)(3 * n_rec + 1) / 2 + 1, &rec)))
    return rc;
  int64_t* const ws_dso = rec;
  P.rec_b0 = (int32_t*)(rec + n_rec + 1);
  P.rec_end = P.rec_b0 + n_rec;
  P.rec_cnt = P.rec_end + n_rec;
  P.bytes = (unsigned long long*)(meta + SM_BYTES);
  P.bad_rec = (unsigned long long*)(meta + SM_BAD);
  P.err = (uint32_t*)(meta + SM_ERR);
  HIP_TRY(hipMemsetAsync(meta, 0, SM_COUNT * sizeof(int64_t), st));
  HIP_TRY(hipMemsetAsync(P.bad_rec, 0xFF, 8, st));
  if (fill) {
    const size_t words = (size_t)(P.nbytes >> 6) + 1;
    if ((rc = ws_get(c, CW_SPLIT_MAP, words, &P.fsmap)) ||
        (rc = ws_get(c, CW_SPLIT_PIECE, (size_t)(n_pieces + 1) + (size_t)(n_pieces + 1) / 2 + 1, &piece)))
      return rc;
    P.piece_cnt = (int32_t*)(piece + n_pieces + 1);
    P.piece_base = piece;
    HIP_TRY(hipMemsetAsync(P.fsmap, 0, words * 8, st));
    d_dso = ws_dso;
    P.doc_sent_off = ws_dso;
  }
  HIP_TRY(launch_split_head(P, c->n_cu, st));
  HIP_TRY(launch_split_count(P, c->n_cu, st));
  HIP_TRY(launch_scan_ntok(P.rec_cnt, n_rec, d_dso, bsum, st));
  if (fill) HIP_TRY(launch_scan_ntok(P.piece_cnt, n_pieces, piece, bsum, st));
  *meta_out = meta;
  *bsum_out = bsum;
  return 0;
}

extern "C" int lddl_split_len(lddl_ctx* c, const uint8_t* d_buf, int64_t nbytes, const int64_t* d_rec_off,
                              int64_t n_rec, int32_t mode, int64_t* d_out_doc_sent_off, int64_t* d_out_id_end,
                              int64_t out_totals[2], int64_t* out_bad_rec, void* stream) {
  int rc;
  if ((rc = split_args(c, d_buf, nbytes, d_rec_off, n_rec, mode, "lddl_split_len"))) return rc;
  if (!d_out_doc_sent_off || !out_totals || !out_bad_rec || (mode == 0 && n_rec > 0 && !d_out_id_end))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  SentSplitParams P{};
  P.buf = d_buf;
  P.nbytes = nbytes;
  P.rec_off = d_rec_off;
  P.n_rec = n_rec;
  P.mode = mode;
  P.props = c->d_split_props;
  P.id_end = d_out_id_end;
  int64_t *meta, *bsum;
  *out_bad_rec = -1;
  if ((rc = split_count_passes(c, P, d_out_doc_sent_off, false, 0, &meta, &bsum, st))) return rc;
  HIP_TRY(fetch_word(c, HW_SPLIT_NSENT, d_out_doc_sent_off + n_rec, 8, st));
  HIP_TRY(fetch_word(c, HW_SPLIT_BYTES, meta + SM_BYTES, 16, st));
  uint32_t e;
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e)
    return set_err(LDDL_EINVAL, "lddl_split_len: d_rec_off does not start at 0, runs backwards or does not end at nbytes");
  if ((unsigned long long)c->h_tot[HW_SPLIT_BAD] != SPLIT_NO_REC) {
    *out_bad_rec = c->h_tot[HW_SPLIT_BAD];
    return set_err(LDDL_EFORMAT, "lddl_split_len: record %lld is not valid UTF-8", (long long)*out_bad_rec);
  }
  out_totals[0] = c->h_tot[HW_SPLIT_NSENT];
  out_totals[1] = c->h_tot[HW_SPLIT_BYTES];
  return 0;
}
static_assert(HW_SPLIT_BAD == HW_SPLIT_BYTES + 1 && SM_BAD == SM_BYTES + 1, "lddl_split[_len] read bytes and bad record with one copy");

extern "C" int lddl_split(lddl_ctx* c, const uint8_t* d_buf, int64_t nbytes, const int64_t* d_rec_off, int64_t n_rec,
                          int32_t mode, const int64_t* d_doc_sent_off, int64_t n_sent, int64_t out_bytes,
                          uint8_t* d_out_data, int64_t* d_out_sent_off, void* stream) {
  int rc;
  if ((rc = split_args(c, d_buf, nbytes, d_rec_off, n_rec, mode, "lddl_split"))) return rc;
  if (n_sent < 0 || out_bytes < 0) return set_err(LDDL_EINVAL, "negative count");
  if (!d_doc_sent_off || !d_out_data || !d_out_sent_off) return set_err(LDDL_EINVAL, "null pointer");
  // (a sentence is at least a byte of the input: larger counts cannot be lddl_split_len's, and the workspace
  // below is sized by them)
  if (n_sent > nbytes || out_bytes > nbytes)
    return set_err(LDDL_EINVAL, "lddl_split: n_sent %lld / out_bytes %lld are not what lddl_split_len gives for %lld bytes",
                   (long long)n_sent, (long long)out_bytes, (long long)nbytes);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  SentSplitParams P{};
  P.buf = d_buf;
  P.nbytes = nbytes;
  P.rec_off = d_rec_off;
  P.n_rec = n_rec;
  P.mode = mode;
  P.props = c->d_split_props;
  P.user_doc_sent_off = d_doc_sent_off;
  P.n_sent = n_sent;
  P.out_bytes = out_bytes;
  P.out = d_out_data;
  // nothing of the length call is kept in the ctx: its passes run again, and the caller's three values are
  // compared with what they give before anything is stored through them
  int64_t *meta, *bsum;
  if ((rc = split_count_passes(c, P, nullptr, true, n_sent, &meta, &bsum, st))) return rc;
  HIP_TRY(launch_split_compare(P, c->n_cu, st));
  HIP_TRY(fetch_word(c, HW_SPLIT_NSENT, P.doc_sent_off + n_rec, 8, st));
  HIP_TRY(fetch_word(c, HW_SPLIT_BYTES, meta + SM_BYTES, 16, st));
  uint32_t e;
  if ((rc = read_err(c, P.err, st, &e))) return rc;
  if (e == SPLIT_E_RECOFF)
    return set_err(LDDL_EINVAL, "lddl_split: d_rec_off does not start at 0, runs backwards or does not end at nbytes");
  if ((unsigned long long)c->h_tot[HW_SPLIT_BAD] != SPLIT_NO_REC)
    return set_err(LDDL_EFORMAT, "lddl_split: record %lld is not valid UTF-8", (long long)c->h_tot[HW_SPLIT_BAD]);
  if (e) return set_err(LDDL_EINVAL, "lddl_split: d_doc_sent_off is not what lddl_split_len gives for this input");
  if (c->h_tot[HW_SPLIT_NSENT] != n_sent || c->h_tot[HW_SPLIT_BYTES] != out_bytes)
    return set_err(LDDL_EINVAL, "lddl_split: the input has %lld sentences of %lld bytes, n_sent is %lld and out_bytes %lld",
                   (long long)c->h_tot[HW_SPLIT_NSENT], (long long)c->h_tot[HW_SPLIT_BYTES], (long long)n_sent,
                   (long long)out_bytes);
  if ((rc = ws_get(c, CW_SPLIT_SENT, (size_t)2 * n_sent, &P.sent_start))) return rc;
  P.sent_end = P.sent_start + n_sent;
  P.sent_off = d_out_sent_off;
  HIP_TRY(launch_split_mark(P, c->n_cu, st));
  HIP_TRY(launch_split_tail(P, c->n_cu, st));
  HIP_TRY(launch_split_lens(P, c->n_cu, st));
  HIP_TRY(launch_scan_ntok(P.sent_end, n_sent, d_out_sent_off, bsum, st));
  HIP_TRY(launch_split_copy(P, c->n_cu, st));
  HIP_TRY(hipMemsetAsync(d_out_data + out_bytes, 0, 16, st));  // the tokenizer's padding
  return 0;
}
