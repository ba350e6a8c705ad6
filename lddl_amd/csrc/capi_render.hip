// C-ABI, host side of the string-column renders (kernels: render.hip).
#include "capi_ctx.h"

// First half of a render: the lens workspace, the length pass, the offset
// scan, and the byte total read back into HW_RENDER_BYTES -- under the same
// synchronize as the error word where the call has one (d_err, cleared here, *e).
template <class Params>
static int render_total(lddl_ctx* c, Params& R, hipError_t (*launch_len)(const Params&, int, hipStream_t),
                        int64_t* d_out_off, hipStream_t st, int32_t* d_err = nullptr, uint32_t* e = nullptr) {
  int64_t* bsum;
  int rc;
  if ((rc = ws_get(c, CW_SHARED_ROWS, (size_t)R.n_rows, &R.lens)) ||
      (rc = ws_get(c, CW_SHARED_BSUM, (size_t)scan_blocks(R.n_rows) + 1, &bsum)))
    return rc;
  if (d_err) HIP_TRY(hipMemsetAsync(d_err, 0, 4, st));
  HIP_TRY(launch_len(R, c->n_cu, st));
  HIP_TRY(launch_scan_ntok(R.lens, R.n_rows, d_out_off, bsum, st));
  HIP_TRY(fetch_word(c, HW_RENDER_BYTES, d_out_off + R.n_rows, 8, st));
  if (d_err) return read_err(c, d_err, st, e);
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

// Reports the total, answers a size query (0) and refuses a short buffer (< 0); 1: the bytes pass may write
static int render_room(const lddl_ctx* c, const uint8_t* d_out_bytes, int64_t out_cap, int64_t* out_nbytes) {
  const int64_t total = c->h_tot[HW_RENDER_BYTES];
  *out_nbytes = total;
  if (!d_out_bytes) return 0;  // size query
  if (out_cap < total)
    return set_err(LDDL_ECAPACITY, "render needs %lld bytes, out_cap %lld", (long long)total, (long long)out_cap);
  return 1;
}

// lddl_render_strings / lddl_render_masked after their parameter setup
static int render_tail(lddl_ctx* c, RenderParams& R, int64_t* d_out_off, uint8_t* d_out_bytes, int64_t out_cap,
                       int64_t* out_nbytes, hipStream_t st) {
  int rc;
  if ((rc = render_total(c, R, launch_render_len, d_out_off, st))) return rc;
  if ((rc = render_room(c, d_out_bytes, out_cap, out_nbytes)) <= 0) return rc;
  R.out_off = d_out_off;
  R.out = d_out_bytes;
  HIP_TRY(launch_render_bytes(R, c->n_cu, st));
  return 0;
}

extern "C" int lddl_render_strings(lddl_ctx* c, const uint16_t* d_tokens, const int64_t* d_row_off,
                                   const uint16_t* d_len0, const uint16_t* d_len1, const uint8_t* d_flags,
                                   int64_t row0, int64_t n_rows, int32_t segment, int32_t codebert,
                                   int64_t* d_out_off, uint8_t* d_out_bytes, int64_t out_cap, int64_t* out_nbytes,
                                   void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (segment < RENDER_SEG0 || segment > RENDER_SPAN) return set_err(LDDL_EINVAL, "segment %d not in 0..3", segment);
  if (row0 < 0 || n_rows < 0) return set_err(LDDL_EINVAL, "negative row range");
  if (!d_tokens || !d_row_off || !d_out_off || !out_nbytes) return set_err(LDDL_EINVAL, "null pointer");
  if (segment != RENDER_ROW && (!d_len0 || (segment == RENDER_SEG1 && (!d_len1 || (codebert && !d_flags)))))
    return set_err(LDDL_EINVAL, "segment %d needs len0/len1%s", segment, codebert ? "/flags" : "");
  HIP_TRY(hipSetDevice(c->device));
  RenderParams R{};
  R.tokens = d_tokens;
  R.row_off = d_row_off;
  R.len0 = d_len0;
  R.len1 = d_len1;
  R.flags = d_flags;
  R.row0 = row0;
  R.n_rows = n_rows;
  R.segment = segment;
  R.codebert = codebert;
  R.vinfo = c->d_rinfo;
  R.vpool = c->d_rpool;
  return render_tail(c, R, d_out_off, d_out_bytes, out_cap, out_nbytes, (hipStream_t)stream);
}

extern "C" int lddl_render_npy(lddl_ctx* c, const int64_t* d_mlm_off, const uint16_t* d_mlm_pos, int64_t row0,
                               int64_t n_rows, const uint16_t* d_hdr, int32_t hdr_len, int32_t kmax, int64_t* d_out_off,
                               uint8_t* d_out_bytes, int64_t out_cap, int64_t* out_nbytes, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (row0 < 0 || n_rows < 0) return set_err(LDDL_EINVAL, "negative row range");
  if (hdr_len <= 0 || (hdr_len & 1) || kmax < 0) return set_err(LDDL_EINVAL, "header length %d must be even and > 0", hdr_len);
  if (!d_out_off || !out_nbytes || (n_rows > 0 && (!d_mlm_off || !d_hdr))) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  NpyParams N{};
  N.moff = d_mlm_off;
  N.mpos = d_mlm_pos;
  N.row0 = row0;
  N.n_rows = n_rows;
  N.hdr = d_hdr;
  N.hdr_u16 = hdr_len / 2;
  N.kmax = kmax;
  int rc;
  uint32_t e;
  if ((rc = ws_get(c, CW_NPY_ERR, 1, &N.err))) return rc;
  if ((rc = render_total(c, N, launch_npy_len, d_out_off, st, N.err, &e))) return rc;
  if (e) return set_err(LDDL_EINVAL, "a row has more than kmax = %d masked positions", kmax);
  if ((rc = render_room(c, d_out_bytes, out_cap, out_nbytes)) <= 0) return rc;
  if (n_rows > 0 && *out_nbytes > 2 * (int64_t)N.hdr_u16 * n_rows && !d_mlm_pos) return set_err(LDDL_EINVAL, "null pointer");
  N.out_off = d_out_off;
  N.out = d_out_bytes;
  HIP_TRY(launch_npy_bytes(N, c->n_cu, st));
  return 0;
}

extern "C" int lddl_render_masked(lddl_ctx* c, const uint16_t* d_ids, const int64_t* d_src, const uint16_t* d_len,
                                  const uint16_t* d_len0, int32_t segment, const int64_t* d_mlm_off,
                                  const uint16_t* d_mlm_pos, const uint16_t* d_mlm_token, int64_t row0, int64_t n_rows,
                                  int64_t* d_out_off, uint8_t* d_out_bytes, int64_t out_cap, int64_t* out_nbytes,
                                  void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (segment != 0 && segment != 1) return set_err(LDDL_EINVAL, "segment %d not 0 / 1", segment);
  if (row0 < 0 || n_rows < 0) return set_err(LDDL_EINVAL, "negative row range");
  if (!d_ids || !d_src || !d_len || !d_len0 || !d_mlm_off || !d_mlm_pos || !d_mlm_token || !d_out_off || !out_nbytes)
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  RenderParams R{};
  R.tokens = d_ids;
  R.row_off = d_src;
  R.len0 = d_len;
  R.row0 = row0;
  R.n_rows = n_rows;
  R.segment = RENDER_SPAN;
  R.vinfo = c->d_rinfo;
  R.vpool = c->d_rpool;
  R.moff = d_mlm_off;
  R.mpos = d_mlm_pos;
  R.mtok = d_mlm_token;
  R.len0m = d_len0;
  R.mseg = segment;
  return render_tail(c, R, d_out_off, d_out_bytes, out_cap, out_nbytes, (hipStream_t)stream);
}
