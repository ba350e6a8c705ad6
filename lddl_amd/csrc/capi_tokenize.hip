// C-ABI, host side of lddl_tokenize (kernels: tokenize_split.hip, tokenize_fallback.hip).
#include "capi_ctx.h"

// LDDL_TOK_DEBUG=1: the counters of P.dbg on stderr
static int tok_debug_report(const TokParams& P, int64_t nt, hipStream_t st) {
  uint64_t h[24];
  HIP_TRY(hipMemcpyAsync(h, P.dbg, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const char* nm[12] = {"loop", "setup", "classify", "except", "units", "urec", "prep", "probe", "records",
                        "tile_end", "entries", "tiles"};
  fprintf(stderr, "[lddl tok5 dbg] ntiles=%lld", (long long)nt);
  for (int k = 0; k < 12; ++k) fprintf(stderr, " %s=%llu", nm[k], (unsigned long long)h[k]);
  const char* wn[6] = {"wp_A", "wp_B", "wp_C", "wp_D", "wp_steps", "wp_lane_steps"};
  for (int k = 0; k < 6; ++k) fprintf(stderr, " %s=%llu", wn[k], (unsigned long long)h[12 + k]);
  fprintf(stderr, " prep_decode=%llu prep_dirty=%llu x_list=%llu x_load=%llu x_apply=%llu", (unsigned long long)h[18],
          (unsigned long long)h[19], (unsigned long long)h[20], (unsigned long long)h[21], (unsigned long long)h[22]);
  fprintf(stderr, "\n");
  return 0;
}

extern "C" int lddl_tokenize(lddl_ctx* c, const uint8_t* d_bytes, int64_t nbytes, const int64_t* d_sent_off,
                             int64_t n_sent, int32_t max_tok, uint16_t* d_out_ids, int64_t out_cap,
                             int32_t* d_out_ntok, int64_t* d_out_tok_off, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n_sent < 0 || max_tok < 1 || max_tok > 65534 || nbytes < 0 || out_cap < 0)
    return set_err(LDDL_EINVAL, "n_sent %lld nbytes %lld max_tok %d out_cap %lld", (long long)n_sent,
                   (long long)nbytes, max_tok, (long long)out_cap);
  if (!d_out_tok_off) return set_err(LDDL_EINVAL, "null device pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (n_sent == 0) {
    HIP_TRY(hipMemsetAsync(d_out_tok_off, 0, sizeof(int64_t), st));
    return 0;
  }
  if (!d_bytes || !d_sent_off || (!d_out_ids && out_cap > 0) || !d_out_ntok)
    return set_err(LDDL_EINVAL, "null device pointer");
  TokParams P{};
  P.bytes = d_bytes;
  P.sent_off = d_sent_off;
  P.n_sent = n_sent;
  P.max_tok = max_tok;
  P.out_ids = d_out_ids;
  P.out_ntok = d_out_ntok;
  P.out_tok_off = d_out_tok_off;
  P.out_cap = out_cap;
  c->spec_ids = nullptr;
  if (c->spec_flags) {
    int rc;
    if ((rc = ws_get(c, CW_SENT_SPEC, n_sent, &P.sent_spec))) return rc;
    c->spec_ids = d_out_ids;
    c->spec_ntok = d_out_ntok;
    c->spec_soff = d_sent_off;
    c->spec_nsent = n_sent;
  }
  P.top = c->d_top;
  P.pages = c->d_pages;
  P.bmp = c->d_bmp;
  P.xmap = c->d_xmap;
  P.multi = c->d_multi;
  P.slots = c->d_slots;
  P.slot_mask = c->slot_mask;
  P.bloom = c->d_bloom;
  P.pool = c->d_pool;
  P.voff = c->d_voff;
  P.maxb[0] = c->maxb[0];
  P.maxb[1] = c->maxb[1];
  for (int k = 0; k < 5; ++k) P.special[k] = c->special[k];
  P.unk = c->special[1];
  P.vt = c->d_vt;
  P.vt_mask = c->vt_mask;
  P.vbloom = c->d_vbloom;
  P.ovf = c->d_ovf;
  P.work_counter = c->d_counter;
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, 64, st));
  const char* dbgenv = getenv("LDDL_TOK_DEBUG");

  if (dbgenv && dbgenv[0] == '1') {
    if (!c->d_tdbg) HIP_TRY(hipMalloc((void**)&c->d_tdbg, 32 * 8));
    HIP_TRY(hipMemsetAsync(c->d_tdbg, 0, 32 * 8, st));
    P.dbg = c->d_tdbg;
  }
  const int64_t nt = tile_count(nbytes);
  // LDDL_SPLIT_SEG (tiles per segment) / LDDL_SPLIT_CHUNKS (record chunks):
  // tests force segment seams and record-capacity fallbacks at small sizes.
  // The serial path (tok_algo 0) is one segment of fallback tiles.
  const char* eseg = getenv("LDDL_SPLIT_SEG");
  const char* ech = getenv("LDDL_SPLIT_CHUNKS");
  const int64_t seg_max = c->tok_algo == 0 ? nt : eseg && atoll(eseg) > 0 ? atoll(eseg) : SPLIT_SEG_TILES;
  const int64_t seg = nt < seg_max ? nt : seg_max;
  const bool split = c->tok_algo == 5;
  int64_t n_chunks = !split ? 1 : split_seg_slots(seg, c->n_cu) / SPLIT_CHUNK;
  if (ech && atoll(ech) > 0 && split) n_chunks = atoll(ech);
  const int64_t slots = n_chunks * SPLIT_CHUNK;
  int64_t* tile_sent;
  SplitParams S{};
  int rc;
  const int64_t fb_cap = fb_list_cap(seg, n_sent);  // sentence ranges, two int64 each
  // (the entry / staging buffer: u16 per byte of a segment + the last
  // sentence's ids past its end)
  if ((rc = ws_get(c, CW_TILE_SENT, nt + 1, &tile_sent)) || (rc = ws_get(c, CW_FB_LIST, (size_t)(2 * fb_cap), &S.fb_list)) ||
      (rc = ws_get(c, CW_FB_COUNT, 16, &S.fb_count)) ||
      (rc = ws_get(c, CW_ENT, (size_t)seg * 1024 + (size_t)max_tok + 4096, &S.ent)) ||
      (rc = ws_get(c, CW_SHARED_BSUM, (size_t)n_chunks + 16, &S.chunk_fill)) ||
      (rc = ws_get(c, CW_SCAN_BSUM, (size_t)scan_blocks(n_sent) + 1, &S.scan_bsum)))
    return rc;
  // (the serial path (0) runs the split path's finish: count / expand read
  // smeta, snslot, cnt8 and, unconditionally, pch[0] -- one chunk of them)
  if ((rc = ws_get(c, CW_SHARED_ROWS, (size_t)slots * 4, &S.rec)) || (rc = ws_get(c, CW_PCS, (size_t)slots * 4, &S.pcs)) ||
      (rc = ws_get(c, CW_PCH, (size_t)slots, &S.pch)) || (rc = ws_get(c, CW_SHARED_META, n_sent, &S.smeta)) ||
      (rc = ws_get(c, CW_SNSLOT, n_sent, &S.snslot)) || (rc = ws_get(c, CW_CNT8, (size_t)slots, &S.cnt8)))
    return rc;
  // (the finish pass -- count_kernel and expand_kernel -- reads these
  // unconditionally: refuse to run it without them)
  if (!S.pch || !S.smeta || !S.snslot || !S.cnt8 || !S.rec || !S.pcs)
    return set_err(LDDL_EINVAL, "tokenize: finish scratch not allocated");
  S.chunk_ctr = S.chunk_fill + n_chunks;
  S.n_chunks = (uint32_t)n_chunks;
  S.seg_tiles = seg;
  S.fb_cap = fb_cap;
  S.seg_sent_cap = n_sent;
  S.n_fallback = c->d_counter + 8;
  if (c->timing) {
    S.n_rec = c->d_nrec;
    HIP_TRY(hipMemsetAsync(c->d_nrec, 0, 8, st));
  }
  if (c->tok_algo == 0) {
    HIP_TRY(launch_tokenize_serial_dense(P, nbytes, tile_sent, S, c->n_cu, c->tok_grid, st));
  } else {
    HIP_TRY(launch_tokenize_split(P, nbytes, tile_sent, S, c->n_cu, c->tok_grid, st,
                                  c->timing ? c->tm : nullptr));
  }
  if (P.dbg) return tok_debug_report(P, nt, st);
  return 0;
}
