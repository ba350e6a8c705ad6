// C-ABI of liblddl_amd.so: the drop-in boundary (declared in include/lddl_amd.h).
// Plain pointers and sizes only; device pointers come from the caller
// (torch tensors via data_ptr(), or hipMalloc).  Every entry point returns 0
// on success and a negative LDDL_E* code on failure; the message is kept in
// a thread-local buffer readable with lddl_last_error().  Nothing aborts.
// Here: the ctx's life, its vocabulary and its switches; the calls that launch work are in
// capi_tokenize / capi_pack / capi_render / capi_collate.hip, what they share in capi_ctx.h.
#include "capi_ctx.h"

static thread_local char g_err[1024];

int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* lddl_last_error(void) { return g_err; }

static void free_ctx(lddl_ctx* c) {
  if (!c) return;
  (void)hipFree(c->d_tdbg);
  (void)hipFree(c->d_pdbg);
  (void)hipFree(c->d_top);
  (void)hipFree(c->d_pages);
  (void)hipFree(c->d_bmp);
  (void)hipFree(c->d_xmap);
  (void)hipFree(c->d_multi);
  (void)hipFree(c->d_slots);
  (void)hipFree(c->d_bloom);
  (void)hipFree(c->d_pool);
  (void)hipFree(c->d_voff);
  (void)hipFree(c->d_rpool);
  (void)hipFree(c->d_rinfo);
  (void)hipFree(c->d_cont);
  (void)hipFree(c->d_vt);
  (void)hipFree(c->d_vbloom);
  (void)hipFree(c->d_ovf);
  (void)hipFree(c->d_counter);
  (void)hipFree(c->d_ctab);
  (void)hipFree(c->d_split_props);
  (void)hipFree(c->d_nrec);
  if (c->tm) {
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 64; ++i) (void)hipEventDestroy(c->tm->ev[k][j][i]);
    delete c->tm;
  }
  for (auto& b : c->ws) (void)hipFree(b.p);
  free_pack(&c->own);
  if (c->h_tot) (void)hipHostFree(c->h_tot);
  delete c;
}

extern "C" void lddl_destroy(lddl_ctx* c) {
  if (c) (void)hipSetDevice(c->device);
  free_ctx(c);
}

static int load_table(lddl_ctx* c, const char* path) {
  UniTables T;
  std::string err;
  int rc = build_uni_tables(path, T, err);
  if (rc) return set_err(rc, "%s", err.c_str());
  c->scan_ok = T.scan_ok;
  if ((rc = upload(&c->d_top, T.top.data(), T.top.size() * 2))) return rc;
  if ((rc = upload(&c->d_pages, T.pages.data(), T.pages.size() * 4))) return rc;
  if ((rc = upload(&c->d_multi, T.multi.data(), T.multi.size() * 4))) return rc;
  if ((rc = upload(&c->d_bmp, T.bmp.data(), T.bmp.size() * 4))) return rc;
  if ((rc = upload(&c->d_xmap, T.xmap.data(), T.xmap.size() * 4))) return rc;
  return 0;
}

static int load_vocab(lddl_ctx* c, const char* path) {
  VocabTables V;
  std::string err;
  int rc = build_vocab_tables(path, V, err);
  if (rc) return set_err(rc, "%s", err.c_str());
  c->vocab_size = (int)V.vocab.size();
  for (int k = 0; k < 5; ++k) c->special[k] = V.special[k];
  c->maxb[0] = V.maxb[0];
  c->maxb[1] = V.maxb[1];
  c->slot_mask = V.slot_mask;
  c->vt_mask = V.vt_mask;
  if ((rc = upload(&c->d_bloom, V.bloom.data(), V.bloom.size() * 4))) return rc;
  if ((rc = upload(&c->d_vt, V.vt.data(), V.vt.size() * 4))) return rc;
  if ((rc = upload(&c->d_vbloom, V.vbloom.data(), V.vbloom.size() * 4))) return rc;
  if ((rc = upload(&c->d_slots, V.slots.data(), V.slots.size() * sizeof(uint4)))) return rc;
  if ((rc = upload(&c->d_pool, V.pool.data(), V.pool.size()))) return rc;
  if ((rc = upload(&c->d_voff, V.voff.data(), V.voff.size() * 4))) return rc;
  if ((rc = upload(&c->d_rpool, V.rpool.data(), V.rpool.size()))) return rc;
  if ((rc = upload(&c->d_rinfo, V.rinfo.data(), V.rinfo.size() * 4))) return rc;
  std::vector<uint32_t> cont((V.vocab.size() + 31) / 32, 0u);
  for (size_t i = 0; i < V.vocab.size(); ++i)
    if (V.vocab[i].compare(0, 2, "##") == 0) cont[i >> 5] |= 1u << (i & 31);
  if ((rc = upload(&c->d_cont, cont.data(), cont.size() * 4))) return rc;
  c->vocab = std::move(V.vocab);
  return 0;
}

// the tokenizer algorithm: the one asked for, or the serial path (0) when it
// does not model the loaded tables (the split tokenizer keeps ids below
// SPLIT_EDEF and derives its byte classes from the ASCII page)
static void select_tok_algo(lddl_ctx* c, int algo) {
  c->tok_algo = algo;
  if (c->tok_algo == 5 && (!c->scan_ok || c->vocab_size > (int)SPLIT_EDEF)) c->tok_algo = 0;
}

extern "C" int lddl_create(const char* vocab_path, const char* table_path, int device, lddl_ctx** out) {
  if (!out || !vocab_path || !table_path) return set_err(LDDL_EINVAL, "null argument");
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return set_err(LDDL_EINVAL, "device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  lddl_ctx* c = new lddl_ctx();
  c->device = device;
  int rc = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) { free_ctx(c); return set_err(LDDL_EHIP, "hipGetDeviceProperties"); }
  c->n_cu = prop.multiProcessorCount;
  if ((rc = load_table(c, table_path)) || (rc = load_vocab(c, vocab_path))) { free_ctx(c); return rc; }
  // 5: the split tokenizer (default); 0: every tile through the exact serial
  // path -- LDDL_TOKENIZE_ALGO selects (tests); select_tok_algo falls back to
  // 0 for tables the split tokenizer does not model
  const char* algo = getenv("LDDL_TOKENIZE_ALGO");
  select_tok_algo(c, algo && algo[0] == '0' ? 0 : 5);
  const char* mcap = getenv("LDDL_MLM_CAP");  // initial masking arena (tests force the regrow path)
  c->mlm_cap0 = mcap ? (uint64_t)atoll(mcap) : 0;
  c->own.device = device;
  c->own.mlm_cap = c->mlm_cap0;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tokenize_fallback_kernel_ptr(), 256, 0) != hipSuccess ||
      per_cu < 1)
    per_cu = 4;
  c->tok_grid = c->n_cu * per_cu;
  const size_t ovf_bytes = (size_t)c->tok_grid * 256 * WB_OVF;
  if (hipMalloc((void**)&c->d_ovf, ovf_bytes) != hipSuccess ||
      hipMalloc((void**)&c->d_counter, 64) != hipSuccess ||
      hipHostMalloc((void**)&c->h_tot, HW_COUNT * sizeof(int64_t)) != hipSuccess) {
    free_ctx(c);
    return set_err(LDDL_ENOMEM, "scratch allocation failed");
  }
  *out = c;
  return 0;
}

extern "C" int lddl_vocab_size(const lddl_ctx* c) { return c ? c->vocab_size : set_err(LDDL_EINVAL, "null ctx"); }

extern "C" int lddl_special_ids(const lddl_ctx* c, int32_t out[5]) {
  if (!c || !out) return set_err(LDDL_EINVAL, "null argument");
  for (int k = 0; k < 5; ++k) out[k] = (int32_t)c->special[k];
  return 0;
}

extern "C" int lddl_vocab_token(const lddl_ctx* c, int32_t id, char* buf, int64_t cap) {
  if (!c || !buf) return set_err(LDDL_EINVAL, "null argument");
  if (id < 0 || id >= c->vocab_size) return set_err(LDDL_EINVAL, "id %d out of range", id);
  const std::string& w = c->vocab[id];
  if ((int64_t)w.size() + 1 > cap) return set_err(LDDL_EINVAL, "buffer too small");
  memcpy(buf, w.data(), w.size());
  buf[w.size()] = 0;
  return (int)w.size();
}

extern "C" int lddl_set_special_flags(lddl_ctx* c, int on) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  c->spec_flags = on != 0;
  return 0;
}

extern "C" int lddl_set_whole_word_mask(lddl_ctx* c, int on) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  c->whole_word = on != 0;
  return 0;
}

extern "C" int lddl_set_span_mask(lddl_ctx* c, int32_t max_span, double geo_p) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (max_span == 0) {
    c->span_max = 0;
    return 0;
  }
  // the ranges are lddl_span_params': nothing is kept that a collate call would refuse later
  double q, cdf[16];
  const int rc = lddl_span_params(max_span, geo_p, 0.0, &q, cdf);
  if (rc) return rc;
  c->span_max = max_span;
  c->span_geo = geo_p;
  return 0;
}

extern "C" int lddl_set_tokenize_algo(lddl_ctx* c, int algo, int* out_algo) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (algo != 0 && algo != 5) return set_err(LDDL_EINVAL, "tokenize algo must be 0 or 5");
  select_tok_algo(c, algo);
  if (out_algo) *out_algo = c->tok_algo;
  return 0;
}

extern "C" int lddl_set_timing(lddl_ctx* c, int on) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  HIP_TRY(hipSetDevice(c->device));
  if (on && !c->tm) {
    c->tm = new SplitTiming();
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 64; ++i) HIP_TRY(hipEventCreate(&c->tm->ev[k][j][i]));
    HIP_TRY(hipMalloc((void**)&c->d_nrec, 16));
  }
  c->timing = on != 0;
  return 0;
}

extern "C" int lddl_tokenize_stats(lddl_ctx* c, double* out, int n) {
  if (!c || !out || n < 6) return set_err(LDDL_EINVAL, "need out[6]");
  if (!c->timing || !c->tm) return set_err(LDDL_EINVAL, "timing is off (lddl_set_timing)");
  HIP_TRY(hipSetDevice(c->device));
  for (int k = 0; k < 3; ++k) {
    double ms = 0.0;
    for (int i = 0; i < c->tm->n[k]; ++i) {
      HIP_TRY(hipEventSynchronize(c->tm->ev[k][1][i]));
      float f = 0.0f;
      HIP_TRY(hipEventElapsedTime(&f, c->tm->ev[k][0][i], c->tm->ev[k][1][i]));
      ms += f;
    }
    out[k] = ms;
  }
  unsigned long long nrec = 0;
  HIP_TRY(hipMemcpy(&nrec, c->d_nrec, 8, hipMemcpyDeviceToHost));
  out[3] = (double)nrec;
  out[4] = (double)c->tm->n[0];
  uint32_t nfb = 0;
  HIP_TRY(hipMemcpy(&nfb, c->d_counter + 8, 4, hipMemcpyDeviceToHost));
  out[5] = (double)nfb;
  return 0;
}
