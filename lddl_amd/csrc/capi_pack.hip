// C-ABI, host side of the packers, the calls that read a pack result and
// lddl_bin (kernels: pack.hip, pack_wave.hip, bin.hip; lddl_row_docs': render.hip).
#include "capi_ctx.h"

// The pack result a call works on: pk, or the ctx's own for callers that pass NULL.
// NULL: refused with LDDL_EINVAL, the message set.
static lddl_pack* pack_of(lddl_ctx* c, lddl_pack* pk) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx"), nullptr;
  lddl_pack* k = pk ? pk : &c->own;
  if (k->device != c->device) return set_err(LDDL_EINVAL, "pack result of another device"), nullptr;
  return k;
}

// LDDL_PACK_DEBUG=1, the BERT packer: the phase ticks of P.dbg and the waves' occupancy timeline on stderr
static int pack_debug_report(const PackParams& P, int64_t n_part, hipStream_t st) {
  uint64_t h[16];
  HIP_TRY(hipMemcpyAsync(h, P.dbg, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const char* nm[16] = {"filter", "ldsfill", "seed", "generate", "shuffle", "bin", "pairs", "parts",
                        "m_cand", "m_draws", "m_trace", "m_choices", "m_write", "m_trace_fbuild", "m_trace_chains",
                        "unused"};
  const char* gn[5] = {"g_doc", "g_fill", "g_pairB", "g_trunc", "g_store"};  // unmasked: generate sub-phases
  fprintf(stderr, "[lddl pack dbg]");
  for (int k = 0; k < (P.masking ? 15 : 13); ++k)
    fprintf(stderr, " %s=%llu", k < 8 || P.masking ? nm[k] : gn[k - 8], (unsigned long long)h[k]);
  fprintf(stderr, "\n");
  // occupancy timeline (100 MHz ticks): the span from the first wave's
  // start to the last one's end, the summed wave time, the most waves
  // resident at once, and how long the residency stays below 90 % / 50 %
  // of that maximum after the peak (the tail)
  std::vector<uint64_t> tl(2 * (size_t)n_part);
  HIP_TRY(hipMemcpyAsync(tl.data(), P.dbg + 16, tl.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  std::vector<std::pair<uint64_t, int>> ev;
  ev.reserve(tl.size());
  uint64_t busy = 0, t_lo = ~0ull, t_hi = 0;
  for (int64_t q = 0; q < n_part; ++q) {
    const uint64_t a = tl[2 * q], b = tl[2 * q + 1];
    if (b < a || a == 0) continue;
    ev.push_back({a, 1});
    ev.push_back({b, -1});
    busy += b - a;
    t_lo = std::min(t_lo, a);
    t_hi = std::max(t_hi, b);
  }
  std::sort(ev.begin(), ev.end());
  int cur = 0, mx = 0;
  uint64_t t_peak = t_lo;
  for (auto& e : ev) {
    cur += e.second;
    if (cur > mx) { mx = cur; t_peak = e.first; }
  }
  uint64_t below90 = 0, below50 = 0, prev = t_lo;
  cur = 0;
  for (auto& e : ev) {
    if (e.first > t_peak) {
      if (cur < 0.9 * mx) below90 += e.first - prev;
      if (cur < 0.5 * mx) below50 += e.first - prev;
    }
    prev = e.first;
    cur += e.second;
  }
  std::vector<uint64_t> du;
  uint64_t last_start = 0;
  for (int64_t q = 0; q < n_part; ++q)
    if (tl[2 * q] && tl[2 * q + 1] >= tl[2 * q]) {
      du.push_back(tl[2 * q + 1] - tl[2 * q]);
      last_start = std::max(last_start, tl[2 * q] - t_lo);
    }
  std::sort(du.begin(), du.end());
  auto pct = [&](double f) { return du.empty() ? 0.0 : du[std::min(du.size() - 1, (size_t)(f * du.size()))] / 100.0; };
  fprintf(stderr, "[lddl pack tl] wave_us p10=%.0f p50=%.0f p90=%.0f max=%.0f last_start_us=%.0f\n", pct(0.1), pct(0.5),
          pct(0.9), pct(1.0), last_start / 100.0);
  fprintf(stderr, "[lddl pack tl] waves=%zu span_us=%.0f busy_wave_us=%.0f max_resident=%d mean_resident=%.0f tail_below90_us=%.0f tail_below50_us=%.0f mean_wave_us=%.0f\n",
          ev.size() / 2, (t_hi - t_lo) / 100.0, busy / 100.0, mx, t_hi > t_lo ? (double)busy / (double)(t_hi - t_lo) : 0.0,
          below90 / 100.0, below50 / 100.0, ev.empty() ? 0.0 : busy / 100.0 / (ev.size() / 2));
  return 0;
}

// which packer a pack call runs (pack_common)
enum PackKind { PACK_BERT = 0, PACK_CODEBERT = 1, PACK_MLM = 2, PACK_SOP = 3 };

static int pack_common(lddl_ctx* c, lddl_pack* pk, PackKind kind, const int32_t* d_ntok, const int64_t* d_tok_off,
                       const int64_t* d_sent_off, int64_t n_sent,
                       const int64_t* d_doc_sent_off, const int32_t* d_doc_nseg_doc, int64_t n_doc,
                       const int64_t* d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                       double short_seq_prob, int32_t duplicate_factor, uint64_t seed, int32_t bin_size,
                       int64_t* out_totals, void* stream, const uint16_t* d_ids = nullptr, int32_t masking = 0,
                       double masked_lm_ratio = 0.15) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (masking) {
    if (!d_ids) return set_err(LDDL_EINVAL, "masking needs the tokenizer ids");
    if (target_seq_length > MLM_MAX_SEQ)
      return set_err(LDDL_EINVAL, "masking supports target_seq_length <= %d", MLM_MAX_SEQ);
    if (!(masked_lm_ratio >= 0.0 && masked_lm_ratio <= 1.0))
      return set_err(LDDL_EINVAL, "masked_lm_ratio %g not in [0, 1]", masked_lm_ratio);
    if (c->vocab_size > 65535) return set_err(LDDL_EINVAL, "masking: vocab larger than 65535");
  }
  if (n_part < 1 || n_doc < 0 || n_sent < 0) return set_err(LDDL_EINVAL, "bad sizes");
  if (!d_ntok || !d_tok_off || !d_sent_off || !d_doc_sent_off || !d_part_doc_off || !out_totals)
    return set_err(LDDL_EINVAL, "null pointer");
  if (kind == PACK_CODEBERT && !d_doc_nseg_doc) return set_err(LDDL_EINVAL, "codebert needs doc_nseg_doc");
  if (target_seq_length < 5 || target_seq_length > 32768)
    return set_err(LDDL_EINVAL, "target_seq_length %d not in [5, 32768]", target_seq_length);
  if (duplicate_factor < 1) return set_err(LDDL_EINVAL, "duplicate_factor %d < 1", duplicate_factor);
  int32_t nbins = 1;
  if (bin_size > 0) {
    // pretrain.py:566-571
    if (bin_size > target_seq_length) return set_err(LDDL_EINVAL, "bin size must be <= target-seq-length");
    if (target_seq_length % bin_size) return set_err(LDDL_EINVAL, "bin size must divide target-seq-length");
    nbins = target_seq_length / bin_size;
  } else {
    bin_size = 1 << 30;
  }
  if (nbins > 255) return set_err(LDDL_EINVAL, "more than 255 bins");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  k->last_npairs = -1;  // until this pack succeeds, nothing to materialise
  k->last_nmask = -1;
  k->last_tokens = nullptr;
  PackParams& P = k->pp;
  P = PackParams{};
  P.ntok = d_ntok;
  P.sent_off = d_sent_off;
  P.doc_sent_off = d_doc_sent_off;
  P.part_doc_off = d_part_doc_off;
  P.doc_nseg_doc = d_doc_nseg_doc;
  P.n_part = n_part;
  P.max_seq = target_seq_length;
  P.dup = duplicate_factor;
  P.short_seq_prob = short_seq_prob;
  P.seed = seed;
  P.bin_size = bin_size;
  P.nbins = nbins;
  const size_t npair_cap = (size_t)duplicate_factor * (size_t)(n_sent ? n_sent : 1);
  int rc;
  if ((rc = ws_get(k->ws, PW_FS_NTOK, n_sent, &P.fs_ntok)) || (rc = ws_get(k->ws, PW_FS_BASE, n_sent, &P.fs_base)) ||
      (rc = ws_get(k->ws, PW_FD_FIRST, n_doc, &P.fd_first)) || (rc = ws_get(k->ws, PW_FD_N, n_doc, &P.fd_n)) ||
      (rc = ws_get(k->ws, PW_FD_ND, n_doc, &P.fd_nd)) ||
      (rc = ws_get(k->ws, PW_PAIRS, npair_cap, &P.pairs)) || (rc = ws_get(k->ws, PW_ORDER, npair_cap, &P.order)) ||
      (rc = ws_get(k->ws, PW_BINNED, npair_cap, &P.binned)) || (rc = ws_get(k->ws, PW_TOK_LOCAL, npair_cap, &P.tok_local)) ||
      (rc = ws_get(k->ws, PW_PART_NPAIRS, n_part, &P.part_npairs)) || (rc = ws_get(k->ws, PW_PART_NTOK, n_part, &P.part_ntok)) ||
      (rc = ws_get(k->ws, PW_BIN_COUNT, (size_t)n_part * nbins, &P.bin_count)) ||
      (rc = ws_get(k->ws, PW_BIN_CURSOR, (size_t)n_part * nbins, &P.bin_cursor)) ||
      (rc = ws_get(k->ws, PW_PART_ERR, n_part, &P.part_err)) || (rc = ws_get(k->ws, PW_KEPT, n_sent + n_part + 1, &P.kept)) ||
      (rc = ws_get(k->ws, PW_FS_DENSE, n_sent, &P.fs_dense)) || (rc = ws_get(k->ws, PW_SPAN, npair_cap, &P.span)))
    return rc;
  {
    uint32_t* mts;
    if ((rc = ws_get(k->ws, PW_MT_STATES, (size_t)((n_part + 63) & ~(int64_t)63) * MT_N, &mts))) return rc;  // (whole 64-partition rows)
    HIP_TRY(launch_mt_seed_states(seed, n_part, mts, st));
    P.mt_states = mts;
  }
  P.tokoff = d_tok_off;  // the tokenizer's dense offsets (lddl_tokenize d_out_tok_off)
  int64_t *pair_base, *tok_base;
  int32_t* err_any;
  if ((rc = ws_get(k->ws, PW_PAIR_BASE, n_part + 1, &pair_base)) || (rc = ws_get(k->ws, PW_TOK_BASE, n_part + 1, &tok_base)) ||
      (rc = ws_get(k->ws, PW_ERR_ANY, 4, &err_any)))
    return rc;
  int64_t *mask_base = nullptr, *mask_base2 = nullptr;
  if (masking) {
    P.masking = 1;
    P.mlm_ratio = masked_lm_ratio;
    P.n_vocab = (uint32_t)c->vocab_size;
    P.cls_id = c->special[2];
    P.sep_id = c->special[3];
    P.mask_id = c->special[4];
    P.ids = d_ids;
    uint8_t *sent_spec, *fs_spec;
    // the flags of the last lddl_tokenize into these buffers, else a pass over the ids
    // (one pack consumes them: a later pack over recycled buffers at the same
    // addresses recomputes the flags from the ids)
    const bool spec_ok = c->spec_ids == d_ids && c->spec_ntok == d_ntok && c->spec_soff == d_sent_off &&
                         c->spec_nsent == n_sent;
    c->spec_ids = nullptr;
    if ((rc = spec_ok ? ws_get(c->ws, CW_SENT_SPEC, n_sent, &sent_spec) : ws_get(k->ws, PW_SENT_SPEC, n_sent, &sent_spec)) ||
        (rc = ws_get(k->ws, PW_FS_SPEC, n_sent, &fs_spec)) ||
        (rc = ws_get(k->ws, PW_MREF, npair_cap, &P.mref)) || (rc = ws_get(k->ws, PW_MLOC, npair_cap, &P.mloc)) ||
        (rc = ws_get(k->ws, PW_PART_NMASK, n_part, &P.part_nmask)) || (rc = ws_get(k->ws, PW_MASK_BASE, n_part + 1, &mask_base)) ||
        (rc = ws_get(k->ws, PW_MASK_BASE2, n_part + 1, &mask_base2)) || (rc = ws_get(k->ws, PW_MCOUNTER, 1, &P.mcounter)) ||
        (rc = ws_get(k->ws, PW_MCAND, (size_t)n_part * MLM_MAX_SEQ, &P.mcand)))
      return rc;
    P.sent_spec = sent_spec;
    P.fs_spec = fs_spec;
    if (!spec_ok) HIP_TRY(launch_sent_special(d_ids, d_tok_off, d_ntok, n_sent, P.cls_id, P.sep_id, sent_spec, st));
    if (!k->mlm_cap) k->mlm_cap = (uint64_t)n_part * 4 * MLM_CHUNK + (uint64_t)duplicate_factor * n_sent * 4;
  }
  if (kind == PACK_BERT) {
    // Wave packer: one 64-lane workgroup per partition runs a serial chain, so
    // throughput is partitions in flight; measured on the bench workload the
    // per-partition arrays are best left in global memory (L2), keeping the
    // workgroup at ~5 KiB of LDS (~30 partitions per CU): 65 ms against 250 ms
    // with 4 partitions per CU.  LDDL_PACK_CAPS=lens,docs,pairs puts them in LDS.
    P.cap_lens = 0;
    P.cap_docs = 0;
    P.cap_pairs = 0;
    const char* caps = getenv("LDDL_PACK_CAPS");  // "lens,docs,pairs" override (tuning)
    if (caps) {
      int a = 0, b = 0, d = 0;
      if (sscanf(caps, "%d,%d,%d", &a, &b, &d) == 3) {
        P.cap_lens = a / 64 * 64;
        P.cap_docs = b / 64 * 64;
        P.cap_pairs = std::min(d / 64 * 64, 65472);
      }
    }
  }
  for (int attempt = 0;; ++attempt) {
    if (masking) {
      if ((rc = ws_get(k->ws, PW_MARENA, k->mlm_cap, &P.marena))) return rc;
      P.mcap = k->mlm_cap;
      HIP_TRY(hipMemsetAsync(P.mcounter, 0, 8, st));
    }
    const char* pdbg = getenv("LDDL_PACK_DEBUG");
    P.dbg = nullptr;
    const int64_t pdbg_n = 16 + 2 * (int64_t)n_part;  // counters + the BERT packer's per-wave start / end
    if (pdbg && pdbg[0] == '1') {
      if (c->pdbg_cap < pdbg_n) {
        (void)hipFree(c->d_pdbg);
        c->d_pdbg = nullptr;
        c->pdbg_cap = 0;
        HIP_TRY(hipMalloc((void**)&c->d_pdbg, pdbg_n * 8));
        c->pdbg_cap = pdbg_n;
      }
      HIP_TRY(hipMemsetAsync(c->d_pdbg, 0, pdbg_n * 8, st));
      P.dbg = c->d_pdbg;
    }
    HIP_TRY(kind == PACK_CODEBERT ? launch_pack_codebert_wave(P, st)
            : kind == PACK_MLM    ? launch_pack_mlm_wave(P, st)
            : kind == PACK_SOP    ? launch_pack_sop_wave(P, st)
                                  : launch_pack_bert_wave(P, st));
    if (P.dbg && kind == PACK_BERT && (rc = pack_debug_report(P, n_part, st))) return rc;
    HIP_TRY(launch_scan_parts(P.part_npairs, P.part_ntok, n_part, pair_base, tok_base, P.part_err, err_any, st));
    HIP_TRY(fetch_word(c, HW_NPAIRS, pair_base + n_part, 8, st));
    HIP_TRY(fetch_word(c, HW_NTOK, tok_base + n_part, 8, st));
    HIP_TRY(fetch_word(c, HW_PACK_ERR, err_any, 4, st));
    HIP_TRY(fetch_word(c, HW_NDENSE, P.tokoff + n_sent, 8, st));
    if (masking) {
      HIP_TRY(launch_scan_parts(P.part_nmask, P.part_nmask, n_part, mask_base, mask_base2, P.part_err, err_any, st));
      HIP_TRY(fetch_word(c, HW_NMASK, mask_base + n_part, 8, st));
      HIP_TRY(fetch_word(c, HW_MARENA_USED, P.mcounter, 8, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // the bump allocator overshot the arena: grow it and pack again (the
    // pack is deterministic, so the rerun reproduces the same rows)
    const uint64_t used = masking ? (uint64_t)c->h_tot[HW_MARENA_USED] : 0;
    if (used > k->mlm_cap && attempt == 0) {
      k->mlm_cap = used + (uint64_t)n_part * MLM_CHUNK;
      continue;
    }
    if (used > k->mlm_cap) return set_err(LDDL_ECAPACITY, "masking arena overflow");
    break;
  }
  const int32_t e = (int32_t)(c->h_tot[HW_PACK_ERR] & 0xFFFFFFFF);
  k->last_nmask = masking ? c->h_tot[HW_NMASK] : -1;
  if (e & PACK_EINDEX) { k->last_npairs = -1; return set_err(LDDL_EINDEX, "IndexError in _truncate_seq (reference quirk)"); }
  if (e & PACK_EASSERT) { k->last_npairs = -1; return set_err(LDDL_EASSERT, "AssertionError: empty segment after truncation"); }
  k->last_npairs = c->h_tot[HW_NPAIRS];
  k->last_ntok = c->h_tot[HW_NTOK];
  k->last_ndense = c->h_tot[HW_NDENSE];
  out_totals[0] = k->last_npairs;
  out_totals[1] = k->last_ntok;
  out_totals[2] = nbins;
  out_totals[3] = masking ? k->last_nmask : 0;
  return 0;
}

extern "C" int lddl_pack_bert(lddl_ctx* c, lddl_pack* pk, const uint16_t* d_ids, const int32_t* d_ntok, const int64_t* d_tok_off,
                              const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                              const int64_t* d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                              double short_seq_prob, int32_t duplicate_factor, int32_t masking,
                              double masked_lm_ratio, uint64_t seed, int32_t bin_size, int64_t* out_totals,
                              void* stream) {
  return pack_common(c, pk, PACK_BERT, d_ntok, d_tok_off, d_sent_off, n_sent, d_doc_sent_off, nullptr, n_doc, d_part_doc_off, n_part,
                     target_seq_length, short_seq_prob, duplicate_factor, seed, bin_size, out_totals, stream, d_ids,
                     masking, masked_lm_ratio);
}

extern "C" int lddl_pack_codebert(lddl_ctx* c, lddl_pack* pk, const int32_t* d_ntok, const int64_t* d_tok_off,
                                  const int64_t* d_sent_off, int64_t n_sent,
                                  const int64_t* d_doc_sent_off, const int32_t* d_doc_nseg_doc, int64_t n_doc,
                                  const int64_t* d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                                  double short_seq_prob, int32_t duplicate_factor, uint64_t seed, int32_t bin_size,
                                  int64_t* out_totals, void* stream) {
  return pack_common(c, pk, PACK_CODEBERT, d_ntok, d_tok_off, d_sent_off, n_sent, d_doc_sent_off, d_doc_nseg_doc, n_doc, d_part_doc_off,
                     n_part, target_seq_length, short_seq_prob, duplicate_factor, seed, bin_size, out_totals, stream);
}

extern "C" int lddl_pack_mlm(lddl_ctx* c, lddl_pack* pk, const int32_t* d_ntok, const int64_t* d_tok_off,
                             const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                             const int64_t* d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                             double short_seq_prob, int32_t duplicate_factor, uint64_t seed, int32_t bin_size,
                             int64_t* out_totals, void* stream) {
  return pack_common(c, pk, PACK_MLM, d_ntok, d_tok_off, d_sent_off, n_sent, d_doc_sent_off, nullptr, n_doc, d_part_doc_off,
                     n_part, target_seq_length, short_seq_prob, duplicate_factor, seed, bin_size, out_totals, stream);
}

extern "C" int lddl_pack_sop(lddl_ctx* c, lddl_pack* pk, const int32_t* d_ntok, const int64_t* d_tok_off,
                             const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                             const int64_t* d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                             double short_seq_prob, int32_t duplicate_factor, uint64_t seed, int32_t bin_size,
                             int64_t* out_totals, void* stream) {
  return pack_common(c, pk, PACK_SOP, d_ntok, d_tok_off, d_sent_off, n_sent, d_doc_sent_off, nullptr, n_doc, d_part_doc_off,
                     n_part, target_seq_length, short_seq_prob, duplicate_factor, seed, bin_size, out_totals, stream);
}

// The view of the last pack call's result that every call reading it works through
static PackView pack_view(const lddl_pack* k) {
  const PackParams& P = k->pp;
  PackView V{};
  V.pairs = P.pairs;
  V.binned = P.binned;
  V.tok_local = P.tok_local;
  V.pair_base = (const int64_t*)k->ws[PW_PAIR_BASE].p;
  V.tok_base = (const int64_t*)k->ws[PW_TOK_BASE].p;
  V.doc_sent_off = P.doc_sent_off;
  V.part_doc_off = P.part_doc_off;
  V.fs_dense = P.fs_dense;
  V.n_part = P.n_part;
  V.dup = P.dup;
  V.bin_size = P.bin_size;
  V.nbins = P.nbins;
  return V;
}

// MatParams of the last pack call with the per-row outputs both of its calls take (lddl_materialize / lddl_row_spans)
static MatParams mat_params(const lddl_ctx* c, const lddl_pack* k, int64_t* tok_off, uint16_t* len0, uint16_t* len1,
                            uint8_t* flags, uint8_t* bin, int64_t* part) {
  MatParams M{};
  M.V = pack_view(k);
  M.cls_id = c->special[2];
  M.sep_id = c->special[3];
  M.out_tok_off = tok_off;
  M.out_len0 = len0;
  M.out_len1 = len1;
  M.out_flags = flags;
  M.out_bin = bin;
  M.out_part = part;
  return M;
}

// MlmParams of the last masked pack call (lddl_masked_lm / lddl_masked_lm_spans)
static MlmParams mlm_params(const lddl_pack* k) {
  const PackParams& P = k->pp;
  MlmParams M{};
  M.V = pack_view(k);
  M.mref = P.mref;
  M.mloc = P.mloc;
  M.mask_base = (const int64_t*)k->ws[PW_MASK_BASE].p;
  M.marena = P.marena;
  return M;
}

extern "C" int lddl_materialize(lddl_ctx* c, lddl_pack* pk, const uint16_t* d_ids, uint16_t* d_out_tokens, int64_t* d_out_tok_off,
                                uint16_t* d_out_len0, uint16_t* d_out_len1, uint8_t* d_out_flags, uint8_t* d_out_bin,
                                int64_t* d_out_part, int64_t* d_bin_count, void* stream) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (k->last_npairs < 0) return set_err(LDDL_EINVAL, "no successful lddl_pack_* call to materialise");
  if (!d_ids || !d_out_tokens || !d_out_tok_off || !d_out_len0 || !d_out_len1 || !d_out_flags || !d_out_bin ||
      !d_out_part)
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const PackParams& P = k->pp;
  // LDDL_MAT_ALGO=1: the wave-per-partition materialize kernel (also taken
  // for unaligned buffers); otherwise the chunked v2 kernel
  const int mat_algo = getenv("LDDL_MAT_ALGO") ? atoi(getenv("LDDL_MAT_ALGO")) : 2;
  MatParams M = mat_params(c, k, d_out_tok_off, d_out_len0, d_out_len1, d_out_flags, d_out_bin, d_out_part);
  M.dense = d_ids;
  M.out_tokens = d_out_tokens;
  if (k->last_npairs == 0) {
    HIP_TRY(hipMemsetAsync(d_out_tok_off, 0, 8, st));
  } else {
    HIP_TRY(launch_materialize(M, k->last_npairs, k->last_ndense + 16, mat_algo, st));
  }
  if (d_bin_count)
    HIP_TRY(hipMemcpyAsync(d_bin_count, P.bin_count, (size_t)P.n_part * P.nbins * 8, hipMemcpyDeviceToDevice, st));
  k->last_tokens = d_out_tokens;
  k->last_tok_off = d_out_tok_off;
  k->last_part = d_out_part;
  return 0;
}

extern "C" int lddl_row_spans(lddl_ctx* c, lddl_pack* pk, int64_t* d_out_src0, int64_t* d_out_src1, int64_t* d_out_tok_off,
                              uint16_t* d_out_len0, uint16_t* d_out_len1, uint8_t* d_out_flags, uint8_t* d_out_bin,
                              int64_t* d_out_part, int64_t* d_bin_count, void* stream) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (k->last_npairs < 0) return set_err(LDDL_EINVAL, "no successful lddl_pack_* call");
  if (!d_out_src0 || !d_out_src1 || !d_out_len0 || !d_out_len1 || !d_out_flags || !d_out_bin || !d_out_part)
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const PackParams& P = k->pp;
  MatParams M = mat_params(c, k, d_out_tok_off, d_out_len0, d_out_len1, d_out_flags, d_out_bin, d_out_part);
  M.out_src0 = d_out_src0;
  M.out_src1 = d_out_src1;
  if (k->last_npairs == 0) {
    if (d_out_tok_off) HIP_TRY(hipMemsetAsync(d_out_tok_off, 0, 8, st));
  } else {
    int32_t* chunk_part = nullptr;
    int64_t* part_pb = nullptr;
    int rc;
    if ((rc =ws_get(c, CW_CHUNK_PART, (size_t)((k->last_npairs + 63) >> 6), &chunk_part)) ||
        (rc = ws_get(c, CW_PART_PB, (size_t)P.n_part, &part_pb)))
      return rc;
    HIP_TRY(launch_chunk_parts(M.V.pair_base, P.doc_sent_off, P.part_doc_off, P.dup, P.n_part, chunk_part, part_pb, st));
    M.span = P.span;
    M.chunk_part = chunk_part;
    M.part_pb = part_pb;
    HIP_TRY(launch_row_spans(M, k->last_npairs, st));
  }
  if (d_bin_count)
    HIP_TRY(hipMemcpyAsync(d_bin_count, P.bin_count, (size_t)P.n_part * P.nbins * 8, hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" int lddl_masked_lm(lddl_ctx* c, lddl_pack* pk, int64_t* d_out_mlm_off, uint16_t* d_out_mlm_pos, uint16_t* d_out_mlm_label,
                              void* stream) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (k->last_npairs < 0 || k->last_nmask < 0 || !k->last_tokens)
    return set_err(LDDL_EINVAL, "lddl_masked_lm needs lddl_pack_bert(masking=1) then lddl_materialize");
  if (!d_out_mlm_off || (k->last_nmask > 0 && (!d_out_mlm_pos || !d_out_mlm_label)))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (k->last_npairs == 0) {
    HIP_TRY(hipMemsetAsync(d_out_mlm_off, 0, 8, st));
  } else {
    MlmParams M = mlm_params(k);
    M.tokens = k->last_tokens;
    M.tok_off = k->last_tok_off;
    M.row_part = k->last_part;
    M.out_off = d_out_mlm_off;
    M.out_pos = d_out_mlm_pos;
    M.out_label = d_out_mlm_label;
    HIP_TRY(launch_masked_lm(M, k->last_npairs, st));
  }
  k->last_nmask = -1;  // the rows are masked in place exactly once
  return 0;
}

extern "C" int lddl_masked_lm_spans(lddl_ctx* c, lddl_pack* pk, const uint16_t* d_ids, const int64_t* d_src0,
                                    const int64_t* d_src1, const uint16_t* d_len0, const int64_t* d_part,
                                    int64_t* d_out_mlm_off, uint16_t* d_out_mlm_pos, uint16_t* d_out_mlm_label,
                                    uint16_t* d_out_mlm_token, void* stream) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (k->last_npairs < 0 || k->last_nmask < 0)
    return set_err(LDDL_EINVAL, "lddl_masked_lm_spans needs lddl_pack_bert(masking=1) then lddl_row_spans");
  if (!d_out_mlm_off || (k->last_npairs > 0 && (!d_ids || !d_src0 || !d_src1 || !d_len0 || !d_part)) ||
      (k->last_nmask > 0 && (!d_out_mlm_pos || !d_out_mlm_label || !d_out_mlm_token)))
    return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (k->last_npairs == 0) {
    HIP_TRY(hipMemsetAsync(d_out_mlm_off, 0, 8, st));
  } else {
    MlmParams M = mlm_params(k);
    M.row_part = d_part;
    M.ids = d_ids;
    M.src0 = d_src0;
    M.src1 = d_src1;
    M.len0 = d_len0;
    M.out_off = d_out_mlm_off;
    M.out_pos = d_out_mlm_pos;
    M.out_label = d_out_mlm_label;
    M.out_token = d_out_mlm_token;
    HIP_TRY(launch_masked_lm(M, k->last_npairs, st));
  }
  return 0;
}

extern "C" int lddl_row_docs(lddl_ctx* c, lddl_pack* pk, int64_t* d_out_doc, void* stream) {
  lddl_pack* k = pack_of(c, pk);
  if (!k) return LDDL_EINVAL;
  if (k->last_npairs < 0) return set_err(LDDL_EINVAL, "no successful lddl_pack_* call");
  if (!d_out_doc) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  const PackParams& P = k->pp;
  RowDocParams D{};
  D.V = pack_view(k);
  D.fs_base = P.fs_base;
  D.sent_off = P.sent_off;
  D.n_rows = k->last_npairs;
  D.out_doc = d_out_doc;
  HIP_TRY(launch_row_docs(D, c->n_cu, (hipStream_t)stream));
  return 0;
}

extern "C" int lddl_pack_new(lddl_ctx* c, lddl_pack** out) {
  if (!c || !out) return set_err(LDDL_EINVAL, "null pointer");
  lddl_pack* k = new (std::nothrow) lddl_pack;
  if (!k) return set_err(LDDL_ENOMEM, "out of host memory");
  k->device = c->device;
  k->mlm_cap = c->mlm_cap0;
  *out = k;
  return 0;
}

extern "C" void lddl_pack_free(lddl_pack* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  free_pack(k);
  delete k;
}

extern "C" int lddl_pack_rows(const lddl_pack* k, int64_t* out_npairs) {
  if (!k || !out_npairs) return set_err(LDDL_EINVAL, "null pointer");
  *out_npairs = k->last_npairs;
  return 0;
}

// ---------------------------------------------------------------- bin ----
extern "C" int lddl_bin(lddl_ctx* c, const int64_t* d_num_tokens, int64_t n, int32_t bin_size, int32_t nbins,
                        int64_t* d_out_perm, int64_t* d_out_bin_counts, void* stream) {
  if (!c) return set_err(LDDL_EINVAL, "null ctx");
  if (n < 0) return set_err(LDDL_EINVAL, "negative row count");
  if (bin_size < 1) return set_err(LDDL_EINVAL, "bin_size %d < 1", bin_size);
  if (nbins < 1 || nbins > 1024) return set_err(LDDL_EINVAL, "nbins %d not in [1, 1024]", nbins);
  if (!d_out_bin_counts || (n > 0 && (!d_num_tokens || !d_out_perm))) return set_err(LDDL_EINVAL, "null pointer");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  const int64_t nh = bin_chunks(n) * nbins;
  int32_t *hist, *err;
  int64_t *base, *bsum;
  int rc;
  uint32_t e;
  if ((rc = ws_get(c, CW_BIN_HIST, (size_t)(nh ? nh : 1), &hist)) || (rc = ws_get(c, CW_BIN_BASE, (size_t)nh + 1, &base)) ||
      (rc = ws_get(c, CW_BIN_BSUM, (size_t)scan_blocks(nh) + 1, &bsum)) || (rc = ws_get(c, CW_BIN_ERR, 1, &err)))
    return rc;
  HIP_TRY(launch_bin(d_num_tokens, n, bin_size, nbins, hist, base, bsum, d_out_perm, d_out_bin_counts, err, st));
  if ((rc = read_err(c, err, st, &e))) return rc;
  if (e) return set_err(LDDL_EINDEX, "IndexError: list index out of range (a length bins below -nbins, binning.py:70-73)");
  return 0;
}
