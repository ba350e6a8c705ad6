// What the files of the C-ABI's host side (capi.hip, capi_tokenize / capi_pack / capi_render /
// capi_collate.hip) share: the ctx and pack-result structs, their workspace and pinned-word slots, error
// reporting and the read-back of a word from the device.  Private: not installed, included by those files only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "../../include/lddl_amd.h"
#include "collate.h"
#include "common.h"
#include "pack.h"
#include "render.h"
#include "tok_tables.h"
#include "tokenize.h"

using namespace lddl;

// keeps the message for lddl_last_error() (thread-local, capi.hip); returns code
__attribute__((visibility("hidden"))) int set_err(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) return set_err(LDDL_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// a device buffer grown on demand
struct WsBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// Slots of lddl_pack::ws, the buffers of one pack result.
enum PackWs {
  PW_FS_NTOK,      // per filtered sentence: its token count
  PW_FS_BASE,      // per filtered sentence: its byte offset
  PW_FD_FIRST,     // per filtered doc: its first filtered sentence
  PW_FD_N,         // per filtered doc: its filtered sentences
  PW_FD_ND,        // per filtered doc: CodeBERT docstring segment count
  PW_PAIRS,        // the pair records
  PW_ORDER,        // their shuffled order
  PW_BINNED,       // their binned order
  PW_TOK_LOCAL,    // per pair: its token offset within the partition
  PW_PART_NPAIRS,  // per partition: its pairs
  PW_PART_NTOK,    // per partition: its tokens
  PW_BIN_COUNT,    // per partition and bin: its rows
  PW_BIN_CURSOR,   // per partition and bin: the binning cursor
  PW_PART_ERR,     // per partition: PACK_E* flags
  PW_PAIR_BASE,    // [n_part + 1] exclusive scan of PW_PART_NPAIRS (read by the post-pack calls)
  PW_TOK_BASE,     // [n_part + 1] exclusive scan of PW_PART_NTOK (read by the post-pack calls)
  PW_ERR_ANY,      // the partitions' error flags or-ed
  PW_KEPT,         // [n_sent + n_part + 1] wave packer scratch
  PW_MT_STATES,    // MT19937 state per partition (whole 64-partition rows)
  PW_SENT_SPEC,    // per sentence: holds [CLS] / [SEP], when the tokenizer's flags (CW_SENT_SPEC) do not apply
  PW_FS_SPEC,      // the same per filtered sentence
  PW_MREF,         // masking: per record, arena offset | #masked << 48
  PW_MLOC,         // masking: per binned position, the masked entries before it
  PW_PART_NMASK,   // masking: per partition, its masked entries
  PW_MASK_BASE,    // masking: [n_part + 1] exclusive scan of PW_PART_NMASK (read by lddl_masked_lm[_spans])
  PW_MASK_BASE2,   // masking: the second output of that scan (unused)
  PW_MCOUNTER,     // masking: the arena's bump allocator
  PW_MARENA,       // masking: the arena of masked entries
  PW_MCAND,        // masking: per partition, MLM_MAX_SEQ candidate positions
  PW_FS_DENSE,     // per filtered sentence: its offset in the tokenizer's dense ids
  PW_SPAN,         // per binned position: the row's SpanRec, streamed by lddl_row_spans
  PW_COUNT
};

// Slots of lddl_ctx::ws.  The header allows one call at a time per ctx, so
// entry points that never need a buffer at the same time share a slot (the
// CW_SHARED_* ones: one allocation serves all their users); CW_SENT_SPEC is
// handed from lddl_tokenize to the next masked lddl_pack_bert on purpose.
enum CtxWs {
  CW_BIN_HIST,     // lddl_bin: per chunk and bin, its rows
  CW_BIN_BASE,     // lddl_bin: exclusive scan of CW_BIN_HIST
  CW_BIN_BSUM,     // lddl_bin: block sums of that scan
  CW_BIN_ERR,      // lddl_bin: the error flag
  CW_NPY_ERR,      // lddl_render_npy: the error flag
  CW_TILE_SENT,    // tokenize: [tiles + 1] first sentence of each tile
  CW_FB_LIST,      // tokenize: sentence ranges for the serial path
  CW_FB_COUNT,     // tokenize: ranges listed in the segment
  CW_ENT,          // tokenize: the segment's entry / staging buffer
  CW_SHARED_ROWS,  // tokenize: rec, the record slots; lddl_render_strings / _npy / _masked: lens, bytes per row
  CW_SHARED_BSUM,  // tokenize: chunk_fill + chunk_ctr; lddl_render_strings / _npy / _masked: block sums of the lens scan;
                   // lddl_collate_rows_cu_seqlens / lddl_rows_from_strings_len: chunk sums of their scans;
                   // lddl_mlm_targets: M, its error word, then the chunk sums of its scan (one memset)
  CW_SHARED_META,  // tokenize: smeta, per sentence; lddl_collate[_rows]_seq_len: max_len;
                   // lddl_collate_rows_cu_seqlens: total, max_len; lddl_rows_from_strings_len: its three totals;
                   // lddl_collate_rows_fixed: total, its error word (one memset)
                   // the lddl_bart_* calls use the three too: ROWS = chunks per document (plan_len) / bytes per chunk
                   // (plan), BSUM = block sums of their scans, META = {bytes total, refused chunk, error word}
  CW_COLLATE_ERR,  // lddl_collate_bert / lddl_collate_rows[_seq_len | _cu_seqlens | _unpadded] / lddl_rows_from_strings[_len]:
                   // the error word
  CW_SENT_SPEC,    // per sentence: holds [CLS] / [SEP]; written by lddl_tokenize (lddl_set_special_flags),
                   // read by the next masked lddl_pack_bert over the same buffers (pack_common)
  CW_PCS,          // tokenize: WordPiece pieces 4.. per record slot
  CW_SNSLOT,       // tokenize: per sentence, its record slots
  CW_CNT8,         // tokenize: per record slot, the word's pieces
  CW_SCAN_BSUM,    // tokenize: block sums of the token-count scan
  CW_PCH,          // tokenize: WordPiece head per record slot
  CW_CHUNK_PART,   // lddl_row_spans: the partition of every 64 rows
  CW_PART_PB,      // lddl_row_spans: per partition, launch_chunk_parts' pair base
  CW_SPLIT_REC,    // lddl_split[_len]: per record, body start / stripped end / sentences (int32 each), then its
                   // own doc_sent_off (int64)
  CW_SPLIT_PIECE,  // lddl_split: sentence starts per piece (int32), then their exclusive scan (int64)
  CW_SPLIT_MAP,    // lddl_split: a bit per input byte, set where a record's first sentence starts
  CW_SPLIT_SENT,   // lddl_split: per sentence, its start and its end / length in the input (int32 each)
  CW_COUNT
};

// Words of lddl_ctx::h_tot, the pinned int64 words through which a call reads a few device values back
// (fetch_word).  One call at a time per ctx, so calls share the words, and two pairs of names share a word
// on purpose: the eight fill one cache line.  A value narrower than 8 bytes fills the word's low bytes.
enum HostWord {
  HW_NPAIRS,        // lddl_pack_bert / _codebert: the rows of the pack
  HW_BART_LO = HW_NPAIRS,  // the same word; lddl_bart_plan_len: the chunks; lddl_bart_render: chunk_off[c0]
  HW_NTOK,          // lddl_pack_bert / _codebert: their tokens; lddl_rows_from_strings_len: the table's ids
  HW_BART_HI = HW_NTOK,    // the same word; lddl_bart_plan_len: the chunks' bytes; lddl_bart_render: chunk_off[c0 + n],
                           // then the lowest refused chunk
  HW_PACK_ERR,      // lddl_pack_bert / _codebert: the partitions' PACK_E* flags or-ed (int32);
                    // lddl_rows_from_strings_len: the table's row tokens (one 24-byte copy with its neighbours)
  HW_BART_NSENT = HW_PACK_ERR,  // the same word; lddl_bart_plan_len: doc_sent_off's last entry, compared with n_sent
  HW_SPLIT_NSENT = HW_NPAIRS, HW_SPLIT_BYTES = HW_NTOK, HW_SPLIT_BAD = HW_PACK_ERR,  // the same words;
                    // lddl_split[_len]: the sentences, their bytes, the lowest record that is not UTF-8
  HW_NMASK,         // lddl_pack_bert (masking): the masked entries; lddl_rows_from_strings_len: the same of the table
  HW_MARENA_USED,   // lddl_pack_bert (masking): the arena entries the bump allocator handed out
  HW_NDENSE,        // lddl_pack_bert / _codebert: the tokenizer's dense ids
  HW_CU_TOTAL = HW_NDENSE,  // the same word; lddl_collate_rows_cu_seqlens: the batch's tokens (one 16-byte copy with HW_MAX_LEN);
                            // lddl_mlm_targets: M, with its error word in HW_MAX_LEN by the same copy;
                            // lddl_collate_rows_fixed: the batch's tokens, with its error word in HW_MAX_LEN likewise
  HW_MAX_LEN,       // lddl_collate_seq_len / lddl_collate_rows_seq_len / lddl_collate_rows_cu_seqlens: the longest row (int32)
  HW_RENDER_BYTES = HW_MAX_LEN,  // the same word; lddl_render_strings / _npy / _masked: the bytes of the rendered column
  HW_ERR,           // lddl_bin, lddl_render_npy, lddl_collate_bert, lddl_collate_rows[_seq_len | _cu_seqlens | _unpadded],
                    // lddl_rows_from_strings[_len]: the error word
  HW_COUNT
};
static_assert(HW_MAX_LEN == HW_CU_TOTAL + 1, "lddl_collate_rows_cu_seqlens reads total and max_len with one copy");
static_assert(HW_PACK_ERR == HW_NTOK + 1 && HW_NMASK == HW_NTOK + 2, "lddl_rows_from_strings_len reads its three totals with one copy");

// The result of one lddl_pack_* call, owned by the caller (lddl_pack_new):
// the pair records, their shuffled / binned order, the per-partition counts
// and offsets and (masking) the masked positions -- everything the post-pack
// calls (lddl_materialize, lddl_row_spans, lddl_masked_lm[_spans],
// lddl_row_docs) read.  A ctx holds one of its own for callers that pass
// NULL.  Buffers grow on demand and are reused by later packs into it.
struct lddl_pack {
  int device = 0;
  WsBuf ws[PW_COUNT];
  PackParams pp{};
  int64_t last_npairs = -1, last_ntok = -1, last_nmask = -1, last_ndense = 0;
  uint64_t mlm_cap = 0;  // masking arena capacity that last sufficed
  uint16_t* last_tokens = nullptr;  // rows of the last lddl_materialize of this result
  const int64_t* last_tok_off = nullptr;
  const int64_t* last_part = nullptr;
};

struct lddl_ctx {
  int device = 0;
  int n_cu = 0;
  int vocab_size = 0;
  uint32_t special[5] = {0, 0, 0, 0, 0};
  std::vector<std::string> vocab;  // host copy (for rendering / tests)
  // device tables
  uint16_t* d_top = nullptr;
  uint32_t* d_pages = nullptr;
  uint32_t* d_bmp = nullptr;  // flat entries of the Basic Multilingual Plane (top/pages resolved)
  uint32_t* d_xmap = nullptr;  // fast exception entries, one per code point (tokenize_split.hip XM_*)
  uint4* d_multi = nullptr;
  uint4* d_slots = nullptr;
  uint32_t* d_bloom = nullptr;
  uint32_t slot_mask = 0;
  uint8_t* d_pool = nullptr;
  uint32_t* d_voff = nullptr;
  uint8_t* d_rpool = nullptr;    // full vocab strings (incl. "##"), 4-aligned: rendering
  uint32_t* d_rinfo = nullptr;   // [V] offset << 8 | length into d_rpool
  uint32_t* d_cont = nullptr;    // [(V + 31) / 32] bit id: entry id begins with "##" (whole-word masking)
  bool whole_word = false;       // lddl_set_whole_word_mask
  int32_t span_max = 0;          // lddl_set_span_mask: max_span (0: off) and geo_p
  double span_geo = 0.0;
  uint32_t maxb[2] = {0, 0};
  uint4* d_vt = nullptr;         // v4 bucketed vocab table
  uint32_t vt_mask = 0;
  uint32_t* d_vbloom = nullptr;  // its Bloom filter
  bool scan_ok = false;          // the ASCII page fits the split scan's per-byte class table
  // per-kernel timing of the split tokenizer (lddl_set_timing)
  bool timing = false;
  SplitTiming* tm = nullptr;
  unsigned long long* d_nrec = nullptr;
  // per-sentence [CLS]/[SEP] flags written by the last lddl_tokenize (CW_SENT_SPEC),
  // reused by a masked lddl_pack_bert over the same id / count buffers
  const void* spec_ids = nullptr;
  const void* spec_ntok = nullptr;
  const void* spec_soff = nullptr;
  int64_t spec_nsent = -1;
  bool spec_flags = false;  // lddl_set_special_flags
  // tokenizer / render / collate workspace (grown on demand)
  WsBuf ws[CW_COUNT];
  int64_t* h_tot = nullptr;  // pinned [HW_COUNT], allocated by lddl_create
  lddl_pack own;             // the pack result of calls that pass no lddl_pack
  uint64_t mlm_cap0 = 0;     // initial masking arena (LDDL_MLM_CAP, tests)
  // scratch
  int tok_grid = 0;
  int tok_algo = 5;  // 5 = split tokenizer, 0 = every tile through the exact serial path
  uint8_t* d_ovf = nullptr;
  uint32_t* d_counter = nullptr;
  // debug counters of the tokenizer (LDDL_TOK_DEBUG=1) and of the packers
  // (LDDL_PACK_DEBUG=1: phase ticks + per-wave start / end), on this ctx's device
  uint64_t* d_tdbg = nullptr;
  uint64_t* d_pdbg = nullptr;
  int64_t pdbg_cap = 0;
  // collate: whole-token vocab table (built on first use)
  uint2* d_ctab = nullptr;
  uint32_t ctab_mask = 0;
  // sentence split: the code point properties (lddl_set_split_props)
  uint8_t* d_split_props = nullptr;
};

template <class T>
static int ws_get(WsBuf* ws, int slot, size_t n, T** out) {
  auto& b = ws[slot];
  const size_t bytes = (n ? n : 1) * sizeof(T);
  if (b.cap < bytes) {
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    HIP_TRY(hipMalloc(&b.p, bytes));
    b.cap = bytes;
  }
  *out = (T*)b.p;
  return 0;
}
template <class T>
static int ws_get(lddl_ctx* c, int slot, size_t n, T** out) {
  return ws_get(c->ws, slot, n, out);
}
static inline void free_pack(lddl_pack* k) {
  for (auto& b : k->ws) {
    (void)hipFree(b.p);
    b = WsBuf{};
  }
}

template <class T>
static int upload(T** dst, const void* src, size_t bytes) {
  HIP_TRY(hipMalloc((void**)dst, bytes ? bytes : 16));
  if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

// queues the copy of a device value into pinned word w: read c->h_tot[w] after the stream's next synchronize
static inline hipError_t fetch_word(lddl_ctx* c, HostWord w, const void* d_src, size_t bytes, hipStream_t st) {
  return hipMemcpyAsync(&c->h_tot[w], d_src, bytes, hipMemcpyDeviceToHost, st);
}

// The error-word round trip: d_err's 4 bytes into HW_ERR, synchronize, *e = the
// word.  Words fetched before it on the stream arrive under the same synchronize.
static inline int read_err(lddl_ctx* c, const void* d_err, hipStream_t st, uint32_t* e) {
  HIP_TRY(fetch_word(c, HW_ERR, d_err, 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  *e = (uint32_t)(c->h_tot[HW_ERR] & 0xFFFFFFFF);
  return 0;
}
