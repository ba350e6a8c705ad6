// BART sentence aggregation (bart.hip): per-sentence str.split() counts, the chunk plan and the chunk text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lddl {

// error words of the BART kernels (first error wins where a row number is kept)
enum : uint32_t {
  BART_E_SENT = 1,   // a sentence's bytes leave [0, nbytes) or run backwards
  BART_E_DOC = 2,    // a document's sentences leave [0, n_sent] or run backwards
  BART_E_BYTES = 3,  // a chunk of 2^31 bytes or more
  BART_E_PLAN = 4,   // doc_chunk_off is not what the walk gives, or leaves [0, n_chunks]
};

static constexpr unsigned long long BART_NO_CHUNK = ~0ull;

struct BartCountParams {
  const uint8_t* data;
  int64_t nbytes;
  const int64_t* sent_off;  // [n_sent + 1]
  int64_t n_sent;
  int32_t* nwords;          // [n_sent]
  uint32_t* err;
};

struct BartPlanParams {
  const int32_t* nwords;        // [n_sent]
  const int64_t* sent_off;      // [n_sent + 1]
  const int64_t* doc_sent_off;  // [n_doc + 1]
  int64_t n_doc, n_sent;
  int64_t target;               // T = target_seq_length - 3
  // length pass
  int32_t* doc_nchunks;         // [n_doc]
  unsigned long long* total_bytes;
  uint32_t* err;
  // fill pass
  const int64_t* doc_chunk_off; // [n_doc + 1]
  int64_t n_chunks;
  int64_t* chunk_sent0;         // [n_chunks]
  int32_t* chunk_nsent;         // [n_chunks]
  int32_t* chunk_num_tokens;    // [n_chunks]
  int32_t* chunk_len;           // [n_chunks] bytes, scanned into chunk_off
};

struct BartRenderParams {
  const uint8_t* data;
  int64_t nbytes;
  const int64_t* sent_off;      // [n_sent + 1]
  int64_t n_sent;
  const int64_t* chunk_sent0;   // indexed by absolute chunk number
  const int32_t* chunk_nsent;
  const int64_t* chunk_off;     // [.. c0 + n + 1]
  int64_t c0, n;
  int64_t* out_off;             // [n + 1], rebased to 0
  uint8_t* out;
  int64_t out_cap;
  unsigned long long* bad;      // lowest refused chunk number, BART_NO_CHUNK when none
};

hipError_t launch_bart_count(const BartCountParams& P, int n_cu, hipStream_t s);
hipError_t launch_bart_plan_len(const BartPlanParams& P, int n_cu, hipStream_t s);
hipError_t launch_bart_plan_fill(const BartPlanParams& P, int n_cu, hipStream_t s);
hipError_t launch_bart_rebase(const BartRenderParams& R, int n_cu, hipStream_t s);
hipError_t launch_bart_render(const BartRenderParams& R, int n_cu, hipStream_t s);

}  // namespace lddl
