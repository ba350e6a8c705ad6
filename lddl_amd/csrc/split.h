// Rule-based sentence split of raw records (split.hip): device side of lddl_split_len / lddl_split.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lddl {

// bits of the code point property table (splitnative.props_table, split_rules.c)
enum : uint32_t { SP_SPACE = 1, SP_UPPER = 2, SP_DIGIT = 4, SP_ALPHA1 = 8 };
constexpr int64_t SPLIT_PROPS_N = 0x110000;

// error word of the split kernels
enum : uint32_t {
  SPLIT_E_RECOFF = 1,  // rec_off does not start at 0, runs backwards or does not end at nbytes
  SPLIT_E_DOCOFF = 2,  // (fill) d_doc_sent_off is not what the length call gives
};

static constexpr unsigned long long SPLIT_NO_REC = ~0ull;
constexpr int SPLIT_PIECE = 4096;  // bytes a wave owns (64 steps of 64 bytes), whatever records they belong to

// int64 words of the calls' device meta block
enum SplitMeta { SM_BYTES, SM_BAD, SM_ERR, SM_COUNT };

struct SentSplitParams {
  const uint8_t* buf;
  int64_t nbytes;
  const int64_t* rec_off;   // [n_rec + 1]
  int64_t n_rec;
  int32_t mode;             // 0: id + body, 1: whole line
  const uint8_t* props;     // [SPLIT_PROPS_N]
  // per record (workspace)
  int32_t* rec_b0;          // body start
  int32_t* rec_end;         // end of the body stripped of whitespace (when it has a sentence)
  int32_t* rec_cnt;         // sentences
  int64_t* id_end;          // output of the length call, may be null
  // meta
  unsigned long long* bytes;    // sum of the sentences' bytes
  unsigned long long* bad_rec;  // lowest record that is not strict UTF-8
  uint32_t* err;
  // fill only (null in the length call)
  unsigned long long* fsmap;    // bit p: p starts the first sentence of a record
  int32_t* piece_cnt;           // sentence starts per piece
  const int64_t* piece_base;    // [pieces + 1] their exclusive scan
  const int64_t* doc_sent_off;  // the length call's scan (workspace copy, compared with the caller's)
  const int64_t* user_doc_sent_off;
  int64_t n_sent, out_bytes;
  int32_t* sent_start;          // [n_sent]
  int32_t* sent_end;            // [n_sent], then the lengths in place
  const int64_t* sent_off;      // [n_sent + 1] output offsets
  uint8_t* out;
};

__host__ __device__ inline int64_t split_pieces(int64_t nbytes) { return (nbytes + SPLIT_PIECE - 1) / SPLIT_PIECE; }

hipError_t launch_split_head(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_count(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_compare(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_mark(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_tail(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_lens(const SentSplitParams& P, int n_cu, hipStream_t s);
hipError_t launch_split_copy(const SentSplitParams& P, int n_cu, hipStream_t s);

}  // namespace lddl
