// Training-time collate of parquet rows into BERT model inputs (device side of
// lddl_collate_seq_len / lddl_collate_bert / lddl_mask_tokens).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lddl {

enum : int32_t { COLLATE_SPECIAL_MASK = 0, COLLATE_STATIC = 1, COLLATE_DYNAMIC = 2 };

// What mode 2 selects, a template constant of its kernels: tokens (`_mask_tokens`), whole words
// (lddl_set_whole_word_mask) or geometric spans of whole words (lddl_set_span_mask).
enum : int { SEL_TOKEN = 0, SEL_WORD = 1, SEL_SPAN = 2 };

// Span masking: lddl_span_params' outputs for the call's mlm_probability.  L = 0: off.
struct SpanLaw {
  double q;        // a word start opens a span iff its select draw is below q
  double cdf[16];  // P(len <= t + 1) in [t], 1.0 from t = L - 1 on
  int32_t L;       // max_span
};

// Whole-token vocab table for convert_tokens_to_ids: open addressing over
// slots {hash, id}; the key bytes are verified against the render pool
// (vinfo[id] = offset << 8 | length, the full entry text incl. "##").
struct CollateVocab {
  const uint2* slots;
  uint32_t mask;
  const uint32_t* vinfo;
  const uint8_t* vpool;
  int32_t unk, cls, sep, mask_id;
  int32_t n_random;  // len(tokenizer): randint bound of the 10 % random words
};

// The string columns of parquet rows as (bytes, offsets [n_rows + 1]) each.
// pos .. lab_off are NULL without static masking.
struct StringColumns {
  const uint8_t* a;
  const int64_t* a_off;
  const uint8_t* b;
  const int64_t* b_off;
  const uint8_t* pos;  // masked_lm_positions: np.save bytes per row
  const int64_t* pos_off;
  const uint8_t* lab;  // masked_lm_labels: space-joined label tokens
  const int64_t* lab_off;
};

struct CollateParams {
  CollateVocab V;
  StringColumns C;
  const uint8_t* is_random_next;  // [n_rows] (bool bytes)
  int64_t n_rows;
  int32_t seq_len;   // output columns (aligned)
  int32_t mode;      // COLLATE_*
  int64_t ignore_index;
  double mlm_probability;
  uint64_t seed, counter;
  const uint32_t* cont;      // whole-word masking (mode 2 with lddl_set_whole_word_mask on): bit id = entry id begins with "##"; else NULL
  SpanLaw span;              // span masking (mode 2 with lddl_set_span_mask on; cont is then set as well)
  int64_t* input_ids;        // [n_rows, seq_len]
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* labels;           // labels, or special_tokens_mask (COLLATE_SPECIAL_MASK)
  int64_t* next_sentence_labels;  // [n_rows]
  int32_t* max_len;          // [1] max over rows of len(A) + len(B) + 3 (seq-len pass)
  uint32_t* err;             // [1] first error code (0 = none) | row << 4
};

struct MaskParams {
  int64_t* inputs;            // [n_rows, seq_len], masked in place
  const int64_t* special;     // [n_rows, seq_len] special_tokens_mask
  int64_t* labels;            // [n_rows, seq_len]
  int64_t n_rows;
  int32_t seq_len, mask_id, n_random;
  int64_t ignore_index;
  double mlm_probability;
  uint64_t seed, counter;
  const uint32_t* cont;       // whole-word masking: as CollateParams::cont, over n_random entries; else NULL
  SpanLaw span;               // span masking: as CollateParams::span
};

// lddl_collate_rows_seq_len / lddl_collate_rows: batch row r is row
// g = rows[r] (rows NULL: row0 + r) of a pack result's spans over the dense ids.
// The lddl_collate_code_rows* calls fill the same struct for CodeBERT rows:
// mlm_off .. mlm_token and next_sentence_labels stay NULL, and the seq-len and
// offsets passes read flags as well.
struct CollateRowsParams {
  const uint16_t* ids;    // the dense ids (16 entries of padding behind the last)
  const int64_t* src0;    // [n_total] lddl_row_spans' outputs
  const int64_t* src1;
  const uint16_t* len0;
  const uint16_t* len1;
  const uint8_t* flags;
  const int64_t* rows;    // [n_rows] or NULL
  int64_t row0, n_rows, n_total;
  const int64_t* mlm_off;     // COLLATE_STATIC: lddl_masked_lm_spans' outputs
  const uint16_t* mlm_pos;
  const uint16_t* mlm_label;
  const uint16_t* mlm_token;
  int32_t cls, sep, mask_id, n_random;
  int32_t seq_len;
  int64_t ignore_index;
  double mlm_probability;
  uint64_t seed, counter;
  const uint32_t* cont;      // whole-word masking: as CollateParams::cont, over n_random entries; else NULL
  SpanLaw span;              // span masking: as CollateParams::span
  int64_t* input_ids;        // [n_rows, seq_len]
  int64_t* token_type_ids;
  int64_t* attention_mask;
  int64_t* labels;
  int64_t* next_sentence_labels;  // [n_rows]
  int32_t* max_len;          // [1] (seq-len pass)
  uint32_t* err;             // [1] as CollateParams::err
};

// lddl_collate_rows_cu_seqlens / lddl_collate_rows_unpadded (collate_unpadded.hip):
// the same batch without its pad columns, row r at tokens [cu_seqlens[r],
// cu_seqlens[r + 1]).  R.seq_len and R.attention_mask are unused; R.max_len is
// the offsets pass's max over the rows of len0 + len1 + 3 (CodeBERT: + 2 + s).
struct CollateUnpaddedParams {
  CollateRowsParams R;     // input_ids, token_type_ids, labels: [total]
  int32_t* cu_seqlens;     // [n_rows + 1]: written by the offsets pass, checked by the fill pass
  int64_t* position_ids;   // [total]
  int64_t total;           // fill pass: the capacity of the token outputs
  uint32_t* chunk_sum;     // offsets pass: [n_chunks] tokens of each chunk of rows
  int64_t* total_out;      // offsets pass: [1] tokens of the batch
  int64_t n_chunks;        // collate_chunks(n_rows)
};

// lddl_collate_rows_fixed / lddl_collate_code_rows_fixed (collate_fixed.hip): the
// padding-free batch in outputs of fixed capacity, offsets and fill in one
// launch.  R.seq_len is max_seqlen, the bound of a row and the length of a pad
// sequence; R.attention_mask and R.max_len are unused.
struct CollateFixedParams {
  CollateRowsParams R;     // input_ids, token_type_ids, labels: [tok_cap]; next_sentence_labels: [seq_cap];
                           // err: [2], the rows' error word, then CERR_TOK_CAP / CERR_SEQ_CAP
  int32_t* cu_seqlens;     // [seq_cap + 1], written
  int64_t* position_ids;   // [tok_cap]
  int64_t tok_cap, seq_cap;
  int64_t rows_per_block;  // the run of batch rows a block takes: a multiple of 4
  int32_t* status;         // [4] total, n_rows, n_seqs, max_seqlen
  int64_t* total_out;      // [1] tokens of the batch, 64-bit
};

// lddl_rows_from_strings_len / lddl_rows_from_strings (rows_from_strings.hip):
// the string columns of a shard into the row table that lddl_row_spans +
// lddl_masked_lm_spans leave behind.  mlm_off .. mlm_token are NULL without
// static masking.  lddl_code_rows_from_strings[_len] fill it for a CodeBERT
// shard: C.a / C.b are doc / code, num_tokens is set, and is_random_next, the
// static columns and every mlm_* field are NULL.
struct RowsFromStringsParams {
  CollateVocab V;         // fill pass only
  StringColumns C;
  const uint8_t* is_random_next;  // [n_rows] (bool bytes; fill pass)
  const uint16_t* num_tokens;     // [n_rows] CodeBERT: a + b + 2 + s
  int64_t n_rows;
  uint16_t* len0;         // [n_rows] written by the length pass, checked by the fill pass
  uint16_t* len1;
  int64_t* src0;          // [n_rows] written by the scan, checked by the fill pass
  int64_t* src1;
  int64_t* tok_off;       // [n_rows + 1] or NULL (length pass)
  int64_t* mlm_off;       // [n_rows + 1]: the length kernel leaves k_r in [r + 1], the scan sums in place
  uint16_t* ids;          // fill pass: [ids_cap]
  int64_t ids_cap;
  uint8_t* flags;         // [n_rows]
  uint16_t* mlm_pos;      // [mlm_cap]
  uint16_t* mlm_label;
  uint16_t* mlm_token;
  int64_t mlm_cap;
  unsigned long long* chunk_sum;  // length pass: [n_chunks] ids (low half) | masked entries (high half) of each chunk of rows
                                  // (CodeBERT: rows with s = 1 in the high half)
  int64_t* totals;        // length pass: [3] ids, row tokens and masked entries (CodeBERT: rows with s = 1) of the table
  int64_t n_chunks;       // collate_chunks(n_rows)
  uint32_t* err;          // [1] as CollateParams::err
};

// lddl_mlm_targets (mlm_targets.hip): the ordered compaction of a labels
// tensor.  Row r is [r * seq_len, (r + 1) * seq_len) (cu_seqlens NULL; the
// host has checked total = n_rows * seq_len) or [cu_seqlens[r],
// cu_seqlens[r + 1]) within [0, total), checked on the device.
struct MlmTargetsParams {
  const int64_t* labels;      // [total]
  const int32_t* cu_seqlens;  // [n_rows + 1] or NULL
  int64_t n_rows, seq_len, total;
  int64_t ignore_index;       // < 0
  int64_t capacity;           // entries of positions / target_labels that may be written
  int64_t* positions;         // [capacity]
  int64_t* target_labels;     // [capacity]
  int32_t* offsets;           // [n_rows + 1]: the count pass leaves row r's count in [r + 1], the scan sums in place
  unsigned long long* chunk_sum;  // [n_chunks] selected tokens of each chunk of rows (zeroed by the host)
  int64_t* count_out;         // [1] M
  uint32_t* err;              // [1] as CollateParams::err
  int64_t n_chunks;           // collate_chunks(n_rows)
};

// error codes in CollateParams::err / CollateRowsParams::err (low 4 bits)
enum : uint32_t {
  CERR_LONG = 1,
  CERR_POS_RANGE = 2,
  CERR_NPY = 3,
  CERR_NLAB = 4,
  CERR_ROW_INDEX = 5,
  CERR_NO_SEP = 6,
  CERR_CU_SEQLENS = 7,  // collate_unpadded.hip: a row's cu_seqlens are not its [c, c + n) within the outputs
  CERR_ROW_COUNTS = 8,  // rows_from_strings.hip: a row's len / src / mlm_off are not what its strings give
  CERR_TABLE_CAP = 9,   // rows_from_strings.hip: the table ends beyond ids_cap / mlm_cap
  CERR_NMASK = 10,      // rows_from_strings.hip: more masked positions than the longest row has tokens
  CERR_CODE_ROW = 11,   // a CodeBERT row whose s is not 0 or 1 (num_tokens - a - b - 2, rows_from_strings.hip), or is 0 with a > 0
  CERR_TOK_CAP = 12,    // collate_fixed.hip: the batch holds more tokens than tok_cap
  CERR_SEQ_CAP = 13     // collate_fixed.hip: the rows and the pad sequences of the slack take more slots than seq_cap
};

constexpr int COLLATE_MAX_LEN = 2048;  // per-row LDS buffer (columns)

// rows per block of the offsets scans (collate_row.h), 8 per thread, and the blocks that n_rows take
constexpr int kChunk = 2048;
inline int64_t collate_chunks(int64_t n_rows) { return (n_rows + kChunk - 1) / kChunk; }

// what a dynamic launch selects, from its params' cont and span
inline int collate_sel(const uint32_t* cont, const SpanLaw& span) { return span.L > 0 ? SEL_SPAN : cont ? SEL_WORD : SEL_TOKEN; }

uint32_t collate_hash_host(const uint8_t* p, int n);
// code: the rows are CodeBERT rows (modes 0 and 2 only)
hipError_t launch_collate_rows_len(const CollateRowsParams& P, bool code, int n_cu, hipStream_t s);
hipError_t launch_collate_rows(const CollateRowsParams& P, bool code, int32_t mode, int n_cu, hipStream_t s);
hipError_t launch_collate_cu_seqlens(const CollateUnpaddedParams& P, bool code, hipStream_t s);
hipError_t launch_collate_unpadded(const CollateUnpaddedParams& P, bool code, int32_t mode, int n_cu, hipStream_t s);
hipError_t launch_collate_fixed(const CollateFixedParams& P, bool code, int32_t mode, int n_cu, hipStream_t s);
hipError_t launch_collate_len(const CollateParams& P, int n_cu, hipStream_t s);
hipError_t launch_collate_fill(const CollateParams& P, int n_cu, hipStream_t s);
// (a CodeBERT shard when P.num_tokens is set)
hipError_t launch_rows_from_strings_len(const RowsFromStringsParams& P, int n_cu, hipStream_t s);
hipError_t launch_rows_from_strings(const RowsFromStringsParams& P, int n_cu, hipStream_t s);
hipError_t launch_mask_tokens(const MaskParams& M, int n_cu, hipStream_t s);
hipError_t launch_mlm_targets(const MlmTargetsParams& P, int n_cu, hipStream_t s);

}  // namespace lddl
