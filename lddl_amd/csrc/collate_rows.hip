// Training-time collate straight from a pack result: the rows are spans of
// the tokenizer's dense ids (lddl_row_spans), picked through a row-index list,
// so a batch goes from the packer's HBM buffers to the model's int64 inputs
// without the parquet detour (render strings, encode, decode, split, vocab
// lookup -- collate.hip's route).
//
// Reference: lddl/torch/bert.py:69-153 `_to_encoded_inputs` and :156-196
// `_mask_tokens`, as in collate.hip; the token ids are the ones the strings
// would be looked up to.  Batch row r is pack row g = rows[r] (rows NULL:
// row0 + r); a = len0[g], b = len1[g], n = a + b + 3:
//   input_ids[r]      = [CLS] ids[src0[g] .. +a) [SEP] ids[src1[g] .. +b) [SEP], 0 padded
//   token_type_ids[r] = 1 on [a + 2, n);  attention_mask[r] = 1 on [0, n)
//   next_sentence_labels[r] = flags[g] & 1
//   labels[r] by mode: 0 special_tokens_mask; 1 the static masks of
//   lddl_masked_lm_spans (input_ids[pos] = mlm_token, labels[pos] = mlm_label,
//   ignore_index elsewhere); 2 mode 0 then mask_one with row = r.
//
// Work mapping: one wave per batch row, four rows per block.  A column's id is
// one 2-B load at an address known from (src, len) alone, so modes 0 and 2 need
// no staging: consecutive lanes read consecutive ids (128 B per wave
// instruction, 2 B in against 40 B out).  Loads stay 2 B wide on purpose: src0
// / src1 are arbitrary u16 offsets, a wider load would need an alignment
// prologue for a stream that is 5 % of the traffic, and a 2-B load never
// reaches past the span.  The bound is the four int64 output streams: a lane
// owns two adjacent columns and stores 16 B to each (1 KiB per wave
// instruction); an odd seq_len (alignment 1) leaves odd rows 8-B aligned only
// and takes the lane = column path with 8-B stores, as do outputs whose base
// is not 16-B aligned.  Mode 1 scatters the row's
// masked positions into a per-wave LDS row first (label | token << 16).
//
// No input faults: the row index is range-checked before anything is loaded
// through it, a row longer than seq_len, a static position >= seq_len and a
// CodeBERT row without docstring (flags bit 1 clear: no [SEP] after segment 0,
// bert.py has no such loader) set the error word and leave the row unwritten.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "wave.h"

namespace lddl {

static constexpr uint32_t kNoMask = 0xFFFFFFFFu;

// the pack row of batch row r, or -1 (error word set) when out of range
__device__ __forceinline__ int64_t pack_row(const CollateRowsParams& P, int64_t r) {
  const int64_t g = P.rows ? P.rows[r] : P.row0 + r;
  return (g < 0 || g >= P.n_total) ? -1 : g;
}

// max over the batch of len0 + len1 + 3: lane = row
__global__ __launch_bounds__(256) void collate_rows_len_kernel(CollateRowsParams P) {
  const int64_t nt = (int64_t)gridDim.x * 256;
  uint32_t m = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < P.n_rows; r += nt) {
    const int64_t g = pack_row(P, r);
    if (g < 0) {
      set_err(P.err, CERR_ROW_INDEX, r);
      continue;
    }
    m = max(m, (uint32_t)P.len0[g] + (uint32_t)P.len1[g] + 3u);
  }
  m = wave_incl_max(m);
  if ((threadIdx.x & 63) == 63 && m) atomicMax(P.max_len, (int32_t)m);
}

struct RowShape {
  const uint16_t* s0;  // ids + src0 - 1: column j of segment 0 is s0[j]
  const uint16_t* s1;  // ids + src1 - (a + 2)
  int32_t a, n;
};

struct ColumnOut {
  int64_t id, tt, am, lab;
};

// the four outputs of column j (0 <= j < seq_len) of batch row r
template <int MODE>
__device__ __forceinline__ ColumnOut column(const CollateRowsParams& P, const RowShape& S, const uint32_t* mlm,
                                            int64_t r, int32_t j) {
  ColumnOut o;
  const int32_t a = S.a, n = S.n;
  const bool special = j == 0 || j == a + 1 || j >= n - 1;
  int64_t id;
  if (j == 0) id = P.cls;
  else if (j == a + 1 || j == n - 1) id = P.sep;
  else if (j <= a) id = S.s0[j];
  else if (j < n) id = S.s1[j];
  else id = 0;
  if (MODE == COLLATE_SPECIAL_MASK) {
    o.lab = special ? 1 : 0;
  } else if (MODE == COLLATE_STATIC) {
    const uint32_t m = mlm[j];
    o.lab = m == kNoMask ? P.ignore_index : (int64_t)(m & 0xFFFFu);
    if (m != kNoMask) id = (int64_t)(m >> 16);
  } else {
    id = mask_one(id, special, r, j, P.seed, P.counter, P.mlm_probability, P.mask_id, P.n_random, P.ignore_index,
                  o.lab);
  }
  o.id = id;
  o.tt = (j >= a + 2 && j < n) ? 1 : 0;
  o.am = j < n ? 1 : 0;
  return o;
}

template <int MODE>
__global__ __launch_bounds__(256) void collate_rows_kernel(CollateRowsParams P) {
  // mode 1 only: per wave, label | token << 16 of every masked column
  __shared__ uint32_t s_mlm[MODE == COLLATE_STATIC ? 4 : 1][MODE == COLLATE_STATIC ? COLLATE_MAX_LEN : 1];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t* mlm = s_mlm[MODE == COLLATE_STATIC ? w : 0];
  const int32_t L = P.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  // 16-B stores need every row of every output 16-B aligned
  const bool wide = (L & 1) == 0 && (((uintptr_t)P.input_ids | (uintptr_t)P.token_type_ids |
                                      (uintptr_t)P.attention_mask | (uintptr_t)P.labels) & 15) == 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    const int64_t g = pack_row(P, r);
    if (g < 0) {
      if (lane == 0) set_err(P.err, CERR_ROW_INDEX, r);
      continue;
    }
    const uint32_t fl = P.flags[g];
    if (!(fl & 2u)) {
      if (lane == 0) set_err(P.err, CERR_NO_SEP, r);
      continue;
    }
    RowShape S;
    S.a = P.len0[g];
    S.n = S.a + (int32_t)P.len1[g] + 3;
    if (S.n > L) {
      if (lane == 0) set_err(P.err, CERR_LONG, r);
      continue;
    }
    S.s0 = P.ids + P.src0[g] - 1;
    S.s1 = P.ids + P.src1[g] - (S.a + 2);
    if (MODE == COLLATE_STATIC) {
      __builtin_amdgcn_wave_barrier();  // the previous row's reads are done
      for (int32_t j = lane; j < L; j += 64) mlm[j] = kNoMask;
      __builtin_amdgcn_wave_barrier();
      bool bad = false;
      const int64_t k1 = P.mlm_off[g + 1];
      for (int64_t k = P.mlm_off[g] + lane; k < k1; k += 64) {
        const int32_t pos = P.mlm_pos[k];
        if (pos >= L) bad = true;
        else mlm[pos] = (uint32_t)P.mlm_label[k] | ((uint32_t)P.mlm_token[k] << 16);
      }
      if (__ballot(bad)) {
        if (lane == 0) set_err(P.err, CERR_POS_RANGE, r);
        continue;
      }
      __builtin_amdgcn_wave_barrier();
    }
    int64_t* o_ids = P.input_ids + r * (int64_t)L;
    int64_t* o_tt = P.token_type_ids + r * (int64_t)L;
    int64_t* o_am = P.attention_mask + r * (int64_t)L;
    int64_t* o_lab = P.labels + r * (int64_t)L;
    if (wide) {
      // two columns and one 16-B store per lane and output
      for (int32_t j = 2 * lane; j < L; j += 128) {
        const ColumnOut c0 = column<MODE>(P, S, mlm, r, j);
        const ColumnOut c1 = column<MODE>(P, S, mlm, r, j + 1);
        *reinterpret_cast<longlong2*>(o_ids + j) = make_longlong2(c0.id, c1.id);
        *reinterpret_cast<longlong2*>(o_tt + j) = make_longlong2(c0.tt, c1.tt);
        *reinterpret_cast<longlong2*>(o_am + j) = make_longlong2(c0.am, c1.am);
        *reinterpret_cast<longlong2*>(o_lab + j) = make_longlong2(c0.lab, c1.lab);
      }
    } else {
      for (int32_t j = lane; j < L; j += 64) {
        const ColumnOut c = column<MODE>(P, S, mlm, r, j);
        o_ids[j] = c.id;
        o_tt[j] = c.tt;
        o_am[j] = c.am;
        o_lab[j] = c.lab;
      }
    }
    if (lane == 0) P.next_sentence_labels[r] = fl & 1u;
  }
}

hipError_t launch_collate_rows_len(const CollateRowsParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  int64_t g = (P.n_rows + 255) / 256;
  if (g > (int64_t)n_cu * 8) g = (int64_t)n_cu * 8;
  hipLaunchKernelGGL(collate_rows_len_kernel, dim3((int)g), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_collate_rows(const CollateRowsParams& P, int32_t mode, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  int64_t g = (P.n_rows + 3) / 4;
  if (g > (int64_t)n_cu * 8) g = (int64_t)n_cu * 8;
  const dim3 grid((int)g), block(256);
  if (mode == COLLATE_SPECIAL_MASK) hipLaunchKernelGGL(collate_rows_kernel<COLLATE_SPECIAL_MASK>, grid, block, 0, s, P);
  else if (mode == COLLATE_STATIC) hipLaunchKernelGGL(collate_rows_kernel<COLLATE_STATIC>, grid, block, 0, s, P);
  else hipLaunchKernelGGL(collate_rows_kernel<COLLATE_DYNAMIC>, grid, block, 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
