// Padding-free collate from a pack result: the batch of collate_rows.hip with
// the pad columns removed.  The rows are concatenated into one token stream,
// row r at [cu_seqlens[r], cu_seqlens[r + 1]), which is what variable-length
// attention kernels take; there is no attention_mask and a position_ids
// stream instead.
//
// No counterpart in the reference (lddl/torch/bert.py:69-153 pads).  Defined
// by the padded batch: with batch row r = pack row g = rows[r] (rows NULL:
// row0 + r), a = len0[g], b = len1[g], n_r = a + b + 3 and t = cu_seqlens[r] + j,
// 0 <= j < n_r:
//   input_ids[t], token_type_ids[t], labels[t] = column j of row r of
//     lddl_collate_rows at the same mode, seed and counter (the dynamic draw is
//     keyed by (seed, counter, r, j), not by seq_len): the same row_column
//     (collate_row.h), never on a pad column
//   position_ids[t] = j;  next_sentence_labels[r] = flags[g] & 1
//
// With CODE the rows are CodeBERT rows (lddl_collate_code_rows_unpadded), as in
// collate_rows.hip: n_r = a + b + 2 + s with s = flags bit 1, modes 0 and 2, no
// next_sentence_labels.
//
// Offsets pass: cu_seqlens is an exclusive scan of n_r, the chunked scan of
// collate_row.h over one quantity: every block sums its chunk of kChunk rows
// (collate_cu_sum_kernel), then collate_cu_scan_kernel is the second level.
// Sums are 64-bit until the total is known to be below 2^31; otherwise nothing
// is written.  A batch is thousands of rows, so this is two launches of a few
// blocks: launch-bound.
//
// Fill pass: one wave per batch row, four rows per block and the per-wave LDS
// row of mode 1, as collate_rows_kernel.  The row's tokens are stream_row's
// (collate_row.h): 16-B aligned token pairs over [cu_seqlens[r], cu_seqlens[r] +
// n_r), or lane = token when an output base is not 16-B aligned.
//
// No input faults: cu_seqlens is not trusted.  A row whose offsets are not
// [c, c + n_r) within [0, total) sets CERR_CU_SEQLENS; the row opener's checks
// come first, with COLLATE_MAX_LEN as the bound, and (mode 1) a static
// position >= n_r after it; such a row is left unwritten.  No row stores
// outside its own tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {
namespace {

template <bool CODE>
__global__ __launch_bounds__(256) void collate_cu_sum_kernel(CollateUnpaddedParams P) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  uint32_t s = 0, m = 0;
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    if (r < P.R.n_rows) {
      // an out-of-range row sets the error word and counts 0
      const int64_t g = pack_row(P.R, r);
      if (g < 0) set_err(P.R.err, CERR_ROW_INDEX, r);
      const uint32_t v = g < 0 ? 0u : row_tokens<CODE>(P.R, g);
      s += v;
      m = max(m, v);
    }
  }
  s = wave_incl_add(s);
  m = wave_incl_max(m);
  if ((threadIdx.x & 63) == 63) {
    atomicAdd(&s_sum, s);
    if (m) atomicMax(P.R.max_len, (int32_t)m);
  }
  __syncthreads();
  if (threadIdx.x == 0) P.chunk_sum[blockIdx.x] = s_sum;
}

template <bool CODE>
__global__ __launch_bounds__(256) void collate_cu_scan_kernel(CollateUnpaddedParams P) {
  __shared__ ChunkScanLds<1> S;
  chunk_scan_bases(S, P.n_chunks, [&](int64_t c, unsigned long long (&q)[1]) { q[0] = P.chunk_sum[c]; });
  const int64_t total = (int64_t)S.total[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *P.total_out = total;
    if (total < (1ll << 31)) P.cu_seqlens[0] = 0;
  }
  if (total >= (1ll << 31)) return;  // refused on the host; nothing narrowed
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  int64_t carry[1] = {(int64_t)S.base[0]}, end[1];
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    // the error word was set by the sum pass; an out-of-range row counts 0 in both
    uint32_t v[1] = {0};
    if (r < P.R.n_rows) {
      const int64_t g = pack_row(P.R, r);
      if (g >= 0) v[0] = row_tokens<CODE>(P.R, g);
    }
    chunk_scan_step(S, it, v, carry, end);
    if (r < P.R.n_rows) P.cu_seqlens[r + 1] = (int32_t)end[0];
  }
}

}  // namespace

// SEL (mode 2 only): tokens, whole words or spans, as in collate_rows_kernel.  The row's tokens: stream_row (collate_row.h).
template <int MODE, bool CODE, int SEL = SEL_TOKEN>
__global__ __launch_bounds__(256) void collate_unpadded_kernel(CollateUnpaddedParams P) {
  static_assert(!(CODE && MODE == COLLATE_STATIC), "CodeBERT rows have no static masks");
  static_assert(SEL == SEL_TOKEN || MODE == COLLATE_DYNAMIC, "whole-word and span masking are dynamic masking");
  // mode 1 only: per wave, label | token << 16 of every masked token
  __shared__ uint32_t s_mlm[MODE == COLLATE_STATIC ? 4 : 1][MODE == COLLATE_STATIC ? COLLATE_MAX_LEN : 1];
  const CollateRowsParams& R = P.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t* mlm = s_mlm[MODE == COLLATE_STATIC ? w : 0];
  const int64_t nw = (int64_t)gridDim.x * 4;
  // 16-B stores need every output 16-B aligned at even token offsets
  const bool wide = (((uintptr_t)R.input_ids | (uintptr_t)R.token_type_ids | (uintptr_t)P.position_ids |
                      (uintptr_t)R.labels) & 15) == 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    uint32_t code = open_row<CODE>(R, r, COLLATE_MAX_LEN, S);
    int32_t n = 0;
    int64_t c0 = 0;
    if (!code) {
      n = S.L.n;
      c0 = P.cu_seqlens[r];
      const int64_t c1 = P.cu_seqlens[r + 1];
      if (c0 < 0 || c1 - c0 != n || c0 + n > P.total) code = CERR_CU_SEQLENS;
    }
    // the bound is n: [n, seq_len) of the padded row would be the next row here
    if (MODE == COLLATE_STATIC && !code && !stage_static_masks(R, S.g, n, mlm)) code = CERR_POS_RANGE;
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    stream_row<MODE, SEL>(R, S, mlm, r, c0, wide, P.position_ids);
    if (!CODE && lane == 0) R.next_sentence_labels[r] = S.flags & 1u;
  }
}

hipError_t launch_collate_cu_seqlens(const CollateUnpaddedParams& P, bool code, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)P.n_chunks), block(256);
  if (code) {
    hipLaunchKernelGGL(collate_cu_sum_kernel<true>, grid, block, 0, s, P);
    hipLaunchKernelGGL(collate_cu_scan_kernel<true>, grid, block, 0, s, P);
  } else {
    hipLaunchKernelGGL(collate_cu_sum_kernel<false>, grid, block, 0, s, P);
    hipLaunchKernelGGL(collate_cu_scan_kernel<false>, grid, block, 0, s, P);
  }
  return hipGetLastError();
}

hipError_t launch_collate_unpadded(const CollateUnpaddedParams& P, bool code, int32_t mode, int n_cu, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  const dim3 grid(grid_rows(P.R.n_rows, n_cu)), block(256);
  const int sel = mode == COLLATE_DYNAMIC ? collate_sel(P.R.cont, P.R.span) : SEL_TOKEN;
  if (sel == SEL_SPAN) {
    if (code) hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, true, SEL_SPAN>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, false, SEL_SPAN>), grid, block, 0, s, P);
  } else if (sel == SEL_WORD) {
    if (code) hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, true, SEL_WORD>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, false, SEL_WORD>), grid, block, 0, s, P);
  } else if (code) {
    dispatch_code_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_unpadded_kernel<decltype(m)::value, true>), grid, block, 0, s, P);
    });
  } else {
    dispatch_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_unpadded_kernel<decltype(m)::value, false>), grid, block, 0, s, P);
    });
  }
  return hipGetLastError();
}

}  // namespace lddl
