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
// row of mode 1, as collate_rows_kernel.  A row starts at any 8-B aligned token
// offset, so the wave works on the 16-B aligned token pairs that cover
// [cu_seqlens[r], cu_seqlens[r] + n_r): a lane computes both tokens of a pair and
// stores 16 B per output; the first pair of a row with an odd start and the
// last pair of one with an odd end hold one token of this row and store 8 B.
// Outputs whose base is not 16-B aligned take the lane = token path.
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

// WWM (mode 2 only): whole-word masking, as in collate_rows_kernel.  A step of
// the wide path is the 128 tokens of 64 aligned pairs, the first of them -1
// (not a token of the row) when the row starts at an odd offset.
template <int MODE, bool CODE, bool WWM = false>
__global__ __launch_bounds__(256) void collate_unpadded_kernel(CollateUnpaddedParams P) {
  static_assert(!(CODE && MODE == COLLATE_STATIC), "CodeBERT rows have no static masks");
  static_assert(!WWM || MODE == COLLATE_DYNAMIC, "whole-word masking is dynamic masking");
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
    int64_t* o_ids = R.input_ids + c0;
    int64_t* o_tt = R.token_type_ids + c0;
    int64_t* o_pos = P.position_ids + c0;
    int64_t* o_lab = R.labels + c0;
    if constexpr (WWM) {
      int32_t carry = -1;
      if (wide) {
        const int32_t head = (int32_t)(c0 & 1);
        const int32_t nq = (head + n + 1) >> 1;
        for (int32_t qb = 0; qb < nq; qb += 64) {
          const int32_t q = qb + lane;
          const int32_t j0 = 2 * q - head, j1 = j0 + 1;
          const bool v0 = q < nq && j0 >= 0, v1 = q < nq && j1 < n;
          const WordColumn w0 = word_column(R, S, j0, v0, false);
          const WordColumn w1 = word_column(R, S, j1, v1, false);
          int32_t wh[2];
          word_heads<2>(2 * qb - head, {w0.start, w1.start}, carry, wh);
          const RowColumn t0 = row_column_word(R, S, r, j0, w0, wh[0]);
          const RowColumn t1 = row_column_word(R, S, r, j1, w1, wh[1]);
          if (v0 && v1) {
            *reinterpret_cast<longlong2*>(o_ids + j0) = make_longlong2(t0.id, t1.id);
            *reinterpret_cast<longlong2*>(o_tt + j0) = make_longlong2(t0.tt, t1.tt);
            *reinterpret_cast<longlong2*>(o_pos + j0) = make_longlong2(j0, j1);
            *reinterpret_cast<longlong2*>(o_lab + j0) = make_longlong2(t0.lab, t1.lab);
          } else if (v0 || v1) {
            const RowColumn t = v0 ? t0 : t1;
            const int32_t k = v0 ? j0 : j1;
            o_ids[k] = t.id;
            o_tt[k] = t.tt;
            o_pos[k] = k;
            o_lab[k] = t.lab;
          }
        }
      } else {
        for (int32_t base = 0; base < n; base += 64) {
          const int32_t j = base + lane;
          const WordColumn w0 = word_column(R, S, j, j < n, false);
          int32_t wh[1];
          word_heads<1>(base, {w0.start}, carry, wh);
          if (j < n) {
            const RowColumn t = row_column_word(R, S, r, j, w0, wh[0]);
            o_ids[j] = t.id;
            o_tt[j] = t.tt;
            o_pos[j] = j;
            o_lab[j] = t.lab;
          }
        }
      }
    } else if (wide) {
      // pair q holds tokens 2q - head and 2q - head + 1: 16-B aligned in the
      // stream.  The first pair of an odd start and the last of an odd end have
      // one token of this row (n >= 2: never the same pair, never neither).
      const int32_t head = (int32_t)(c0 & 1);
      const int32_t nq = (head + n + 1) >> 1;
      for (int32_t q = lane; q < nq; q += 64) {
        const int32_t j0 = 2 * q - head, j1 = j0 + 1;
        const bool v0 = j0 >= 0, v1 = j1 < n;
        const int32_t k0 = v0 ? j0 : 0, k1 = v1 ? j1 : n - 1;
        const RowColumn t0 = row_column<MODE>(R, S, mlm, r, k0, false);
        const RowColumn t1 = row_column<MODE>(R, S, mlm, r, k1, false);
        if (v0 && v1) {
          *reinterpret_cast<longlong2*>(o_ids + j0) = make_longlong2(t0.id, t1.id);
          *reinterpret_cast<longlong2*>(o_tt + j0) = make_longlong2(t0.tt, t1.tt);
          *reinterpret_cast<longlong2*>(o_pos + j0) = make_longlong2(j0, j1);
          *reinterpret_cast<longlong2*>(o_lab + j0) = make_longlong2(t0.lab, t1.lab);
        } else {
          const RowColumn t = v0 ? t0 : t1;
          const int32_t k = v0 ? k0 : k1;
          o_ids[k] = t.id;
          o_tt[k] = t.tt;
          o_pos[k] = k;
          o_lab[k] = t.lab;
        }
      }
    } else {
      for (int32_t j = lane; j < n; j += 64) {
        const RowColumn t = row_column<MODE>(R, S, mlm, r, j, false);
        o_ids[j] = t.id;
        o_tt[j] = t.tt;
        o_pos[j] = j;
        o_lab[j] = t.lab;
      }
    }
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
  if (mode == COLLATE_DYNAMIC && P.R.cont) {
    if (code) hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, true, true>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_unpadded_kernel<COLLATE_DYNAMIC, false, true>), grid, block, 0, s, P);
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
