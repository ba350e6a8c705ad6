// Text-infilling collate (BART's denoising objective over a WordPiece
// vocabulary; include/lddl_amd.h defines it with lddl_infill_params): every
// selected span of a row collapses to one [MASK], so the encoder input is
// shorter than the row, and the decoder is teacher-forced on the row itself.
// The rows are CodeBERT / MLM-only rows of a row table, opened as
// collate_rows.hip opens them; the selection is span masking's (span_select,
// collate_dev.h) under a Poisson length law.  No counterpart in the reference,
// whose BART preprocessor stops at the text column.
//
// This is the one collate that changes a row's length: an ordered compaction
// per row.  Work mapping: one wave per batch row, four rows per block, no
// block-wide barrier (collate_rows.hip's).  The wave walks the row 64 columns a
// step, lane = column:
//   select   word_column + span_select, the span state carried from step to
//            step as there
//   emit     a column is dropped iff it and the column before it are selected.
//            Both are bits of the step's ballot of `selected`: shifted up by
//            one, with the last lane's bit of the step before (wave-uniform)
//            shifted in at lane 0, the mask is every lane's "the column before
//            me is selected".  No lane exchange
//   place    the emitted column's place in the output is the row's running
//            count + the emit ballot's bits below the lane (v_mbcnt)
//   stage    the emitted token ([MASK] or the id) goes to that place of the
//            wave's LDS slice as uint16: 2048 x 2 B = 4 KiB per wave, 16 KiB per
//            block.  The places are arbitrary, so nothing is scattered to
//            global memory
// After the last step the wave streams the encoder's planes out of the slice
// and the decoder's planes out of the row table (the row's ids shifted by one:
// 2-B loads at known addresses, L2 hits after the walk), every plane with
// 16-B stores of the token pairs that are 16-B aligned in it (store_tokens).
// A row of the padded batch is its seq_len columns, padding included; a row of
// the padding-free streams starts at any token offset, and the first pair of an
// odd start and the last of an odd end store 8 B.
//
// Padding-free route: the count pass runs the same walk without staging and
// leaves e_r and n_r - 1 in the two offset arrays, with the sums of every chunk
// of kChunk rows; the second level is collate_row.h's chunked scan over two
// quantities, in place.  The fill pass runs the walk again (the hashes are
// cheaper than a plane of selection bits written and read back), checks its
// count and both offset pairs against the streams' capacities before it stores
// anything, and fills both streams.
//
// No input faults: the row opener's checks come first (a row index is
// range-checked before anything is loaded through it); a refused row sets the
// error word and is left unwritten; no row stores outside its own tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "collate_tokens.h"
#include "wave.h"

namespace lddl {
namespace {

// infill_walk (collate_tokens.h) over the row table itself, every run collapsing to [MASK]
template <bool STAGE>
__device__ __forceinline__ int32_t infill_row(const CollateRowsParams& P, const OpenRow& R, int64_t r, uint16_t* tok) {
  return infill_walk<STAGE>(
      P, R, r, tok, [&](int32_t k) { return (int32_t)(k <= R.L.a ? R.s0[k] : R.s1[k]); },
      [&](int32_t) { return P.mask_id; });
}

// ------------------------------------------------------------- padded batch --
__global__ __launch_bounds__(256) void infill_rows_kernel(CollateInfillParams P) {
  __shared__ uint16_t s_tok[4][COLLATE_MAX_LEN];
  const CollateRowsParams& R = P.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t* tok = s_tok[w];
  const int32_t L = R.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const enc[2] = {R.input_ids, R.attention_mask};
  int64_t* const dec[2] = {P.decoder_input_ids, R.labels};
  const bool wide_enc = planes_aligned(enc), wide_dec = planes_aligned(dec);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, L, S);
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    wave_sync();  // the reads of the row before are done
    const int32_t e = infill_row<true>(R, S, r, tok);  // e <= n <= L <= COLLATE_MAX_LEN
    wave_sync();
    const int64_t c0 = r * (int64_t)L;
    store_tokens<2>(enc, c0, L, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < e ? (int64_t)tok[j] : 0;
      v[1] = j < e ? 1 : 0;
    });
    const int32_t m = S.L.n - 1;
    store_tokens<2>(dec, c0, L, wide_dec, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < m ? row_id(R, S, j) : 0;
      v[1] = j < m ? row_id(R, S, j + 1) : R.ignore_index;
    });
    if (lane == 0) P.enc_len[r] = e;
  }
}

// ------------------------------------------------------- padding-free batch --
// e_r and n_r - 1 of every batch row into cu_enc[r + 1] and cu_dec[r + 1], their chunk sums and maxima.  A refused
// row sets the error word and counts 0 in both.
__global__ __launch_bounds__(256) void infill_count_kernel(CollateInfillParams P) {
  const CollateRowsParams& R = P.R;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    int32_t e = 0, m = 0;
    if (!code) {
      e = infill_row<false>(R, S, r, nullptr);
      m = S.L.n - 1;
    }
    if (lane == 0) {
      if (code) set_err(R.err, code, r);
      P.cu_enc[r + 1] = e;
      P.cu_dec[r + 1] = m;
      if (!code) {  // e >= 2 and m >= 1
        uint32_t* sum = P.chunk_sum + 2 * (r / kChunk);
        atomicAdd(&sum[0], (uint32_t)e);
        atomicAdd(&sum[1], (uint32_t)m);
        atomicMax(&P.max_out[0], e);
        atomicMax(&P.max_out[1], m);
      }
    }
  }
}

// the second level of both scans, in place; nothing is narrowed while a total does not fit int32
__global__ __launch_bounds__(256) void infill_scan_kernel(CollateInfillParams P) {
  __shared__ ChunkScanLds<2> S;
  chunk_scan_bases(S, P.n_chunks, [&](int64_t c, unsigned long long(&q)[2]) {
    q[0] = P.chunk_sum[2 * c];
    q[1] = P.chunk_sum[2 * c + 1];
  });
  const int64_t te = (int64_t)S.total[0], td = (int64_t)S.total[1];
  const bool fits = te < (1ll << 31) && td < (1ll << 31);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    P.totals_out[0] = te;
    P.totals_out[1] = td;
    if (fits) P.cu_enc[0] = P.cu_dec[0] = 0;
  }
  if (!fits) return;  // refused on the host
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  int64_t carry[2] = {(int64_t)S.base[0], (int64_t)S.base[1]}, end[2];
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    uint32_t v[2] = {0, 0};
    if (r < P.R.n_rows) {
      v[0] = (uint32_t)P.cu_enc[r + 1];
      v[1] = (uint32_t)P.cu_dec[r + 1];
    }
    chunk_scan_step(S, it, v, carry, end);
    if (r < P.R.n_rows) {
      P.cu_enc[r + 1] = (int32_t)end[0];
      P.cu_dec[r + 1] = (int32_t)end[1];
    }
  }
}

__global__ __launch_bounds__(256) void infill_unpadded_kernel(CollateInfillParams P) {
  __shared__ uint16_t s_tok[4][COLLATE_MAX_LEN];
  const CollateRowsParams& R = P.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t* tok = s_tok[w];
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const enc[2] = {R.input_ids, P.position_ids};
  int64_t* const dec[3] = {P.decoder_input_ids, R.labels, P.decoder_position_ids};
  const bool wide_enc = planes_aligned(enc), wide_dec = planes_aligned(dec);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    int32_t e = 0, m = 0;
    int64_t c0 = 0, d0 = 0;
    if (!code) {
      // the offsets are checked, not trusted: the decoder's against n_r - 1, the encoder's against the walk's count
      m = S.L.n - 1;
      c0 = P.cu_enc[r];
      d0 = P.cu_dec[r];
      const int64_t c1 = P.cu_enc[r + 1], d1 = P.cu_dec[r + 1];
      if (c0 < 0 || c1 < c0 || c1 - c0 > S.L.n || c1 > P.total_enc || d0 < 0 || d1 - d0 != m || d0 + m > P.total_dec) {
        code = CERR_CU_SEQLENS;
      } else {
        wave_sync();  // the reads of the row before are done
        e = infill_row<true>(R, S, r, tok);
        wave_sync();
        if (e != c1 - c0) code = CERR_CU_SEQLENS;
      }
    }
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    store_tokens<2>(enc, c0, e, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = tok[j];
      v[1] = j;
    });
    store_tokens<3>(dec, d0, m, wide_dec, [&](int32_t j, int64_t(&v)[3]) {
      v[0] = row_id(R, S, j);
      v[1] = row_id(R, S, j + 1);
      v[2] = j;
    });
  }
}

}  // namespace

hipError_t launch_infill_rows(const CollateInfillParams& P, int n_cu, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(infill_rows_kernel, dim3(grid_rows(P.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_infill_cu_seqlens(const CollateInfillParams& P, int n_cu, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(infill_count_kernel, dim3(grid_rows(P.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return launch_infill_scan(P, s);
}

// the second level alone, for collate_corrupt.hip's count pass, which leaves the same fields as infill_count_kernel
hipError_t launch_infill_scan(const CollateInfillParams& P, hipStream_t s) {
  hipLaunchKernelGGL(infill_scan_kernel, dim3((unsigned)P.n_chunks), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_infill_unpadded(const CollateInfillParams& P, int n_cu, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(infill_unpadded_kernel, dim3(grid_rows(P.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
