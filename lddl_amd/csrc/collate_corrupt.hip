// Span-corruption collate (T5's denoising objective, also CodeT5's and UL2's R / X denoisers, over a WordPiece
// vocabulary; include/lddl_amd.h defines it): the k-th selected run of a row becomes sentinel k in the encoder
// input, and the target is sentinel_0 span_0 sentinel_1 span_1 ... [SEP].  Rows, selection and law are text
// infilling's (collate_infill.hip); no counterpart in the reference.
//
// Two ordered compactions per row, both shorter than the row or as long: the encoder's e_r tokens and the target's
// t_r.  Work mapping as collate_infill.hip: one wave per batch row, four rows per block, no block-wide barrier,
// lane = column, 64 columns a step.  Per step, all from ballots (wave-uniform 64-bit masks) and v_mbcnt:
//   open     selected, and the column before is not: the ballot of `selected` and-not itself shifted up by one,
//            with the last lane's bit of the step before shifted in at lane 0.  A run that continues from the step
//            before opens nothing here; a run that begins at lane 0 does
//   ordinal  of the run a selected column lies in: the runs opened in the steps before (a wave-uniform count) + the
//            open ballot's bits at or below the lane - 1
//   corrupt  selected and ordinal < num_sentinels.  A run is corrupted as a whole (its columns share the ordinal),
//            so "opens a corrupted run" is open and corrupt, and the places below count bits of the corrupt
//            ballots, never of `selected`
//   encoder  a column is dropped iff it is corrupt and does not open; place = running e + emit bits below the lane;
//            the token is the sentinel or the id
//   target   a corrupt column's id goes to running t + corrupt bits below the lane + corrupt-open bits at or below
//            it; a lane that opens writes its sentinel one place in front.  One lane appends [SEP] after the walk
// Both streams are staged as uint16 in LDS slices of COLLATE_MAX_LEN entries (t_r <= n and e_r <= n: the header
// says why), two slices per wave, 32 KiB per block; DESIGN.md 4f weighs that against one slice and two walks.
// decoder_input_ids is the target slice read one place back with [CLS] in front.  After the walk the wave streams
// every plane out of the slices with store_tokens' 16-B stores, padded rows and both padding-free streams alike.
//
// Padding-free route: the count pass is the walk without staging; it leaves e_r and t_r where infill's count pass
// leaves e_r and n_r - 1, so the second level is infill's scan kernel as it is.  The fill walks again and compares
// both counts with both offset pairs before it stores anything.
//
// No input faults: the row opener's checks come first; a refused row sets the error word and is left unwritten; no
// row stores outside its own tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "collate_tokens.h"
#include "wave.h"

namespace lddl {
namespace {

// The walk of open batch row r by its wave.  With STAGE the encoder's tokens are left in enc[0, e) and the target
// in tgt[0, t).  e <= n and t <= n: the caller's bound on n is the bound on what is written.  The placement of a
// step is corrupt_step (collate_tokens.h), shared with collate_segment.hip.
template <bool STAGE>
__device__ __forceinline__ CorruptLen corrupt_row(const CollateCorruptParams& P, const OpenRow& R, int64_t r,
                                                  uint16_t* enc, uint16_t* tgt) {
  const CollateRowsParams& C = P.I.R;
  const int lane = threadIdx.x & 63;
  const int32_t n = R.L.n;
  SpanCarry carry;
  CorruptWalk w;
  for (int32_t base = 0; base < n; base += 64) {
    const int32_t j = base + lane;
    const WordColumn c = word_column(C, R, j, j < n, false);
    const bool st[1] = {c.start}, sp[1] = {c.special};
    bool sel[1];  // false on a special column and behind the row
    span_select<1>(C.span, C.seed, C.counter, r, base, st, sp, carry, sel);
    corrupt_step<STAGE>(P, __ballot(sel[0]), sel[0], j < n, (uint16_t)c.id, w, enc, tgt);
  }
  return corrupt_finish<STAGE>(C.sep, w, tgt);
}

// ------------------------------------------------------------- padded batch --
__global__ __launch_bounds__(256) void corrupt_rows_kernel(CollateCorruptParams P) {
  __shared__ uint16_t s_tok[4][2][COLLATE_MAX_LEN];
  const CollateRowsParams& R = P.I.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t *enc = s_tok[w][0], *tgt = s_tok[w][1];
  const int32_t L = R.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const eo[2] = {R.input_ids, R.attention_mask};
  int64_t* const dout[2] = {P.I.decoder_input_ids, R.labels};
  const bool wide_enc = planes_aligned(eo), wide_dec = planes_aligned(dout);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, L, S);
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    wave_sync();  // the reads of the row before are done
    const CorruptLen n = corrupt_row<true>(P, S, r, enc, tgt);  // e, t <= n_r <= L <= COLLATE_MAX_LEN
    wave_sync();
    const int64_t c0 = r * (int64_t)L;
    store_tokens<2>(eo, c0, L, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < n.e ? (int64_t)enc[j] : 0;
      v[1] = j < n.e ? 1 : 0;
    });
    store_tokens<2>(dout, c0, L, wide_dec, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = 0;
      v[1] = R.ignore_index;
      if (j < n.t) decoder_token(tgt, R.cls, j, v[0], v[1]);
    });
    if (lane == 0) {
      P.I.enc_len[r] = n.e;
      P.dec_len[r] = n.t;
    }
  }
}

// ------------------------------------------------------- padding-free batch --
// e_r and t_r of every batch row into cu_enc[r + 1] and cu_dec[r + 1], their chunk sums and maxima: what
// infill_scan_kernel sums.  A refused row sets the error word and counts 0 in both.
__global__ __launch_bounds__(256) void corrupt_count_kernel(CollateCorruptParams P) {
  const CollateRowsParams& R = P.I.R;
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    CorruptLen n{0, 0};
    if (!code) n = corrupt_row<false>(P, S, r, nullptr, nullptr);
    if (lane == 0) {
      if (code) set_err(R.err, code, r);
      P.I.cu_enc[r + 1] = n.e;
      P.I.cu_dec[r + 1] = n.t;
      if (!code) {  // e >= 2 and t >= 1
        uint32_t* sum = P.I.chunk_sum + 2 * (r / kChunk);
        atomicAdd(&sum[0], (uint32_t)n.e);
        atomicAdd(&sum[1], (uint32_t)n.t);
        atomicMax(&P.I.max_out[0], n.e);
        atomicMax(&P.I.max_out[1], n.t);
      }
    }
  }
}

__global__ __launch_bounds__(256) void corrupt_unpadded_kernel(CollateCorruptParams P) {
  __shared__ uint16_t s_tok[4][2][COLLATE_MAX_LEN];
  const CollateInfillParams& I = P.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t *enc = s_tok[w][0], *tgt = s_tok[w][1];
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const eo[2] = {R.input_ids, I.position_ids};
  int64_t* const dout[3] = {I.decoder_input_ids, R.labels, I.decoder_position_ids};
  const bool wide_enc = planes_aligned(eo), wide_dec = planes_aligned(dout);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    CorruptLen n{0, 0};
    int64_t c0 = 0, d0 = 0;
    if (!code) {
      // the offsets are checked, not trusted: each side against the stream's capacity first, then against the
      // walk's own count, before anything of the row is stored
      c0 = I.cu_enc[r];
      d0 = I.cu_dec[r];
      const int64_t c1 = I.cu_enc[r + 1], d1 = I.cu_dec[r + 1];
      if (!offsets_ok(c0, c1, S.L.n, I.total_enc) || !offsets_ok(d0, d1, S.L.n, I.total_dec)) {
        code = CERR_CU_SEQLENS;
      } else {
        wave_sync();  // the reads of the row before are done
        n = corrupt_row<true>(P, S, r, enc, tgt);
        wave_sync();
        if (n.e != c1 - c0 || n.t != d1 - d0) code = CERR_CU_SEQLENS;
      }
    }
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    store_tokens<2>(eo, c0, n.e, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = enc[j];
      v[1] = j;
    });
    store_tokens<3>(dout, d0, n.t, wide_dec, [&](int32_t j, int64_t(&v)[3]) {
      decoder_token(tgt, R.cls, j, v[0], v[1]);
      v[2] = j;
    });
  }
}

}  // namespace

hipError_t launch_corrupt_rows(const CollateCorruptParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(corrupt_rows_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_corrupt_cu_seqlens(const CollateCorruptParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(corrupt_count_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_infill_scan(P.I, s);
}

hipError_t launch_corrupt_unpadded(const CollateCorruptParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(corrupt_unpadded_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
