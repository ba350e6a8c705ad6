// Fixed-shape padding-free collate from a pack result: the batch of
// collate_unpadded.hip in outputs whose sizes do not depend on the batch, in
// one launch.  tok_cap = T tokens, seq_cap = N sequence slots, max_seqlen = S.
//
// No counterpart in the reference (lddl/torch/bert.py:69-153 pads rows, not
// the stream).  With n rows of n_r tokens each and total = sum n_r:
//   [0, total), cu_seqlens[0 .. n], next_sentence_labels[0 .. n): the outputs of
//     collate_cu_*_kernel + collate_unpadded_kernel for the same rows, bit for
//     bit: the same open_row / stream_row (collate_row.h), the draw keyed by
//     (seed, counter, r, j)
//   [total, T): p = ceil((T - total) / S) pad sequences in slots n .. n + p - 1,
//     each of S tokens but the last; a pad token at offset j of its sequence is
//     input_ids 0, token_type_ids 0, position_ids j, labels ignore_index
//     (mode 0: special_tokens_mask 1)
//   cu_seqlens[r] = min(total + (r - n) * S, T) for n < r <= N: the pad
//     sequences, then empty slots at T;  next_sentence_labels[r] = ignore_index
//     for n <= r < N
//   status = {total, n, n + p, S};  *total_out = total in 64 bits
//
// One launch, no host read and no grid-wide sync.  A block takes a contiguous
// run of rows_per_block batch rows.  Offsets: every block sums row_tokens over
// the whole batch, once: the rows in front of its run give the stream offset of
// its first row, all of them give total, which every block needs for the slack.
// That is n * 5 B of len0 / len1 / flags (and 8 B of the index list) per block
// out of L2: two loads per thread for the 512 rows of a 65 536-token batch,
// cheaper than a second launch or a flag that the last block would publish and
// the others wait for.  Sums are 64-bit until the total is known to be within T.
// Then the block scans its run 256 rows at a time (wave_incl_add and the four
// wave totals in LDS), writes cu_seqlens and leaves each row's end in LDS.
//
// Fill: one wave per row, four rows of the run at a time, the per-wave LDS row
// of mode 1, stream_row for the tokens.  Slack: every thread of the grid takes
// its share of the pad tokens (16 B per lane per output when the bases are 16-B
// aligned; lane = token otherwise), of the cu_seqlens tail and of the
// next_sentence_labels tail.
//
// No input faults and nothing is stored outside the capacities: a row is
// stored only when it ends within T; total > T sets CERR_TOK_CAP, n + p > N
// CERR_SEQ_CAP (block 0, in the word behind the rows' error word, so that the
// host can report a row's error first; the slots that exist are still filled);
// a row longer than S is the row opener's CERR_LONG with S as the bound, and
// (mode 1) a static position >= n_r CERR_POS_RANGE; such a row is left
// unwritten.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {
namespace {

// the sum of x over the wave, in lane 63: two 16-bit halves, so that 64 values of 32 bits cannot overflow
__device__ __forceinline__ unsigned long long wave_total64(uint32_t x) {
  return (unsigned long long)wave_incl_add(x & 0xFFFFu) + ((unsigned long long)wave_incl_add(x >> 16) << 16);
}

}  // namespace

template <int MODE, bool CODE, int SEL = SEL_TOKEN>
__global__ __launch_bounds__(256) void collate_fixed_kernel(CollateFixedParams P) {
  static_assert(!(CODE && MODE == COLLATE_STATIC), "CodeBERT rows have no static masks");
  static_assert(SEL == SEL_TOKEN || MODE == COLLATE_DYNAMIC, "whole-word and span masking are dynamic masking");
  // mode 1 only: per wave, label | token << 16 of every masked token
  __shared__ uint32_t s_mlm[MODE == COLLATE_STATIC ? 4 : 1][MODE == COLLATE_STATIC ? COLLATE_MAX_LEN : 1];
  __shared__ unsigned long long s_sum[2];  // tokens in front of the block's run, tokens of the batch
  __shared__ uint32_t s_wave[4];
  __shared__ int64_t s_end[256];           // per row of the scan step: the end of its tokens in the stream
  const CollateRowsParams& R = P.R;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t* mlm = s_mlm[MODE == COLLATE_STATIC ? w : 0];
  const int64_t n = R.n_rows, T = P.tok_cap, N = P.seq_cap;
  const int32_t S = R.seq_len;
  const int64_t lo = min((int64_t)blockIdx.x * P.rows_per_block, n), hi = min(lo + P.rows_per_block, n);
  // 16-B stores need every output 16-B aligned at even token offsets
  const bool wide = (((uintptr_t)R.input_ids | (uintptr_t)R.token_type_ids | (uintptr_t)P.position_ids |
                      (uintptr_t)R.labels) & 15) == 0;

  // ---- offsets: the tokens in front of the run, and all of them --------------
  if (tid < 2) s_sum[tid] = 0;
  __syncthreads();
  {
    // a thread's share is n / 256 <= 2^12 rows of less than 2^18 tokens; an out-of-range row counts 0 here and in the
    // scan below, and is reported by the wave that opens it
    uint32_t below = 0, all = 0;
    for (int64_t r = tid; r < n; r += 256) {
      const int64_t g = pack_row(R, r);
      const uint32_t v = g < 0 ? 0u : row_tokens<CODE>(R, g);
      all += v;
      if (r < lo) below += v;
    }
    const unsigned long long b = wave_total64(below), a = wave_total64(all);
    if (lane == 63) {
      if (b) atomicAdd(&s_sum[0], b);
      atomicAdd(&s_sum[1], a);
    }
  }
  __syncthreads();
  const int64_t total = (int64_t)s_sum[1];
  const int64_t slack = T - total;                          // < 0: refused
  const int64_t n_pad = slack > 0 ? (slack + S - 1) / S : 0;  // p
  if (blockIdx.x == 0 && tid == 0) {
    // (a word of their own: the host reports a row's error before these, whichever block was first)
    if (total > T) R.err[1] = CERR_TOK_CAP;
    else if (n + n_pad > N) R.err[1] = CERR_SEQ_CAP;
    *P.total_out = total;
    P.status[0] = (int32_t)min(total, (int64_t)INT32_MAX);
    P.status[1] = (int32_t)n;
    P.status[2] = (int32_t)(n + n_pad);
    P.status[3] = S;
    P.cu_seqlens[0] = 0;
  }

  // ---- the run: scan 256 rows, then fill them, one wave per row ---------------
  int64_t carry = (int64_t)s_sum[0];
  for (int64_t r0 = lo; r0 < hi; r0 += 256) {
    const int64_t r = r0 + tid;
    uint32_t v = 0;
    if (r < hi) {
      const int64_t g = pack_row(R, r);
      if (g >= 0) v = row_tokens<CODE>(R, g);
    }
    const uint32_t incl = wave_incl_add(v);
    if (lane == 63) s_wave[w] = incl;
    __syncthreads();
    uint32_t before = 0, step = 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = s_wave[k];
      step += x;
      if (k < w) before += x;
    }
    const int64_t end = carry + before + incl;
    carry += step;
    s_end[tid] = end;
    if (r < hi && end <= T) P.cu_seqlens[r + 1] = (int32_t)end;  // (T <= INT32_MAX: narrowed only when it fits)
    __syncthreads();
    const int m = (int)min((int64_t)256, hi - r0);
    for (int t = w; t < m; t += 4) {
      const int64_t rr = r0 + t;
      OpenRow O;
      uint32_t code = open_row<CODE>(R, rr, S, O);
      // the bound is n_r: [n_r, ..) would be the next row here
      if (MODE == COLLATE_STATIC && !code && !stage_static_masks(R, O.g, O.L.n, mlm)) code = CERR_POS_RANGE;
      if (code) {
        if (lane == 0) set_err(R.err, code, rr);
        continue;
      }
      const int64_t c1 = s_end[t];
      if (c1 > T) continue;  // the batch passes tok_cap (block 0 says so): a row that would pass it is not stored
      stream_row<MODE, SEL>(R, O, mlm, rr, c1 - O.L.n, wide, P.position_ids);
      if (!CODE && lane == 0) R.next_sentence_labels[rr] = O.flags & 1u;
    }
    // (the next step's s_wave / s_end are written behind its first barrier / after every wave has left this loop)
  }

  // ---- the slack, shared by every thread of the grid -------------------------
  const int64_t gt = (int64_t)blockIdx.x * 256 + tid, G = (int64_t)gridDim.x * 256;
  const int64_t pad_lab = MODE == COLLATE_SPECIAL_MASK ? 1 : R.ignore_index;
  if (slack > 0) {  // pad token t sits at offset (t - total) % S of its pad sequence; the slack is below 2^31
    const auto pad_one = [&](int64_t t) {
      R.input_ids[t] = 0;
      R.token_type_ids[t] = 0;
      P.position_ids[t] = (int64_t)((uint32_t)(t - total) % (uint32_t)S);
      R.labels[t] = pad_lab;
    };
    if (wide) {
      const int64_t t0 = total + (total & 1);  // the first 16-B aligned pair; t0 <= T
      const int64_t n_pair = (T - t0) >> 1;
      if ((total & 1) && gt == 0) pad_one(total);
      if (((T - t0) & 1) && gt == G - 1) pad_one(T - 1);
      const longlong2 zero = make_longlong2(0, 0), labs = make_longlong2(pad_lab, pad_lab);
      for (int64_t q = gt; q < n_pair; q += G) {
        const int64_t t = t0 + 2 * q;
        const uint32_t j0 = (uint32_t)(t - total) % (uint32_t)S;
        const uint32_t j1 = j0 + 1 == (uint32_t)S ? 0u : j0 + 1;
        *reinterpret_cast<longlong2*>(R.input_ids + t) = zero;
        *reinterpret_cast<longlong2*>(R.token_type_ids + t) = zero;
        *reinterpret_cast<longlong2*>(P.position_ids + t) = make_longlong2((int64_t)j0, (int64_t)j1);
        *reinterpret_cast<longlong2*>(R.labels + t) = labs;
      }
    } else {
      for (int64_t t = total + gt; t < T; t += G) pad_one(t);
    }
  }
  // slots n + 1 .. N: the ends of the pad sequences, then T (also when the batch is refused: within N either way)
  for (int64_t r = n + 1 + gt; r <= N; r += G) P.cu_seqlens[r] = (int32_t)min(total + (r - n) * S, T);
  if (!CODE)
    for (int64_t r = n + gt; r < N; r += G) R.next_sentence_labels[r] = R.ignore_index;
}

hipError_t launch_collate_fixed(const CollateFixedParams& P0, bool code, int32_t mode, int n_cu, hipStream_t s) {
  if (P0.R.n_rows <= 0) return hipSuccess;
  CollateFixedParams P = P0;
  // a wave per row, and enough blocks for the slack of a short batch: a wave per 256 tokens of tok_cap
  const int64_t n = P.R.n_rows;
  const int g = grid_rows(n > P.tok_cap / 256 ? n : P.tok_cap / 256, n_cu);
  P.rows_per_block = ((n + g - 1) / g + 3) & ~(int64_t)3;
  const dim3 grid(g), block(256);
  const int sel = mode == COLLATE_DYNAMIC ? collate_sel(P.R.cont, P.R.span) : SEL_TOKEN;
  if (sel == SEL_SPAN) {
    if (code) hipLaunchKernelGGL((collate_fixed_kernel<COLLATE_DYNAMIC, true, SEL_SPAN>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_fixed_kernel<COLLATE_DYNAMIC, false, SEL_SPAN>), grid, block, 0, s, P);
  } else if (sel == SEL_WORD) {
    if (code) hipLaunchKernelGGL((collate_fixed_kernel<COLLATE_DYNAMIC, true, SEL_WORD>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_fixed_kernel<COLLATE_DYNAMIC, false, SEL_WORD>), grid, block, 0, s, P);
  } else if (code) {
    dispatch_code_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_fixed_kernel<decltype(m)::value, true>), grid, block, 0, s, P);
    });
  } else {
    dispatch_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_fixed_kernel<decltype(m)::value, false>), grid, block, 0, s, P);
    });
  }
  return hipGetLastError();
}

}  // namespace lddl
