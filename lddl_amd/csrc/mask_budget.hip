// Exact-count dynamic masking (lddl_set_mask_budget; include/lddl_amd.h defines
// it): the per-row threshold that the fill kernels test their rank keys
// against.  The reference has this rule in its static path only
// (pretrain.py:182-238 `create_masked_lm_predictions`: a shuffle of the
// candidates, cut at max(1, round(len * ratio))); here it is a selection over
// the counter-based draws of the dynamic path, so that every route and the
// fill agree on it without a sort or a list.
//
// For batch row r the units are its non-special columns (token mode) or its
// words (whole-word mode: weight = tokens of the word, identified by the head
// column).  Unit h has the 64-bit key R(r, h) = budget_key (collate_dev.h),
// unique within the row.  thr[r] is the smallest key that is not selected:
// the units below it are the longest prefix in ascending key order whose
// weights sum to at most budget.  No unit at or above thr[r]: UINT64_MAX
// (no key is that: its low 20 bits would be a column of 2^20 - 1).
//
// Work mapping: one wave per row, four rows per block, no block-wide
// barrier.  An MSD radix select on weights, eight bits a level:
//   histogram  the wave walks the row 64 columns a step; a non-special column
//              whose head's key carries the prefix found so far adds, with
//              one LDS atomic, weight 1 (low word) and "a head is here" (high
//              word) to the bin of the key's next eight bits.  256 bins of
//              8 B per wave: the weights and the heads of a bin reach the row
//              length each, and lddl_mask_tokens takes rows of up to 2^20
//              columns, so neither fits a half word.
//   scan       lane l owns bins 4 l .. 4 l + 3: their weights summed, an
//              inclusive wave scan (wave.h, DPP), and the first bin B whose
//              cumulative weight passes what is left of the budget, by ballot.
//   descend    no such bin: everything is taken (level 0 only: below it the
//              bin's weight is known to pass).  B holds one head, or nothing
//              is left: the first unit of B does not fit, thr = B's lowest
//              key.  Otherwise the weight in front of B is spent, B joins the
//              prefix, next level.  Keys are unique, so a bin of the eighth
//              level holds one head at most and the search ends there.
// The hashes are computed again at every level: one splitmix64 per column
// against 2048 x 8 B of registers or LDS per row.  The ids (whole-word mode
// reads them for "##") are read again as well: 2 B a column out of L2, which
// the first level has just filled; holding them would take 4 KiB of LDS per
// wave and halve the waves per CU for a kernel whose second level is the
// expected last one.  Columns of a row table come from open_row / word_column
// (collate_row.h), those of lddl_mask_tokens from the caller's planes.
// No global atomics, no stores but thr[r].
//
// No input faults: a row that open_row refuses gets thr 0 and is left to the
// fill, which reports it; nothing is read through a row index before its
// range check.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {
namespace {

constexpr uint64_t kTakeAll = ~0ull;

// min(max_predictions, c, max(1, rint(c * p))), 0 for c = 0: the product in double, round-half-even
__device__ __forceinline__ uint32_t row_budget(uint32_t c, double p, int32_t max_predictions) {
  if (c == 0) return 0;
  const double want = fmax(1.0, rint((double)c * p));  // <= c < 2^20: exact in double
  return min(min((uint32_t)max_predictions, c), (uint32_t)want);
}

// thr of one row of n columns, by the whole wave.  flags(base, special, start): of column base + lane, called by
// every lane for the steps of the row in ascending order, at every level (special: true behind the row; start is
// read in whole-word mode only).  hist: the wave's 256 bins.
template <bool WORD, class Flags>
__device__ __forceinline__ uint64_t budget_threshold(int32_t n, int64_t row, uint64_t k, double p,
                                                     int32_t max_predictions, unsigned long long* hist, Flags flags) {
  const int lane = threadIdx.x & 63;
  uint64_t prefix = 0;  // the digits found so far
  uint32_t left = 0;    // what is left of the budget for the units under the prefix
  for (int level = 0; level < 8; ++level) {
    const int shift = 56 - 8 * level;
#pragma unroll
    for (int t = 0; t < 4; ++t) hist[4 * lane + t] = 0;
    wave_sync();
    int32_t carry = -1;
    uint32_t c = 0;
    for (int32_t base = 0; base < n; base += 64) {
      bool special, start;
      flags(base, special, start);
      int32_t head[1] = {base + lane};
      if constexpr (WORD) word_heads<1>(base, {start}, carry, head);
      else start = !special;
      c += (uint32_t)__popcll(__ballot(!special));
      if (!special) {
        const uint64_t key = budget_key(k, row, head[0]);
        if (level == 0 || (key >> (shift + 8)) == prefix)
          atomicAdd(&hist[(key >> shift) & 255u], 1ull | (start ? 1ull << 32 : 0ull));
      }
    }
    wave_sync();
    if (level == 0) left = row_budget(c, p, max_predictions);
    // the first bin whose cumulative weight passes `left`
    uint32_t wt[4], hd[4], sum = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned long long v = hist[4 * lane + t];
      wt[t] = (uint32_t)v;
      hd[t] = (uint32_t)(v >> 32);
      sum += wt[t];
    }
    uint32_t run = wave_incl_add(sum) - sum;
    int found = -1;
    uint32_t before = 0, heads = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (found < 0 && run + wt[t] > left) {
        found = t;
        before = run;
        heads = hd[t];
      }
      run += wt[t];
    }
    const uint64_t m = __ballot(found >= 0);
    if (!m) return kTakeAll;
    const int l = __ffsll((long long)m) - 1;
    const uint64_t bin = 4u * (uint32_t)l + (uint32_t)lane_get(found, l);
    before = lane_get(before, l);
    heads = lane_get(heads, l);
    prefix = prefix << 8 | bin;
    if (heads == 1 || before == left) return prefix << shift;
    left -= before;
  }
  return prefix;  // not reached: a bin of the last level holds one head
}

// Rows of a row table: batch row r as the fill kernels open it.
template <bool CODE, bool WORD>
__global__ __launch_bounds__(256) void mask_budget_kernel(CollateRowsParams P, int32_t bound) {
  __shared__ unsigned long long s_hist[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const uint64_t k = mask_key(P.seed, P.counter);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    OpenRow R;
    uint64_t thr = 0;
    if (!open_row<CODE>(P, r, bound, R)) {
      const int32_t n = R.L.n;
      thr = budget_threshold<WORD>(n, r, k, P.mlm_probability, P.max_predictions, s_hist[w],
                                   [&](int32_t base, bool& special, bool& start) {
                                     const int32_t j = base + lane;
                                     if constexpr (WORD) {
                                       const WordColumn c = word_column(P, R, j, j < n, false);
                                       special = c.special;
                                       start = c.start;
                                     } else {
                                       special = j >= n || R.L.special(j);
                                     }
                                   });
    }
    if (lane == 0) P.thr[r] = thr;
  }
}

// The planes of lddl_mask_tokens: special is the caller's mask, a word starts as in mask_tokens_word_kernel
// (collate.hip).
template <bool WORD>
__global__ __launch_bounds__(256) void mask_budget_tokens_kernel(MaskParams M) {
  __shared__ unsigned long long s_hist[4][256];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int32_t S = M.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const uint64_t k = mask_key(M.seed, M.counter);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < M.n_rows; r += nw) {
    const int64_t* in = M.inputs + r * (int64_t)S;
    const int64_t* sp = M.special + r * (int64_t)S;
    uint32_t left_special = 1;  // of the column in front of the step: none in front of column 0
    const uint64_t thr = budget_threshold<WORD>(
        S, r, k, M.mlm_probability, M.max_predictions, s_hist[w], [&](int32_t base, bool& special, bool& start) {
          const int32_t j = base + lane;
          const uint32_t s = j < S ? (sp[j] != 0 ? 1u : 0u) : 1u;
          special = s != 0;
          if constexpr (WORD) {
            if (base == 0) left_special = 1;  // a new level starts the row again
            const uint32_t shifted = wave_shr1(s);
            const uint32_t before = lane ? shifted : left_special;
            left_special = lane_get(s, 63);
            const int64_t id = j < S ? in[j] : 0;
            start = !s && (before || !word_cont(M.cont, M.n_random, id));
          }
        });
    if (lane == 0) M.thr[r] = thr;
  }
}

}  // namespace

hipError_t launch_mask_budget_rows(const CollateRowsParams& P, bool code, int32_t bound, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  const dim3 grid(grid_rows(P.n_rows, n_cu)), block(256);
  if (P.cont) {
    if (code) hipLaunchKernelGGL((mask_budget_kernel<true, true>), grid, block, 0, s, P, bound);
    else hipLaunchKernelGGL((mask_budget_kernel<false, true>), grid, block, 0, s, P, bound);
  } else {
    if (code) hipLaunchKernelGGL((mask_budget_kernel<true, false>), grid, block, 0, s, P, bound);
    else hipLaunchKernelGGL((mask_budget_kernel<false, false>), grid, block, 0, s, P, bound);
  }
  return hipGetLastError();
}

hipError_t launch_mask_budget_tokens(const MaskParams& M, int n_cu, hipStream_t s) {
  if (M.n_rows * (int64_t)M.seq_len <= 0) return hipSuccess;
  const dim3 grid(grid_rows(M.n_rows, n_cu)), block(256);
  if (M.cont) hipLaunchKernelGGL(mask_budget_tokens_kernel<true>, grid, block, 0, s, M);
  else hipLaunchKernelGGL(mask_budget_tokens_kernel<false>, grid, block, 0, s, M);
  return hipGetLastError();
}

}  // namespace lddl
