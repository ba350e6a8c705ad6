// Compact MLM targets (lddl_mlm_targets): the ordered compaction of a labels
// tensor into the masked positions and their labels, which a trainer gathers
// the hidden states at before the LM head.  The static shards carry these
// lists per row (masked_lm_positions / masked_lm_labels, which
// lddl/torch/bert.py:113-116 scatters into the dense labels); with dynamic
// masking they never exist, so this has no counterpart in the reference and
// is defined by the labels of the same batch:
//   F = the ascending flat indices t inside a row with labels[t] != ignore_index,
//   M = len(F);  positions[k] = F[k], target_labels[k] = labels[F[k]] for k < M,
//   (0, ignore_index) for M <= k < capacity;  offsets[r] = the selected tokens
//   of the rows before r, offsets[n_rows] = M.
// Row r is [r * seq_len, (r + 1) * seq_len) of a padded batch or
// [cu_seqlens[r], cu_seqlens[r + 1]) of a padding-free one.
//
// Three launches, each over data the one before it wrote (a batch is a few
// hundred thousand tokens at most, so the call is launch-bound: the host adds
// one memset of its scratch words in front and one 16-byte copy behind):
//   count  one wave per row, four rows per block, grid_rows: a ballot and a
//          popcount per 64 columns; the row's count goes to offsets[r + 1] and
//          into the sum of its chunk of kChunk rows.  That sum is an integer
//          atomicAdd: its value does not depend on the arrival order.
//   scan   the second level of collate_row.h over one quantity, one block per
//          chunk as collate_cu_scan_kernel: offsets in place, and M.  Sums are
//          64-bit until M is known to be below 2^31; otherwise nothing is
//          narrowed and the fill pass writes nothing.
//   fill   the count pass again, and a selected lane stores at offsets[r] + the
//          selected columns before it in the row (the step's ballot ranked by
//          mbcnt, plus the steps before).  Then the grid pads [M, capacity).
// Every store's place follows from the labels alone: the order is fixed.
//
// No input faults: cu_seqlens is not trusted.  A row with cu[r] < 0,
// cu[r + 1] < cu[r] or cu[r + 1] > total sets CERR_CU_SEQLENS, counts 0 and is
// never read through, and the fill pass writes nothing once the error word is
// set (rows can overlap only across such a row, so without one M <= total).
// No store goes to an entry >= capacity, whatever M is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {
namespace {

// the tokens [lo, hi) of row r; false for a row of cu_seqlens that does not lie in [0, total)
__device__ __forceinline__ bool targets_row(const MlmTargetsParams& P, int64_t r, int64_t& lo, int64_t& hi) {
  if (!P.cu_seqlens) {
    lo = r * P.seq_len;
    hi = lo + P.seq_len;
    return true;
  }
  lo = P.cu_seqlens[r];
  hi = P.cu_seqlens[r + 1];
  return lo >= 0 && hi >= lo && hi <= P.total;
}

__global__ __launch_bounds__(256) void mlm_targets_count_kernel(MlmTargetsParams P) {
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    int64_t lo, hi;
    uint32_t n = 0;
    if (targets_row(P, r, lo, hi)) {
      for (int64_t base = lo; base < hi; base += 64) {
        const int64_t t = base + lane;
        const bool sel = t < hi && P.labels[t] != P.ignore_index;
        n += (uint32_t)__popcll(__ballot(sel));
      }
    } else if (lane == 0) {
      set_err(P.err, CERR_CU_SEQLENS, r);
    }
    if (lane == 0) {
      P.offsets[r + 1] = (int32_t)n;  // a row holds fewer than 2^31 tokens: total does
      if (n) atomicAdd(&P.chunk_sum[r / kChunk], (unsigned long long)n);
    }
  }
}

__global__ __launch_bounds__(256) void mlm_targets_scan_kernel(MlmTargetsParams P) {
  __shared__ ChunkScanLds<1> S;
  chunk_scan_bases(S, P.n_chunks, [&](int64_t c, unsigned long long (&q)[1]) { q[0] = P.chunk_sum[c]; });
  const int64_t count = (int64_t)S.total[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *P.count_out = count;
    if (count < (1ll << 31)) P.offsets[0] = 0;
  }
  if (count >= (1ll << 31)) return;  // overlapping rows of a refused cu_seqlens; nothing narrowed
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  int64_t carry[1] = {(int64_t)S.base[0]}, end[1];
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    uint32_t v[1] = {0};
    if (r < P.n_rows) v[0] = (uint32_t)P.offsets[r + 1];  // the count pass's
    chunk_scan_step(S, it, v, carry, end);
    if (r < P.n_rows) P.offsets[r + 1] = (int32_t)end[0];
  }
}

__global__ __launch_bounds__(256) void mlm_targets_fill_kernel(MlmTargetsParams P) {
  const int64_t count = *P.count_out;
  if (*P.err || count >= (1ll << 31)) return;  // the same for every thread
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    int64_t lo, hi;
    if (!targets_row(P, r, lo, hi)) continue;
    int64_t k0 = P.offsets[r];
    for (int64_t base = lo; base < hi; base += 64) {
      const int64_t t = base + lane;
      const int64_t lab = t < hi ? P.labels[t] : P.ignore_index;
      const bool sel = lab != P.ignore_index;
      const uint64_t m = __ballot(sel);
      const int64_t k = k0 + bits_below(m);
      if (sel && (uint64_t)k < (uint64_t)P.capacity) {
        P.positions[k] = t;
        P.target_labels[k] = lab;
      }
      k0 += __popcll(m);
    }
  }
  const int64_t nt = (int64_t)gridDim.x * 256;
  for (int64_t k = count + (int64_t)blockIdx.x * 256 + threadIdx.x; k < P.capacity; k += nt) {
    P.positions[k] = 0;
    P.target_labels[k] = P.ignore_index;
  }
}

}  // namespace

hipError_t launch_mlm_targets(const MlmTargetsParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  const dim3 rows(grid_rows(P.n_rows, n_cu)), block(256);
  hipLaunchKernelGGL(mlm_targets_count_kernel, rows, block, 0, s, P);
  hipLaunchKernelGGL(mlm_targets_scan_kernel, dim3((unsigned)P.n_chunks), block, 0, s, P);
  hipLaunchKernelGGL(mlm_targets_fill_kernel, rows, block, 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
