// What the collates that change a row's length share on the device (collate_infill.hip, collate_corrupt.hip): the
// id of a column of an open row, and the store of a row's tokens into int64 planes by one wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_row.h"

namespace lddl {

// the id the open row shows at column j < n
__device__ __forceinline__ int64_t row_id(const CollateRowsParams& P, const OpenRow& R, int32_t j) {
  return R.L.base_id(j, P.cls, P.sep, [&](int32_t k) { return (int32_t)(k <= R.L.a ? R.s0[k] : R.s1[k]); });
}

// Tokens [0, count) of one row into N int64 planes at token offset c0 of each, by one wave.  f(j, v): v[0 .. N) =
// the planes' values of token j.  wide (every plane's base is 16-B aligned): the wave works on the 16-B aligned
// token pairs that cover [c0, c0 + count); a lane computes both tokens of a pair and stores 16 B per plane, the
// first pair of an odd c0 and the last of an odd end hold one token of the row and store 8 B.  Else lane = token.
template <int N, class F>
__device__ __forceinline__ void store_tokens(int64_t* const (&out)[N], int64_t c0, int32_t count, bool wide, F f) {
  const int lane = threadIdx.x & 63;
  if (!wide) {
    for (int32_t j = lane; j < count; j += 64) {
      int64_t v[N];
      f(j, v);
#pragma unroll
      for (int t = 0; t < N; ++t) out[t][c0 + j] = v[t];
    }
    return;
  }
  const int32_t head = (int32_t)(c0 & 1), nq = (head + count + 1) >> 1;
  for (int32_t q = lane; q < nq; q += 64) {
    const int32_t j0 = 2 * q - head, j1 = j0 + 1;  // j0 <= count - 1
    const bool v0 = j0 >= 0, v1 = j1 < count;
    int64_t a[N] = {}, b[N] = {};
    if (v0) f(j0, a);
    if (v1) f(j1, b);
#pragma unroll
    for (int t = 0; t < N; ++t) {
      if (v0 && v1) *reinterpret_cast<longlong2*>(out[t] + c0 + j0) = make_longlong2(a[t], b[t]);
      else if (v0) out[t][c0 + j0] = a[t];
      else if (v1) out[t][c0 + j1] = b[t];
    }
  }
}

template <int N>
__device__ __forceinline__ bool planes_aligned(int64_t* const (&out)[N]) {
  uintptr_t x = 0;
#pragma unroll
  for (int t = 0; t < N; ++t) x |= (uintptr_t)out[t];
  return (x & 15) == 0;
}

}  // namespace lddl
