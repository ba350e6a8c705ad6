// Device helpers shared by the collate kernels (collate.hip: rows from parquet
// strings; collate_rows.hip / collate_unpadded.hip: rows from a pack result's
// spans, padded and padding-free): the error word
// and the counter-based draws of `_mask_tokens`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lddl {

// first error wins: code in the low 4 bits, the batch row above them
__device__ __forceinline__ void set_err(uint32_t* err, uint32_t code, int64_t row) {
  atomicCAS(err, 0u, code | ((uint32_t)row << 4));
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ double unit53(uint64_t h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }

// _mask_tokens for one column: returns the (possibly replaced) input id and
// sets label
__device__ __forceinline__ int64_t mask_one(int64_t id, bool special, int64_t row, int32_t col, uint64_t seed,
                                            uint64_t counter, double p, int32_t mask_id, int32_t n_random,
                                            int64_t ignore, int64_t& label) {
  const uint64_t k = splitmix64(seed ^ splitmix64(counter));
  const uint64_t idx = ((uint64_t)row << 20 | (uint64_t)col) * 3ull;
  label = ignore;
  if (special || !(unit53(splitmix64(k + idx)) < p)) return id;
  label = id;
  const uint64_t h = splitmix64(k + idx + 1);
  if (unit53(h) < 0.8) return mask_id;
  const uint64_t g = splitmix64(k + idx + 2);
  if (unit53(g) < 0.5) return (int64_t)(((g & 0xFFFFFFFFull) * (uint64_t)n_random) >> 32);
  return id;
}

}  // namespace lddl
