// What the collates that change a row's length share on the device (collate_infill.hip, collate_corrupt.hip,
// collate_segment.hip, collate_denoise.hip): the id of a column of an open row, the store of a row's tokens into
// int64 planes by one wave, text infilling's walk over a token source, and span corruption's placement of a step's
// columns into both of its streams.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_row.h"
#include "wave.h"

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

// ------------------------------------------------------- text infilling's walk --
// The walk of open batch row r by its wave, as the head of collate_infill.hip tells: returns e_r (wave-uniform) and,
// with STAGE, leaves the encoder's tokens in tok[0, e_r).  e_r <= n: the caller's bound on n is the bound on what is
// written.  at(k): the token source (word_column's); opened(j): what the run that opens at column j collapses to.
template <bool STAGE, class At, class Opened>
__device__ __forceinline__ int32_t infill_walk(const CollateRowsParams& P, const OpenRow& R, int64_t r, uint16_t* tok,
                                               At at, Opened opened) {
  const int lane = threadIdx.x & 63;
  const int32_t n = R.L.n;
  SpanCarry carry;
  int32_t count = 0;
  uint64_t last = 0;  // the last column of the step before is selected
  for (int32_t base = 0; base < n; base += 64) {
    const int32_t j = base + lane;
    const WordColumn c = word_column(P, R, j, j < n, false, at);
    const bool st[1] = {c.start}, sp[1] = {c.special};
    bool sel[1];  // false on a special column and behind the row
    span_select<1>(P.span, P.seed, P.counter, r, base, st, sp, carry, sel);
    const uint64_t ms = __ballot(sel[0]);
    const bool before = lane_in(ms << 1 | last);  // the column before this one is selected
    const bool emit = j < n && !(sel[0] && before);
    const uint64_t me = __ballot(emit);
    if (STAGE && emit) tok[count + bits_below(me)] = (uint16_t)(sel[0] ? opened(j) : (int32_t)c.id);
    count += (int32_t)__popcll(me);
    last = ms >> 63;
  }
  return count;
}

// ------------------------------------------------ span corruption's placement --
// What both selections of span corruption (collate_corrupt.hip: runs of whole words under the Poisson law;
// collate_segment.hip: T5's exact-count segmentation) drive: given which columns of a 64-column step are selected,
// the run ordinals, the sentinel cap and the places of both streams, as the head of collate_corrupt.hip tells.
struct CorruptLen {
  int32_t e, t;  // wave-uniform
};

// what a row carries from step to step, wave-uniform
struct CorruptWalk {
  int32_t e = 0, t = 0, runs = 0;  // runs: opened in the steps before, corrupted or not
  uint64_t last = 0;               // the last column of the step before is selected
};

// One step of the walk.  ms: the step's selected columns, sel: this lane's bit of it; valid: the lane's column is a
// column of the row, id: its id.  With STAGE the tokens go to enc[w.e ..) and tgt[w.t ..).
template <bool STAGE>
__device__ __forceinline__ void corrupt_step(const CollateCorruptParams& P, uint64_t ms, bool sel, bool valid,
                                             uint16_t id, CorruptWalk& w, uint16_t* enc, uint16_t* tgt) {
  const uint64_t mo = ms & ~(ms << 1 | w.last);
  const bool open = lane_in(mo);
  const int32_t ord = w.runs + bits_below(mo) + (open ? 1 : 0) - 1;
  const bool corrupt = sel && ord < P.num_sentinels;
  const uint64_t mc = __ballot(corrupt), mco = mc & mo;
  const bool emit = valid && (!corrupt || open);
  const uint64_t me = __ballot(emit);
  if (STAGE) {
    const uint16_t sentinel = (uint16_t)(P.sentinel_base + ord);
    if (emit) enc[w.e + bits_below(me)] = corrupt ? sentinel : id;
    if (corrupt) {
      const int32_t place = w.t + bits_below(mc) + bits_below(mco) + (open ? 1 : 0);
      if (open) tgt[place - 1] = sentinel;
      tgt[place] = id;
    }
  }
  w.e += (int32_t)__popcll(me);
  w.t += (int32_t)__popcll(mc) + (int32_t)__popcll(mco);
  w.runs += (int32_t)__popcll(mo);
  w.last = ms >> 63;
}

// the [SEP] that ends the target, and both lengths
template <bool STAGE>
__device__ __forceinline__ CorruptLen corrupt_finish(int32_t sep, const CorruptWalk& w, uint16_t* tgt) {
  if (STAGE && (threadIdx.x & 63) == 0) tgt[w.t] = (uint16_t)sep;  // t <= n - 1 here
  return {w.e, w.t + 1};
}

// the decoder's planes of target token j < t out of the staged target: decoder_input_ids, labels
__device__ __forceinline__ void decoder_token(const uint16_t* tgt, int32_t cls, int32_t j, int64_t& in, int64_t& lab) {
  in = j ? (int64_t)tgt[j - 1] : (int64_t)cls;
  lab = tgt[j];
}

// whether [c0, c1) can be a row of at most n tokens inside a stream of `total`
__device__ __forceinline__ bool offsets_ok(int64_t c0, int64_t c1, int32_t n, int64_t total) {
  return c0 >= 0 && c1 >= c0 && c1 - c0 <= n && c1 <= total;
}

}  // namespace lddl
