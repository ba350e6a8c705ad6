// Device helpers shared by the collate kernels (collate.hip: rows from parquet
// strings; rows_from_strings.hip: a row table from parquet strings;
// collate_rows.hip / collate_unpadded.hip: rows from a pack result's
// spans, padded and padding-free): the error word, the counter-based draws of
// `_mask_tokens` with the wave-level scans of whole-word and span selection,
// and what reads a string column: Python's str.split(), the
// whole-token vocab lookup and the np.save header of masked_lm_positions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "wave.h"

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

// the three draws of (row, col) are the hashes of k + idx, + 1 and + 2
__device__ __forceinline__ uint64_t mask_key(uint64_t seed, uint64_t counter) {
  return splitmix64(seed ^ splitmix64(counter));
}
__device__ __forceinline__ uint64_t mask_idx(int64_t row, int32_t col) {
  return ((uint64_t)row << 20 | (uint64_t)col) * 3ull;
}

// a selected column (row, col): its label, and [MASK] / a random id / the id
// kept by its own second and third draws
__device__ __forceinline__ int64_t mask_selected(int64_t id, int64_t row, int32_t col, uint64_t k, int32_t mask_id,
                                                 int32_t n_random, int64_t& label) {
  label = id;
  const uint64_t idx = mask_idx(row, col);
  const uint64_t h = splitmix64(k + idx + 1);
  if (unit53(h) < 0.8) return mask_id;
  const uint64_t g = splitmix64(k + idx + 2);
  if (unit53(g) < 0.5) return (int64_t)(((g & 0xFFFFFFFFull) * (uint64_t)n_random) >> 32);
  return id;
}

// _mask_tokens for one column whose select draw is taken at column sel of its
// row and whose replacement draws are its own: returns the (possibly replaced)
// input id and sets label
__device__ __forceinline__ int64_t mask_one_at(int64_t id, bool special, int64_t row, int32_t col, int32_t sel,
                                               uint64_t seed, uint64_t counter, double p, int32_t mask_id,
                                               int32_t n_random, int64_t ignore, int64_t& label) {
  const uint64_t k = mask_key(seed, counter);
  label = ignore;
  if (special || !(unit53(splitmix64(k + mask_idx(row, sel))) < p)) return id;
  return mask_selected(id, row, col, k, mask_id, n_random, label);
}

// _mask_tokens for one column: every column selects for itself
__device__ __forceinline__ int64_t mask_one(int64_t id, bool special, int64_t row, int32_t col, uint64_t seed,
                                            uint64_t counter, double p, int32_t mask_id, int32_t n_random,
                                            int64_t ignore, int64_t& label) {
  return mask_one_at(id, special, row, col, col, seed, counter, p, mask_id, n_random, ignore, label);
}

// ------------------------------------------------------ whole-word masking --
// cont(id): vocabulary entry id begins with "##" (bit id of the ctx's table;
// an id outside [0, n_vocab) is no continuation)
__device__ __forceinline__ bool word_cont(const uint32_t* bits, int32_t n_vocab, int64_t id) {
  return (uint64_t)id < (uint64_t)n_vocab && ((bits[id >> 5] >> (id & 31)) & 1u);
}

// The head of every column of one step of a row: the last column at or before
// it where a word starts.  A step is W * 64 columns, lane l owns columns
// base + W * l + k (k < W) and says in st[k] whether a word starts there
// (false on a column that is not the row's).  head[k] is the highest start at
// or below the lane's column k, from the ballots of the step; without one,
// carry: the last start of the row's earlier steps (-1 before the first; the
// caller sets it so for every row).  carry is wave-uniform and moves on to the
// step's last start.  Registers and scalars only.  Every lane of the wave
// calls it.
template <int W>
__device__ __forceinline__ void word_heads(int32_t base, const bool (&st)[W], int32_t& carry, int32_t (&head)[W]) {
  const int lane = threadIdx.x & 63;
  const uint64_t upto = (2ull << lane) - 1ull;  // the lanes at or below this one
  uint64_t m[W];
#pragma unroll
  for (int t = 0; t < W; ++t) m[t] = __ballot(st[t]);
  int32_t last = carry;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    head[k] = carry;
#pragma unroll
    for (int t = 0; t < W; ++t) {
      // sub-column t of a lane is at or before sub-column k of this one: the lanes below, and this one when t <= k
      const uint64_t b = m[t] & (t <= k ? upto : upto >> 1);
      if (b) head[k] = max(head[k], base + W * (63 - __clzll((long long)b)) + t);
    }
  }
#pragma unroll
  for (int t = 0; t < W; ++t)
    if (m[t]) last = max(last, base + W * (63 - __clzll((long long)m[t])) + t);
  carry = last;
}

// ------------------------------------------------------------ span masking --
// (lddl_set_span_mask; include/lddl_amd.h defines it.)  What a row carries
// from step to step, wave-uniform: the running word index, and the furthest
// reach of the open heads so far.
struct SpanCarry {
  uint32_t word = 0, reach = 0;
};

// len(h) of the open head at (row, col): 1 + the entries of cdf that its draw
// is not below.  The entries from L - 1 on are 1.0, above every draw, so the
// compares need no L and every index is a constant (scalar loads).
__device__ __forceinline__ uint32_t span_len(const SpanLaw& S, uint64_t ks, int64_t row, int32_t col) {
  const double u = unit53(splitmix64(ks + mask_idx(row, col)));
  uint32_t len = 1;
#pragma unroll
  for (int t = 0; t < 15; ++t) len += u >= S.cdf[t] ? 1u : 0u;
  return len;
}

// Which columns of one step of a row are selected.  The step and st are
// word_heads'; sp[k]: the lane's column k is special (true as well on a column
// that is not the row's).  The word index of a column is a running count over
// the row, + 1 at every word start and + L at every special column: the
// ballots' bits below the lane, the lane's own columns and carry.word.  An
// open head h reaches up to index(h) + len(h); a column is selected iff the
// furthest reach of the open heads at or before it (an inclusive max-scan over
// the lanes, and carry.reach) exceeds its index.  The + L keeps a reach out of
// the segments behind it: their indices start above index(h) + L.  The length
// draw is taken on the lanes that hold an open head only.  Registers, scalars
// and wave operations only.  Every lane of the wave calls it.
template <int W>
__device__ __forceinline__ void span_select(const SpanLaw& S, uint64_t seed, uint64_t counter, int64_t row,
                                            int32_t base, const bool (&st)[W], const bool (&sp)[W], SpanCarry& carry,
                                            bool (&sel)[W]) {
  const int lane = threadIdx.x & 63;
  const uint64_t k = mask_key(seed, counter), ks = splitmix64(k ^ 0x5350414E4D41534Bull);
  const uint32_t L = (uint32_t)S.L;
  uint32_t x = carry.word, step = 0;
#pragma unroll
  for (int t = 0; t < W; ++t) {
    const uint64_t ms = __ballot(st[t]), mp = __ballot(sp[t]);
    x += (uint32_t)bits_below(ms) + L * (uint32_t)bits_below(mp);
    step += (uint32_t)__popcll(ms) + L * (uint32_t)__popcll(mp);
  }
  uint32_t index[W], reach[W], m = 0;  // reach[t]: of the lane's own open heads up to its column t
#pragma unroll
  for (int t = 0; t < W; ++t) {
    x += st[t] ? 1u : sp[t] ? L : 0u;
    index[t] = x;
    const int32_t col = base + W * lane + t;
    if (st[t] && unit53(splitmix64(k + mask_idx(row, col))) < S.q) m = max(m, x + span_len(S, ks, row, col));
    reach[t] = m;
  }
  const uint32_t incl = wave_incl_max(m);
  const uint32_t before = max(carry.reach, wave_shr1(incl));  // of the lanes below, and of the steps before
#pragma unroll
  for (int t = 0; t < W; ++t) sel[t] = !sp[t] && max(before, reach[t]) > index[t];
  carry.word += step;
  carry.reach = max(carry.reach, lane_get(incl, 63));
}

// -------------------------------- a step of whole-word or of span selection --
struct StepCarry {
  int32_t head = -1;  // SEL_WORD: word_heads' carry
  SpanCarry span;     // SEL_SPAN
};

// pick[k] of the lane's column k: the head of its word (SEL_WORD), or whether
// a span covers it (SEL_SPAN); st and sp as span_select has them
template <int SEL, int W>
__device__ __forceinline__ void step_picks(const SpanLaw& S, uint64_t seed, uint64_t counter, int64_t row, int32_t base,
                                           const bool (&st)[W], const bool (&sp)[W], StepCarry& carry,
                                           int32_t (&pick)[W]) {
  static_assert(SEL == SEL_WORD || SEL == SEL_SPAN, "tokens select for themselves");
  if constexpr (SEL == SEL_WORD) {
    word_heads<W>(base, st, carry.head, pick);
  } else {
    bool sel[W];
    span_select<W>(S, seed, counter, row, base, st, sp, carry.span, sel);
#pragma unroll
    for (int t = 0; t < W; ++t) pick[t] = sel[t] ? 1 : 0;
  }
}

// _mask_tokens for one column with its pick of step_picks
template <int SEL>
__device__ __forceinline__ int64_t mask_one_picked(int64_t id, bool special, int64_t row, int32_t col, int32_t pick,
                                                   uint64_t seed, uint64_t counter, double p, int32_t mask_id,
                                                   int32_t n_random, int64_t ignore, int64_t& label) {
  if constexpr (SEL == SEL_WORD) {
    return mask_one_at(id, special, row, col, pick, seed, counter, p, mask_id, n_random, ignore, label);
  } else {
    label = ignore;
    if (!pick) return id;
    return mask_selected(id, row, col, mask_key(seed, counter), mask_id, n_random, label);
  }
}

static constexpr uint32_t kEmpty = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint32_t chash_step(uint32_t h, uint32_t b) {
  h ^= b;
  return h * 0x01000193u;  // FNV-1a 32
}

__host__ __device__ __forceinline__ uint32_t chash_final(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

// Python str.isspace() for the characters str.split() splits on
__device__ __forceinline__ bool py_space(uint32_t c) {
  if (c < 0x80) return (c >= 9 && c <= 13) || (c >= 0x1c && c <= 0x20);
  return c == 0x85 || c == 0xa0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200a) || c == 0x2028 || c == 0x2029 ||
         c == 0x202f || c == 0x205f || c == 0x3000;
}

// decode the UTF-8 character starting at p[i] (a lead byte), i < e
__device__ __forceinline__ uint32_t decode_at(const uint8_t* p, int64_t i, int64_t e, int& n) {
  const uint32_t b = p[i];
  if (b < 0x80) {
    n = 1;
    return b;
  }
  n = b >= 0xF0 ? 4 : b >= 0xE0 ? 3 : 2;
  uint32_t c = b & (0x7Fu >> n);
  for (int k = 1; k < n; ++k) c = (c << 6) | (i + k < e ? (p[i + k] & 0x3Fu) : 0u);
  return c;
}

// does byte i (s <= i < e) belong to a whitespace character?
__device__ __forceinline__ bool ws_byte(const uint8_t* p, int64_t i, int64_t s, int64_t e) {
  const uint32_t b = p[i];
  if (b < 0x80) return py_space(b);
  int64_t j = i;
  while (j > s && j > i - 3 && (p[j] & 0xC0u) == 0x80u) --j;
  int n;
  return py_space(decode_at(p, j, e, n));
}

__device__ __forceinline__ int32_t vocab_lookup(const CollateVocab& V, const uint8_t* p, int64_t i, int64_t e,
                                                int64_t& end) {
  uint32_t h = 0x811c9dc5u;
  int64_t j = i;
  while (j < e) {
    const uint32_t b = p[j];
    if (b < 0x80) {
      if (py_space(b)) break;
      h = chash_step(h, b);
      ++j;
      continue;
    }
    int n;
    const uint32_t c = decode_at(p, j, e, n);
    if (py_space(c)) break;
    for (int k = 0; k < n && j + k < e; ++k) h = chash_step(h, p[j + k]);
    j += n;
  }
  if (j > e) j = e;
  end = j;
  h = chash_final(h);
  const uint32_t len = (uint32_t)(j - i);
  for (uint32_t s = h & V.mask;; s = (s + 1) & V.mask) {
    const uint2 t = V.slots[s];
    if (t.y == kEmpty) return V.unk;
    if (t.x != h) continue;
    const uint32_t vi = V.vinfo[t.y];
    if ((vi & 0xFFu) != len) continue;
    const uint8_t* q = V.vpool + (vi >> 8);
    uint32_t k = 0;
    while (k < len && q[k] == p[i + k]) ++k;
    if (k == len) return (int32_t)t.y;
  }
}

// Walk the tokens of bytes [s, e): calls f(ordinal, start) on the owning lane
// (ordinal in token order); returns the token count (wave-uniform).
template <class F>
__device__ __forceinline__ int32_t scan_tokens(const uint8_t* p, int64_t s, int64_t e, F f) {
  const int lane = threadIdx.x & 63;
  int32_t count = 0;
  for (int64_t base = s; base < e; base += 64) {
    const int64_t i = base + lane;
    bool st = false;
    if (i < e) {
      const uint32_t b = p[i];
      st = (b & 0xC0u) != 0x80u && !ws_byte(p, i, s, e) && (i == s || ws_byte(p, i - 1, s, e));
    }
    const uint64_t m = __ballot(st);
    if (st) f(count + (int32_t)__popcll(m & ((1ull << lane) - 1ull)), i);
    count += (int32_t)__popcll(m);
  }
  return count;
}

// np.save v1.x bytes q[0, qn) of a 1-D '<u2' array (masked_lm_positions,
// lddl/utils.py deserialize_np_array): d = its payload, np = its entries;
// false when the bytes are not that
__device__ __forceinline__ bool npy_u16_payload(const uint8_t* q, int64_t qn, const uint8_t*& d, int64_t& np) {
  bool ok = qn >= 10 && q[0] == 0x93 && q[1] == 'N' && q[2] == 'U' && q[3] == 'M' && q[4] == 'P' && q[5] == 'Y' &&
            q[6] == 1;
  const int64_t hl = ok ? (int64_t)q[8] | ((int64_t)q[9] << 8) : 0;
  ok = ok && 10 + hl <= qn && ((qn - 10 - hl) & 1) == 0;
  if (!ok) return false;
  np = (qn - 10 - hl) >> 1;
  d = q + 10 + hl;
  return true;
}

}  // namespace lddl
