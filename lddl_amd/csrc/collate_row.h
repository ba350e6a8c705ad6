// What the collate kernels share about a `[CLS] A [SEP] B [SEP]` row (BERT, and
// CodeBERT with or without the first [SEP]), written once: the row layout (collate.hip, collate_rows.hip, collate_unpadded.hip,
// rows_from_strings.hip), opening a batch row of a row table and labelling its
// columns by mode (collate_rows.hip, collate_unpadded.hip, collate_fixed.hip),
// a row's tokens into a padding-free stream (collate_unpadded.hip,
// collate_fixed.hip), the second level of the chunked offsets scans
// (collate_unpadded.hip, rows_from_strings.hip) and the launch helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "collate.h"
#include "collate_dev.h"
#include "wave.h"

namespace lddl {

// ------------------------------------------------------------ the row layout --
// A row of a = len(A) and b = len(B) tokens holds n = a + b + 2 + s columns,
// s = 1 when a [SEP] follows segment 0:
//   0 [CLS] | [1, a] A | a + 1 [SEP] | [a + 2, n - 2] B | n - 1 [SEP] | [n, ..) padding
// (lddl/torch/bert.py:69-153).  token_type_ids is 1 on B and its [SEP]; the
// special_tokens_mask is 1 on the three special tokens and, in a padded batch,
// on the padding.  Every BERT row has s = 1.  A CodeBERT row (doc = segment 0,
// code = segment 1; pretrain_codebert.py:425-433) of a document without
// docstring segments has s = 0 and a = 0:
//   0 [CLS] | [1, n - 2] code | n - 1 [SEP]
// one sequence, token_type_ids 0 throughout.
struct RowLayout {
  int32_t a, n, s = 1;
  __device__ __forceinline__ bool is_cls(int32_t j) const { return j == 0; }
  __device__ __forceinline__ bool is_sep(int32_t j) const { return (s && j == a + 1) || j == n - 1; }
  __device__ __forceinline__ bool special(int32_t j) const { return is_cls(j) || is_sep(j); }
  __device__ __forceinline__ bool seg0(int32_t j) const { return j >= 1 && j <= a; }
  __device__ __forceinline__ bool seg1(int32_t j) const { return j >= a + 1 + s && j < n - 1; }
  __device__ __forceinline__ bool pad(int32_t j) const { return j >= n; }
  __device__ __forceinline__ int32_t token_type(int32_t j) const { return (s && j >= a + 2 && j < n) ? 1 : 0; }
  // the id the row shows at column j < n, before any masking: at(j) is asked
  // for the columns of the two segments only
  template <class At>
  __device__ __forceinline__ int32_t base_id(int32_t j, int32_t cls, int32_t sep, At at) const {
    if (is_cls(j)) return cls;
    if (is_sep(j)) return sep;
    return at(j);
  }
};

// ------------------------------------------------- a batch row of a row table --
// Every reader of a row table takes the kind of its rows as a template
// constant: CODE false, BERT rows (s = 1; a row whose flags lack bit 1 is
// refused); CODE true, CodeBERT rows (s = flags bit 1).

// the pack row of batch row r (rows NULL: row0 + r), or -1 when out of range
__device__ __forceinline__ int64_t pack_row(const CollateRowsParams& P, int64_t r) {
  const int64_t g = P.rows ? P.rows[r] : P.row0 + r;
  return (g < 0 || g >= P.n_total) ? -1 : g;
}

// n of pack row g
template <bool CODE>
__device__ __forceinline__ uint32_t row_tokens(const CollateRowsParams& P, int64_t g) {
  const uint32_t s = CODE ? ((uint32_t)P.flags[g] >> 1) & 1u : 1u;
  return (uint32_t)P.len0[g] + (uint32_t)P.len1[g] + 2u + s;
}

struct OpenRow {
  int64_t g;           // the pack row
  uint32_t flags;
  RowLayout L;
  const uint16_t* s0;  // ids + src0 - 1: column j of segment 0 is s0[j]
  const uint16_t* s1;  // ids + src1 - (a + 1 + s)
};

// Opens batch row r whose n may be `bound` at most: 0 and the row, or the error
// code to set.  Nothing is loaded through a row index before it is
// range-checked; the order of the checks decides which code a row with several
// faults reports.
template <bool CODE>
__device__ __forceinline__ uint32_t open_row(const CollateRowsParams& P, int64_t r, int32_t bound, OpenRow& o) {
  o.g = pack_row(P, r);
  if (o.g < 0) return CERR_ROW_INDEX;
  o.flags = P.flags[o.g];
  o.L.s = CODE ? (int32_t)((o.flags >> 1) & 1u) : 1;
  if (!CODE && !(o.flags & 2u)) return CERR_NO_SEP;  // a CodeBERT row without docstring: no [SEP] after segment 0
  o.L.a = P.len0[o.g];
  if (CODE && !o.L.s && o.L.a > 0) return CERR_CODE_ROW;  // doc tokens and no [SEP] to end them: not the packer's
  o.L.n = o.L.a + (int32_t)P.len1[o.g] + 2 + o.L.s;
  if (o.L.n > bound) return CERR_LONG;
  o.s0 = P.ids + P.src0[o.g] - 1;
  o.s1 = P.ids + P.src1[o.g] - (o.L.a + 1 + o.L.s);
  return 0;
}

constexpr uint32_t kNoMask = 0xFFFFFFFFu;

// COLLATE_STATIC: label | token << 16 of pack row g's masked positions into the
// first `bound` words of the wave's LDS row, kNoMask elsewhere.  False when a
// position is >= bound (nothing is stored for it).
__device__ __forceinline__ bool stage_static_masks(const CollateRowsParams& P, int64_t g, int32_t bound,
                                                   uint32_t* mlm) {
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_wave_barrier();  // the previous row's reads are done
  for (int32_t j = lane; j < bound; j += 64) mlm[j] = kNoMask;
  __builtin_amdgcn_wave_barrier();
  bool bad = false;
  const int64_t k1 = P.mlm_off[g + 1];
  for (int64_t k = P.mlm_off[g] + lane; k < k1; k += 64) {
    const int32_t pos = P.mlm_pos[k];
    if (pos >= bound) bad = true;
    else mlm[pos] = (uint32_t)P.mlm_label[k] | ((uint32_t)P.mlm_token[k] << 16);
  }
  const bool ok = !__ballot(bad);
  __builtin_amdgcn_wave_barrier();
  return ok;
}

struct RowColumn {
  int64_t id, tt, lab;
};

// Column j of batch row r, labelled by MODE: 0 the special_tokens_mask; 1 the
// staged static masks (input_ids[pos] = mlm_token, labels[pos] = mlm_label,
// ignore_index elsewhere); 2 mask_one with row = r.  pad: j is a pad column of
// a padded batch (id 0, special); without padding j < n and pad is false.
template <int MODE>
__device__ __forceinline__ RowColumn row_column(const CollateRowsParams& P, const OpenRow& R, const uint32_t* mlm,
                                                int64_t r, int32_t j, bool pad) {
  RowColumn o;
  const bool special = pad || R.L.special(j);
  int64_t id = 0;
  if (!pad) id = R.L.base_id(j, P.cls, P.sep, [&](int32_t c) { return (int32_t)(c <= R.L.a ? R.s0[c] : R.s1[c]); });
  if (MODE == COLLATE_SPECIAL_MASK) {
    o.lab = special ? 1 : 0;
  } else if (MODE == COLLATE_STATIC) {
    const uint32_t m = mlm[j];
    o.lab = m == kNoMask ? P.ignore_index : (int64_t)(m & 0xFFFFu);
    if (m != kNoMask) id = (int64_t)(m >> 16);
  } else {
    id = mask_one(id, special, r, j, P.seed, P.counter, P.mlm_probability, P.mask_id, P.n_random, P.ignore_index,
                  o.lab);
  }
  o.id = id;
  o.tt = R.L.token_type(j);
  return o;
}

// Whole-word and span masking (mode 2, P.cont set): a column in two halves,
// with step_picks (collate_dev.h) over the start flags of the step between them.
struct WordColumn {
  int64_t id;    // the unmasked id (0 where !valid or pad)
  bool special;  // never selected: a special token, a pad column, or not a column of the row
  bool start;    // a word starts here
};

// valid: j is a column of the batch row (the wide paths compute a neighbour
// that is not); pad as in row_column
__device__ __forceinline__ WordColumn word_column(const CollateRowsParams& P, const OpenRow& R, int32_t j, bool valid,
                                                  bool pad) {
  WordColumn c;
  c.special = !valid || pad || R.L.special(j);
  c.id = 0;
  if (valid && !pad)
    c.id = R.L.base_id(j, P.cls, P.sep, [&](int32_t k) { return (int32_t)(k <= R.L.a ? R.s0[k] : R.s1[k]); });
  // j - 1 is special exactly where j begins a segment: no column is in front of [CLS]
  c.start = !c.special && (R.L.special(j - 1) || !word_cont(P.cont, P.n_random, c.id));
  return c;
}

// the picks of a step of batch row r (step_picks, collate_dev.h): lane l holds columns base + W * l + k
template <int SEL, int W>
__device__ __forceinline__ void row_picks(const CollateRowsParams& P, int64_t r, int32_t base, const WordColumn (&c)[W],
                                          StepCarry& carry, int32_t (&pick)[W]) {
  bool st[W], sp[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    st[k] = c[k].start;
    sp[k] = c[k].special;
  }
  step_picks<SEL, W>(P.span, P.seed, P.counter, r, base, st, sp, carry, pick);
}

// row_column<COLLATE_DYNAMIC> of a column with its pick: the column where its word starts (SEL_WORD), or whether a
// span covers it (SEL_SPAN)
template <int SEL>
__device__ __forceinline__ RowColumn row_column_picked(const CollateRowsParams& P, const OpenRow& R, int64_t r, int32_t j,
                                                       const WordColumn& c, int32_t pick) {
  RowColumn o;
  o.id = mask_one_picked<SEL>(c.id, c.special, r, j, pick, P.seed, P.counter, P.mlm_probability, P.mask_id, P.n_random,
                              P.ignore_index, o.lab);
  o.tt = R.L.token_type(j);
  return o;
}

// ------------------------------------------------- a row of a token stream --
// The columns [0, n) of open batch row r at tokens [c0, c0 + n) of the
// padding-free outputs (R.input_ids, R.token_type_ids, position_ids, R.labels;
// collate_unpadded.hip, collate_fixed.hip), by one wave.  mlm: the wave's staged
// static masks (mode 1).  A row starts at any 8-B aligned token offset, so with
// `wide` (every output base 16-B aligned) the wave works on the 16-B aligned
// token pairs that cover the row: a lane computes both tokens of a pair and
// stores 16 B per output; the first pair of an odd start and the last pair of an
// odd end hold one token of this row and store 8 B.  Without it, lane = token.
// SEL (word or span: mode 2 only): what is selected, as in collate_rows_kernel.
// A step of the wide path is the 128 tokens of 64 aligned pairs, the first of
// them -1 (not a token of the row) when the row starts at an odd offset.
template <int MODE, int SEL>
__device__ __forceinline__ void stream_row(const CollateRowsParams& R, const OpenRow& S, const uint32_t* mlm, int64_t r,
                                           int64_t c0, bool wide, int64_t* position_ids) {
  const int lane = threadIdx.x & 63;
  const int32_t n = S.L.n;
  int64_t* o_ids = R.input_ids + c0;
  int64_t* o_tt = R.token_type_ids + c0;
  int64_t* o_pos = position_ids + c0;
  int64_t* o_lab = R.labels + c0;
  if constexpr (SEL != SEL_TOKEN) {
    StepCarry carry;
    if (wide) {
      const int32_t head = (int32_t)(c0 & 1);
      const int32_t nq = (head + n + 1) >> 1;
      for (int32_t qb = 0; qb < nq; qb += 64) {
        const int32_t q = qb + lane;
        const int32_t j0 = 2 * q - head, j1 = j0 + 1;
        const bool v0 = q < nq && j0 >= 0, v1 = q < nq && j1 < n;
        const WordColumn w[2] = {word_column(R, S, j0, v0, false), word_column(R, S, j1, v1, false)};
        int32_t pick[2];
        row_picks<SEL, 2>(R, r, 2 * qb - head, w, carry, pick);
        const RowColumn t0 = row_column_picked<SEL>(R, S, r, j0, w[0], pick[0]);
        const RowColumn t1 = row_column_picked<SEL>(R, S, r, j1, w[1], pick[1]);
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
        const WordColumn w[1] = {word_column(R, S, j, j < n, false)};
        int32_t pick[1];
        row_picks<SEL, 1>(R, r, base, w, carry, pick);
        if (j < n) {
          const RowColumn t = row_column_picked<SEL>(R, S, r, j, w[0], pick[0]);
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
}

// ------------------------------------------------ the chunked offsets scan --
// An exclusive scan of N per-row quantities over any number of rows, in two
// levels.  Level one is each caller's own: chunk c's sums of its kChunk rows
// (a chunk's sum fits 32 bits: kChunk * (2 * 65535 + 3) < 2^29).  Level two is
// one block of 256 threads per chunk: chunk_scan_bases adds the chunk sums in
// front of the block (base) and all of them (total), in 64 bits; then the
// block walks its chunk 256 rows at a time and chunk_scan_step gives every
// thread the sum up to and including its row.  One __syncthreads per step:
// the steps alternate between the two halves of `wave`.
template <int N>
struct ChunkScanLds {
  unsigned long long base[N], total[N];
  uint32_t wave[2][N][4];
};

// sums(c, q): q[0 .. N) = the sums of chunk c.  Ends with a __syncthreads:
// S.base and S.total are final for every thread.
template <int N, class Sums>
__device__ __forceinline__ void chunk_scan_bases(ChunkScanLds<N>& S, int64_t n_chunks, Sums sums) {
  const int tid = threadIdx.x;
  if (tid < N) S.base[tid] = S.total[tid] = 0;
  __syncthreads();
  unsigned long long below[N] = {}, all[N] = {};
  for (int64_t c = tid; c < n_chunks; c += 256) {
    unsigned long long q[N];
    sums(c, q);
#pragma unroll
    for (int t = 0; t < N; ++t) {
      all[t] += q[t];
      if (c < (int64_t)blockIdx.x) below[t] += q[t];
    }
  }
#pragma unroll
  for (int t = 0; t < N; ++t) {
    if (below[t]) atomicAdd(&S.base[t], below[t]);
    if (all[t]) atomicAdd(&S.total[t], all[t]);
  }
  __syncthreads();
}

// step `it` of the block's chunk: v = this thread's row (0 behind the last
// row); end[t] = the sum of quantity t over rows [0, this row]; carry starts
// at S.base and moves on by the step's 256 rows
template <int N>
__device__ __forceinline__ void chunk_scan_step(ChunkScanLds<N>& S, int it, const uint32_t (&v)[N], int64_t (&carry)[N],
                                                int64_t (&end)[N]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t incl[N];
#pragma unroll
  for (int t = 0; t < N; ++t) {
    incl[t] = wave_incl_add(v[t]);
    if (lane == 63) S.wave[it & 1][t][w] = incl[t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < N; ++t) {
    uint32_t before = 0, step = 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = S.wave[it & 1][t][k];
      step += x;
      if (k < w) before += x;
    }
    end[t] = carry[t] + before + incl[t];
    carry[t] += step;
  }
}

// ------------------------------------------------------------------- launches --
// one wave per row, four rows per block, at most eight blocks per CU
inline int grid_rows(int64_t n_rows, int n_cu) {
  int64_t g = (n_rows + 3) / 4;
  const int64_t cap = (int64_t)n_cu * 8;
  if (g > cap) g = cap;
  return (int)(g < 1 ? 1 : g);
}

// f(std::integral_constant<int, MODE>) for the kernels that take the mode as a template constant
template <class F>
inline void dispatch_mode(int32_t mode, F f) {
  if (mode == COLLATE_SPECIAL_MASK) f(std::integral_constant<int, COLLATE_SPECIAL_MASK>{});
  else if (mode == COLLATE_STATIC) f(std::integral_constant<int, COLLATE_STATIC>{});
  else f(std::integral_constant<int, COLLATE_DYNAMIC>{});
}

// the same for CodeBERT rows, which have no static masks: modes 0 and 2
template <class F>
inline void dispatch_code_mode(int32_t mode, F f) {
  if (mode == COLLATE_SPECIAL_MASK) f(std::integral_constant<int, COLLATE_SPECIAL_MASK>{});
  else f(std::integral_constant<int, COLLATE_DYNAMIC>{});
}

}  // namespace lddl
