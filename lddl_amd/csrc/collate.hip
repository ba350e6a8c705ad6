// Training-time collate: parquet rows -> BERT model inputs, and the dynamic
// 80/10/10 MLM masking, on the GPU.
//
// Reference: lddl/torch/bert.py:69-153 `_to_encoded_inputs` and :156-196
// `_mask_tokens`.  Per row: A.split() / B.split() (Python str.split: runs of
// Unicode whitespace), convert_tokens_to_ids (vocab lookup, [UNK] for a miss),
// tokens = [CLS] A [SEP] B [SEP] padded with 0 to the batch's longest row
// rounded up to `sequence_length_alignment`; token_type_ids 1 on B and its
// [SEP]; attention_mask 1 on the row; next_sentence_labels = is_random_next.
// Static masking (bert.py:113-116): labels = ignore_index except
// labels[positions] = ids(masked_lm_labels.split()), positions decoded from the
// row's np.save bytes.  Dynamic (bert.py:117-122, 156-196): special_tokens_mask
// = [CLS], the middle [SEP] and everything from the last [SEP] on; a
// non-special column is masked with probability mlm_probability, then [MASK]
// with p 0.8, else a random id in [0, len(tokenizer)) with p 0.5, else kept;
// labels = original id on masked columns, ignore_index elsewhere.  The draws
// come from a counter-based hash of (seed, counter, row, column) instead of
// torch's CPU generator: same distribution, not the same stream.
//
// Work mapping: one wave per row.  Pass 1 (token scan) walks the segment's
// bytes 64 at a time: lane i owns byte i, a token starts where a
// non-whitespace character follows whitespace; the token's ordinal is the
// ballot prefix count, the owning lane reads the token to its end, hashes it
// and probes the L2-resident vocab table.  Ids land in a per-wave LDS row;
// pass 2 writes the five int64 columns coalesced (lane = column).  The bound
// is the int64 output stream (40 B per column) against a few bytes of input.
// What column j of a row holds is RowLayout's (collate_row.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {

uint32_t collate_hash_host(const uint8_t* p, int n) {
  uint32_t h = 0x811c9dc5u;
  for (int i = 0; i < n; ++i) h = chash_step(h, p[i]);
  return chash_final(h);
}

// max_len = max over rows of len(A) + len(B) + 3
__global__ __launch_bounds__(256) void collate_len_kernel(CollateParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < P.n_rows; r += nw) {
    auto none = [](int32_t, int64_t) {};
    const int32_t na = scan_tokens(P.C.a, P.C.a_off[r], P.C.a_off[r + 1], none);
    const int32_t nb = scan_tokens(P.C.b, P.C.b_off[r], P.C.b_off[r + 1], none);
    if (lane == 0) atomicMax(P.max_len, na + nb + 3);
  }
}

// SEL (word or span: launched for mode 2 only, P.cont set): whole-word or span
// masking; pass 2 finds every column's pick with step_picks over the ids of
// the LDS row
template <int SEL>
__global__ __launch_bounds__(256) void collate_fill_kernel(CollateParams P) {
  __shared__ int32_t s_ids[4][COLLATE_MAX_LEN];
  __shared__ int32_t s_lab[4][COLLATE_MAX_LEN];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  int32_t* ids = s_ids[w];
  int32_t* lab = s_lab[w];
  const int32_t L = P.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    const CollateVocab& V = P.V;
    const StringColumns& C = P.C;
    // pass 1: token ids into the LDS row (positions >= L are dropped and flagged)
    int32_t na = scan_tokens(C.a, C.a_off[r], C.a_off[r + 1], [&](int32_t k, int64_t i) {
      int64_t end;
      const int32_t id = vocab_lookup(V, C.a, i, C.a_off[r + 1], end);
      if (1 + k < L) ids[1 + k] = id;
    });
    int32_t nb = scan_tokens(C.b, C.b_off[r], C.b_off[r + 1], [&](int32_t k, int64_t i) {
      int64_t end;
      const int32_t id = vocab_lookup(V, C.b, i, C.b_off[r + 1], end);
      if (na + 2 + k < L) ids[na + 2 + k] = id;
    });
    const RowLayout S{na, na + nb + 3};
    if (S.n > L) {
      if (lane == 0) set_err(P.err, CERR_LONG, r);
      continue;
    }
    if (P.mode == COLLATE_STATIC) {
      for (int32_t j = lane; j < L; j += 64) lab[j] = -1;
      // positions: np.save v1.x bytes of a 1-D '<u2' array
      const uint8_t* d;
      int64_t np64;
      if (!npy_u16_payload(C.pos + C.pos_off[r], C.pos_off[r + 1] - C.pos_off[r], d, np64)) {
        if (lane == 0) set_err(P.err, CERR_NPY, r);
        continue;
      }
      const int32_t np = (int32_t)np64;
      __builtin_amdgcn_wave_barrier();
      // labels[positions[k]] = id(masked_lm_labels.split()[k])
      const int64_t l0 = C.lab_off[r], l1 = C.lab_off[r + 1];
      bool bad = false;
      const int32_t nl = scan_tokens(C.lab, l0, l1, [&](int32_t k, int64_t i) {
        int64_t end;
        const int32_t id = vocab_lookup(V, C.lab, i, l1, end);
        if (k < np) {
          const int32_t pos = (int32_t)d[2 * k] | ((int32_t)d[2 * k + 1] << 8);
          if (pos >= L) bad = true;
          else lab[pos] = id;
        }
      });
      if (nl != np) {
        if (lane == 0) set_err(P.err, CERR_NLAB, r);
        continue;
      }
      if (__ballot(bad)) {
        if (lane == 0) set_err(P.err, CERR_POS_RANGE, r);
        continue;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // pass 2: the int64 columns, lane = column
    int64_t* o_ids = P.input_ids + r * (int64_t)L;
    int64_t* o_tt = P.token_type_ids + r * (int64_t)L;
    int64_t* o_am = P.attention_mask + r * (int64_t)L;
    int64_t* o_lab = P.labels + r * (int64_t)L;
    if constexpr (SEL != SEL_TOKEN) {
      StepCarry carry;
      for (int32_t base = 0; base < L; base += 64) {
        const int32_t j = base + lane;
        const bool pad = j >= L || S.pad(j);
        const bool special = pad || S.special(j);
        int64_t id = 0;
        if (!pad) id = S.base_id(j, V.cls, V.sep, [&](int32_t c) { return ids[c]; });
        const bool start = !special && (S.special(j - 1) || !word_cont(P.cont, V.n_random, id));
        int32_t pick[1];
        step_picks<SEL, 1>(P.span, P.seed, P.counter, r, base, {start}, {special}, carry, pick);
        if (j < L) {
          int64_t l;
          id = mask_one_picked<SEL>(id, special, r, j, pick[0], P.seed, P.counter, P.mlm_probability, V.mask_id,
                                    V.n_random, P.ignore_index, l);
          o_ids[j] = id;
          o_tt[j] = S.token_type(j);
          o_am[j] = pad ? 0 : 1;
          o_lab[j] = l;
        }
      }
      if (lane == 0) P.next_sentence_labels[r] = P.is_random_next[r] ? 1 : 0;
      continue;
    }
    for (int32_t j = lane; j < L; j += 64) {
      const bool pad = S.pad(j);
      const bool special = pad || S.special(j);
      int64_t id = 0;
      if (!pad) id = S.base_id(j, V.cls, V.sep, [&](int32_t c) { return ids[c]; });
      int64_t l;
      if (P.mode == COLLATE_SPECIAL_MASK) l = special ? 1 : 0;
      else if (P.mode == COLLATE_STATIC) l = lab[j] < 0 ? P.ignore_index : (int64_t)lab[j];
      else id = mask_one(id, special, r, j, P.seed, P.counter, P.mlm_probability, V.mask_id, V.n_random,
                         P.ignore_index, l);
      o_ids[j] = id;
      o_tt[j] = S.token_type(j);
      o_am[j] = pad ? 0 : 1;
      o_lab[j] = l;
    }
    if (lane == 0) P.next_sentence_labels[r] = P.is_random_next[r] ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void mask_tokens_kernel(MaskParams M) {
  const int64_t total = M.n_rows * (int64_t)M.seq_len;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / M.seq_len;
    const int32_t j = (int32_t)(e - r * M.seq_len);
    int64_t l;
    M.inputs[e] = mask_one(M.inputs[e], M.special[e] != 0, r, j, M.seed, M.counter, M.mlm_probability, M.mask_id,
                           M.n_random, M.ignore_index, l);
    M.labels[e] = l;
  }
}

// mask_tokens_kernel with whole-word masking: one wave per row, lane = column,
// 64 columns per step, in place.  A word starts at a non-special column that
// is the row's first, follows a special one or holds no "##" entry (an id
// outside the vocabulary is none).  A lane reads its id and its special flag,
// and takes the flag of the column to its left from its neighbour (lane 0:
// from lane 63 of the step before), before it stores.  SEL: whole words, or
// spans of them (special: the caller's mask, and the columns behind the row).
template <int SEL>
__global__ __launch_bounds__(256) void mask_tokens_word_kernel(MaskParams M) {
  const int lane = threadIdx.x & 63;
  const int32_t S = M.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < M.n_rows; r += nw) {
    int64_t* in = M.inputs + r * (int64_t)S;
    const int64_t* sp = M.special + r * (int64_t)S;
    int64_t* lab = M.labels + r * (int64_t)S;
    StepCarry carry;
    uint32_t left_special = 1;  // of the column in front of the step: none in front of column 0
    for (int32_t base = 0; base < S; base += 64) {
      const int32_t j = base + lane;
      const bool in_row = j < S;
      const int64_t id = in_row ? in[j] : 0;
      const uint32_t special = in_row ? (sp[j] != 0 ? 1u : 0u) : 1u;
      const uint32_t shifted = wave_shr1(special);  // by the whole wave, outside the select
      const uint32_t before = lane ? shifted : left_special;
      left_special = lane_get(special, 63);
      const bool start = !special && (before || !word_cont(M.cont, M.n_random, id));
      int32_t pick[1];
      step_picks<SEL, 1>(M.span, M.seed, M.counter, r, base, {start}, {special != 0}, carry, pick);
      if (in_row) {
        int64_t l;
        in[j] = mask_one_picked<SEL>(id, special != 0, r, j, pick[0], M.seed, M.counter, M.mlm_probability, M.mask_id,
                                     M.n_random, M.ignore_index, l);
        lab[j] = l;
      }
    }
  }
}

hipError_t launch_collate_len(const CollateParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(collate_len_kernel, dim3(grid_rows(P.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_collate_fill(const CollateParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  const dim3 grid(grid_rows(P.n_rows, n_cu)), block(256);
  const int sel = P.mode == COLLATE_DYNAMIC ? collate_sel(P.cont, P.span) : SEL_TOKEN;
  if (sel == SEL_SPAN) hipLaunchKernelGGL(collate_fill_kernel<SEL_SPAN>, grid, block, 0, s, P);
  else if (sel == SEL_WORD) hipLaunchKernelGGL(collate_fill_kernel<SEL_WORD>, grid, block, 0, s, P);
  else hipLaunchKernelGGL(collate_fill_kernel<SEL_TOKEN>, grid, block, 0, s, P);
  return hipGetLastError();
}

hipError_t launch_mask_tokens(const MaskParams& M, int n_cu, hipStream_t s) {
  const int64_t total = M.n_rows * (int64_t)M.seq_len;
  if (total <= 0) return hipSuccess;
  if (M.cont) {
    const dim3 grid(grid_rows(M.n_rows, n_cu)), block(256);
    if (M.span.L > 0) hipLaunchKernelGGL(mask_tokens_word_kernel<SEL_SPAN>, grid, block, 0, s, M);
    else hipLaunchKernelGGL(mask_tokens_word_kernel<SEL_WORD>, grid, block, 0, s, M);
    return hipGetLastError();
  }
  int64_t g = (total + 255) / 256;
  if (g > (int64_t)n_cu * 16) g = (int64_t)n_cu * 16;
  hipLaunchKernelGGL(mask_tokens_kernel, dim3((int)g), dim3(256), 0, s, M);
  return hipGetLastError();
}

}  // namespace lddl
