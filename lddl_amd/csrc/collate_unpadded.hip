// Padding-free collate from a pack result: the batch of collate_rows.hip with
// the pad columns removed.  The rows are concatenated into one token stream,
// row r at [cu_seqlens[r], cu_seqlens[r + 1]), which is what variable-length
// attention kernels take; there is no attention_mask and a position_ids
// stream instead.
//
// No counterpart in the reference (lddl/torch/bert.py:69-153 pads).  Defined
// by the padded batch: with batch row r = pack row g = rows[r] (rows NULL:
// row0 + r), a = len0[g], b = len1[g], n_r = a + b + 3 and t = cu_seqlens[r] + j,
// 0 <= j < n_r:
//   input_ids[t], token_type_ids[t], labels[t] = column j of row r of
//     lddl_collate_rows at the same mode, seed and counter (the dynamic draw is
//     keyed by (seed, counter, r, j), not by seq_len)
//   position_ids[t] = j;  next_sentence_labels[r] = flags[g] & 1
//
// Offsets pass: cu_seqlens is an exclusive scan of n_r, in two levels: every
// block sums its chunk of kChunk rows (collate_cu_sum_kernel), then adds the
// chunk sums in front of it, scans its chunk again and writes
// (collate_cu_scan_kernel).  Sums are 64-bit until the total is known to be
// below 2^31; otherwise nothing is written.  A batch is thousands of rows, so
// this is two launches of a few blocks: launch-bound.
//
// Fill pass: one wave per batch row, four rows per block and the per-wave LDS
// row of mode 1, as collate_rows_kernel.  A row starts at any 8-B aligned token
// offset, so the wave works on the 16-B aligned token pairs that cover
// [cu_seqlens[r], cu_seqlens[r] + n_r): a lane computes both tokens of a pair and
// stores 16 B per output; the first pair of a row with an odd start and the
// last pair of one with an odd end hold one token of this row and store 8 B.
// Outputs whose base is not 16-B aligned take the lane = token path.
//
// No input faults: cu_seqlens is not trusted.  A row whose offsets are not
// [c, c + n_r) within [0, total) sets CERR_CU_SEQLENS; a row index out of
// range, a CodeBERT row, a row longer than COLLATE_MAX_LEN and (mode 1) a static
// position >= n_r set the codes of collate_rows.hip; such a row is left
// unwritten.  No row stores outside its own tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "wave.h"

namespace lddl {
namespace {

constexpr uint32_t kNoMask = 0xFFFFFFFFu;
constexpr int kChunk = 2048;  // rows per block of the offsets pass: 8 per thread

// n_r of batch row r, or 0 (error word set) when its row index is out of range
__device__ __forceinline__ uint32_t row_len(const CollateRowsParams& R, int64_t r) {
  const int64_t g = R.rows ? R.rows[r] : R.row0 + r;
  if (g < 0 || g >= R.n_total) {
    set_err(R.err, CERR_ROW_INDEX, r);
    return 0;
  }
  return (uint32_t)R.len0[g] + (uint32_t)R.len1[g] + 3u;
}

// a chunk's sum fits 32 bits: kChunk * (2 * 65535 + 3) < 2^29
__global__ __launch_bounds__(256) void collate_cu_sum_kernel(CollateUnpaddedParams P) {
  __shared__ uint32_t s_sum;
  if (threadIdx.x == 0) s_sum = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  uint32_t s = 0, m = 0;
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    if (r < P.R.n_rows) {
      const uint32_t v = row_len(P.R, r);
      s += v;
      m = max(m, v);
    }
  }
  s = wave_incl_add(s);
  m = wave_incl_max(m);
  if ((threadIdx.x & 63) == 63) {
    atomicAdd(&s_sum, s);
    if (m) atomicMax(P.R.max_len, (int32_t)m);
  }
  __syncthreads();
  if (threadIdx.x == 0) P.chunk_sum[blockIdx.x] = s_sum;
}

__global__ __launch_bounds__(256) void collate_cu_scan_kernel(CollateUnpaddedParams P) {
  __shared__ unsigned long long s_base, s_total;
  __shared__ uint32_t s_wave[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) s_base = s_total = 0;
  __syncthreads();
  unsigned long long below = 0, all = 0;
  for (int64_t c = tid; c < P.n_chunks; c += 256) {
    const uint32_t v = P.chunk_sum[c];
    all += v;
    if (c < (int64_t)blockIdx.x) below += v;
  }
  if (below) atomicAdd(&s_base, below);
  if (all) atomicAdd(&s_total, all);
  __syncthreads();
  const int64_t total = (int64_t)s_total;
  if (blockIdx.x == 0 && tid == 0) {
    *P.total_out = total;
    if (total < (1ll << 31)) P.cu_seqlens[0] = 0;
  }
  if (total >= (1ll << 31)) return;  // refused on the host; nothing narrowed
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  int64_t carry = (int64_t)s_base;
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + tid;
    // the error word was set by the sum pass; an out-of-range row counts 0 in both
    uint32_t v = 0;
    if (r < P.R.n_rows) {
      const int64_t g = P.R.rows ? P.R.rows[r] : P.R.row0 + r;
      if (g >= 0 && g < P.R.n_total) v = (uint32_t)P.R.len0[g] + (uint32_t)P.R.len1[g] + 3u;
    }
    const uint32_t incl = wave_incl_add(v);
    if (lane == 63) s_wave[it & 1][w] = incl;
    __syncthreads();  // one per step: the steps alternate between the two rows of s_wave
    uint32_t before = 0, step = 0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t t = s_wave[it & 1][k];
      step += t;
      if (k < w) before += t;
    }
    if (r < P.R.n_rows) P.cu_seqlens[r + 1] = (int32_t)(carry + before + incl);
    carry += step;
  }
}

struct Row {
  const uint16_t* s0;  // ids + src0 - 1: token j of segment 0 is s0[j]
  const uint16_t* s1;  // ids + src1 - (a + 2)
  int32_t a, n;
};

struct Token {
  int64_t id, tt, lab;
};

// token j (0 <= j < n) of batch row r: collate_rows.hip's column<MODE>() for a
// column in front of the padding
template <int MODE>
__device__ __forceinline__ Token token(const CollateRowsParams& R, const Row& S, const uint32_t* mlm, int64_t r,
                                       int32_t j) {
  Token o;
  const int32_t a = S.a, n = S.n;
  const bool special = j == 0 || j == a + 1 || j == n - 1;
  int64_t id;
  if (j == 0) id = R.cls;
  else if (special) id = R.sep;
  else if (j <= a) id = S.s0[j];
  else id = S.s1[j];
  if (MODE == COLLATE_SPECIAL_MASK) {
    o.lab = special ? 1 : 0;
  } else if (MODE == COLLATE_STATIC) {
    const uint32_t m = mlm[j];
    o.lab = m == kNoMask ? R.ignore_index : (int64_t)(m & 0xFFFFu);
    if (m != kNoMask) id = (int64_t)(m >> 16);
  } else {
    id = mask_one(id, special, r, j, R.seed, R.counter, R.mlm_probability, R.mask_id, R.n_random, R.ignore_index,
                  o.lab);
  }
  o.id = id;
  o.tt = j >= a + 2 ? 1 : 0;
  return o;
}

}  // namespace

template <int MODE>
__global__ __launch_bounds__(256) void collate_unpadded_kernel(CollateUnpaddedParams P) {
  // mode 1 only: per wave, label | token << 16 of every masked token
  __shared__ uint32_t s_mlm[MODE == COLLATE_STATIC ? 4 : 1][MODE == COLLATE_STATIC ? COLLATE_MAX_LEN : 1];
  const CollateRowsParams& R = P.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t* mlm = s_mlm[MODE == COLLATE_STATIC ? w : 0];
  const int64_t nw = (int64_t)gridDim.x * 4;
  // 16-B stores need every output 16-B aligned at even token offsets
  const bool wide = (((uintptr_t)R.input_ids | (uintptr_t)R.token_type_ids | (uintptr_t)P.position_ids |
                      (uintptr_t)R.labels) & 15) == 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    const int64_t g = R.rows ? R.rows[r] : R.row0 + r;
    if (g < 0 || g >= R.n_total) {
      if (lane == 0) set_err(R.err, CERR_ROW_INDEX, r);
      continue;
    }
    const uint32_t fl = R.flags[g];
    if (!(fl & 2u)) {
      if (lane == 0) set_err(R.err, CERR_NO_SEP, r);
      continue;
    }
    Row S;
    S.a = R.len0[g];
    S.n = S.a + (int32_t)R.len1[g] + 3;
    const int32_t n = S.n;
    if (n > COLLATE_MAX_LEN) {
      if (lane == 0) set_err(R.err, CERR_LONG, r);
      continue;
    }
    const int64_t c0 = P.cu_seqlens[r], c1 = P.cu_seqlens[r + 1];
    if (c0 < 0 || c1 - c0 != n || c0 + n > P.total) {
      if (lane == 0) set_err(R.err, CERR_CU_SEQLENS, r);
      continue;
    }
    S.s0 = R.ids + R.src0[g] - 1;
    S.s1 = R.ids + R.src1[g] - (S.a + 2);
    if (MODE == COLLATE_STATIC) {
      __builtin_amdgcn_wave_barrier();  // the previous row's reads are done
      for (int32_t j = lane; j < n; j += 64) mlm[j] = kNoMask;
      __builtin_amdgcn_wave_barrier();
      bool bad = false;
      const int64_t k1 = R.mlm_off[g + 1];
      for (int64_t k = R.mlm_off[g] + lane; k < k1; k += 64) {
        const int32_t pos = R.mlm_pos[k];
        if (pos >= n) bad = true;  // [n, seq_len) of the padded row would be the next row here
        else mlm[pos] = (uint32_t)R.mlm_label[k] | ((uint32_t)R.mlm_token[k] << 16);
      }
      if (__ballot(bad)) {
        if (lane == 0) set_err(R.err, CERR_POS_RANGE, r);
        continue;
      }
      __builtin_amdgcn_wave_barrier();
    }
    int64_t* o_ids = R.input_ids + c0;
    int64_t* o_tt = R.token_type_ids + c0;
    int64_t* o_pos = P.position_ids + c0;
    int64_t* o_lab = R.labels + c0;
    if (wide) {
      // pair q holds tokens 2q - head and 2q - head + 1: 16-B aligned in the
      // stream.  The first pair of an odd start and the last of an odd end have
      // one token of this row (n >= 3: never the same pair, never neither).
      const int32_t head = (int32_t)(c0 & 1);
      const int32_t nq = (head + n + 1) >> 1;
      for (int32_t q = lane; q < nq; q += 64) {
        const int32_t j0 = 2 * q - head, j1 = j0 + 1;
        const bool v0 = j0 >= 0, v1 = j1 < n;
        const int32_t k0 = v0 ? j0 : 0, k1 = v1 ? j1 : n - 1;
        const Token t0 = token<MODE>(R, S, mlm, r, k0);
        const Token t1 = token<MODE>(R, S, mlm, r, k1);
        if (v0 && v1) {
          *reinterpret_cast<longlong2*>(o_ids + j0) = make_longlong2(t0.id, t1.id);
          *reinterpret_cast<longlong2*>(o_tt + j0) = make_longlong2(t0.tt, t1.tt);
          *reinterpret_cast<longlong2*>(o_pos + j0) = make_longlong2(j0, j1);
          *reinterpret_cast<longlong2*>(o_lab + j0) = make_longlong2(t0.lab, t1.lab);
        } else {
          const Token t = v0 ? t0 : t1;
          const int32_t k = v0 ? k0 : k1;
          o_ids[k] = t.id;
          o_tt[k] = t.tt;
          o_pos[k] = k;
          o_lab[k] = t.lab;
        }
      }
    } else {
      for (int32_t j = lane; j < n; j += 64) {
        const Token t = token<MODE>(R, S, mlm, r, j);
        o_ids[j] = t.id;
        o_tt[j] = t.tt;
        o_pos[j] = j;
        o_lab[j] = t.lab;
      }
    }
    if (lane == 0) R.next_sentence_labels[r] = fl & 1u;
  }
}

int64_t collate_cu_chunks(int64_t n_rows) { return (n_rows + kChunk - 1) / kChunk; }

hipError_t launch_collate_cu_seqlens(const CollateUnpaddedParams& P, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)P.n_chunks), block(256);
  hipLaunchKernelGGL(collate_cu_sum_kernel, grid, block, 0, s, P);
  hipLaunchKernelGGL(collate_cu_scan_kernel, grid, block, 0, s, P);
  return hipGetLastError();
}

hipError_t launch_collate_unpadded(const CollateUnpaddedParams& P, int32_t mode, int n_cu, hipStream_t s) {
  if (P.R.n_rows <= 0) return hipSuccess;
  int64_t g = (P.R.n_rows + 3) / 4;
  if (g > (int64_t)n_cu * 8) g = (int64_t)n_cu * 8;
  const dim3 grid((int)g), block(256);
  if (mode == COLLATE_SPECIAL_MASK)
    hipLaunchKernelGGL(collate_unpadded_kernel<COLLATE_SPECIAL_MASK>, grid, block, 0, s, P);
  else if (mode == COLLATE_STATIC) hipLaunchKernelGGL(collate_unpadded_kernel<COLLATE_STATIC>, grid, block, 0, s, P);
  else hipLaunchKernelGGL(collate_unpadded_kernel<COLLATE_DYNAMIC>, grid, block, 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
