// A shard's string columns into a GPU row table, once per shard: what
// lddl_row_spans + lddl_masked_lm_spans leave behind for a pack result, built
// from the parquet columns A, B, is_random_next and (static masking)
// masked_lm_positions, masked_lm_labels.  After it collate_rows.hip and
// collate_unpadded.hip serve files on disk as they serve a pack result.
//
// Reference: the decode-and-lookup half of the loader, done per batch there:
// lddl/torch/bert.py:42-60 `_decode_record_batch`, :83-89 and :109-124
// (`split()` and `convert_tokens_to_ids`), lddl/utils.py
// `deserialize_np_array`.  Per row r with a = #tokens of A, b = #tokens of B,
// n = a + b + 3 and k = #positions (the np.save payload / 2):
//   len0[r] = a, len1[r] = b, flags[r] = is_random_next[r] | 2
//   ids[src0[r] .. + a) = ids of A.split(), ids[src1[r] .. + b) = of B.split()
//     (a miss gives [UNK]); src0 = exclusive scan of a + b, src1 = src0 + a
//   tok_off = exclusive scan of n, mlm_off = exclusive scan of k
//   mlm_pos[mlm_off[r] + j] = positions[j], mlm_label[..] = id of
//     labels.split()[j], mlm_token[..] = what the row shows at that position
//     ([CLS], [SEP] or the A / B id there: a masked shard's A and B hold the
//     masked tokens already).
//
// A CodeBERT shard (CODE; lddl_code_rows_from_strings, the columns doc, code and
// num_tokens of pretrain_codebert.py:425-433, for which the reference has no
// loader) goes through the same three kernels.  Per row a = #tokens of doc,
// b = #tokens of code and s = num_tokens - a - b - 2, which says whether a
// [SEP] follows the doc segment:
//   len0[r] = a, len1[r] = b, flags[r] = s << 1, ids and src0 / src1 as above
//   tok_off = exclusive scan of a + b + 2 + s
// There are no static columns; the scan's second quantity is s in place of k
// (read from num_tokens again, so nothing travels through mlm_off).  A row
// whose s is not 0 or 1, or is 0 with a > 0 (doc tokens with no [SEP] to end
// them), is refused with CERR_CODE_ROW by both passes.
//
// Work mapping, as collate.hip: one wave per row, four rows per block, 64
// bytes per step, the owning lane looks its token up.  Ids go straight to
// global memory from the owning lane, 2 B each (no LDS anywhere in this file);
// the stream is 2 B per token against the 5 - 6 B of text read per token.
//
// Length pass: rows_len_kernel counts a, b and k, validates the static columns
// (np.save header, label count = position count, every position < n) and adds
// the row to its chunk's sums (one 64-bit atomic per row: ids in the low
// half, positions in the high half; the row tokens of a chunk are its ids + 3
// per row).  rows_scan_kernel is the second level of collate_row.h's chunked
// scan over two quantities, ids and positions.  k_r travels from the first
// kernel to the second in mlm_off[r + 1], which the scan then overwrites with
// the sum.
//
// Fill pass: rows_fill_kernel does not take len / src / mlm_off on trust: a wave
// counts its row's tokens again first and refuses (CERR_ROW_COUNTS) a row whose
// counts are not what the strings give, whose src1 is not src0 + len0, whose
// mlm_off[r + 1] is not mlm_off[r] + k, or whose span leaves [0, ids_cap) /
// [0, mlm_cap), before it stores anything: a refused row is left unwritten and
// a row stores only inside [src0, src0 + a + b) and [mlm_off[r], mlm_off[r + 1])
// as it was given them, within the capacities.  What one row can check ends
// there: an altered src0 that lies inside the capacity is taken, also on top of
// another row's span (the running sum is the scan's, not a row's, to know).
// Then it scans again with the lookups.  mlm_token reads the ids the wave has
// just stored (after a fence and a wave barrier), at the column RowLayout
// (collate_row.h) gives the position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {
namespace {

constexpr int64_t kMaxSeg = 65535;   // len0 / len1 are u16
constexpr int64_t kMaxMask = 2 * kMaxSeg + 3;  // positions of a row: at most its tokens
// a chunk's sums fit 32 bits each: kChunk * 2 * kMaxSeg and kChunk * kMaxMask < 2^29

__device__ __forceinline__ int32_t count_tokens(const uint8_t* p, int64_t s, int64_t e) {
  return scan_tokens(p, s, e, [](int32_t, int64_t) {});
}

// the static columns of row r whose row holds n tokens: 0 and (d, np) = the
// positions, or the error code
__device__ __forceinline__ uint32_t static_columns(const RowsFromStringsParams& P, int64_t r, int32_t n,
                                                   const uint8_t*& d, int64_t& np) {
  const int lane = threadIdx.x & 63;
  const StringColumns& C = P.C;
  if (!npy_u16_payload(C.pos + C.pos_off[r], C.pos_off[r + 1] - C.pos_off[r], d, np)) return CERR_NPY;
  if (np > kMaxMask) return CERR_NMASK;
  if ((int64_t)count_tokens(C.lab, C.lab_off[r], C.lab_off[r + 1]) != np) return CERR_NLAB;
  bool bad = false;
  for (int32_t j = lane; j < (int32_t)np; j += 64) {
    const int32_t pos = (int32_t)d[2 * j] | ((int32_t)d[2 * j + 1] << 8);
    if (pos >= n) bad = true;
  }
  return __ballot(bad) ? CERR_POS_RANGE : 0u;
}

// CodeBERT: s of row r whose segments hold na and nb tokens, or -1 when num_tokens[r] allows none
__device__ __forceinline__ int32_t code_sep(const RowsFromStringsParams& P, int64_t r, int32_t na, int32_t nb) {
  const int32_t s = (int32_t)P.num_tokens[r] - na - nb - 2;
  return (s == 1 || (s == 0 && na == 0)) ? s : -1;
}

}  // namespace

template <bool CODE>
__global__ __launch_bounds__(256) void rows_len_kernel(RowsFromStringsParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < P.n_rows; r += nw) {
    int32_t na = count_tokens(P.C.a, P.C.a_off[r], P.C.a_off[r + 1]);
    int32_t nb = count_tokens(P.C.b, P.C.b_off[r], P.C.b_off[r + 1]);
    uint32_t code = (na > kMaxSeg || nb > kMaxSeg) ? (uint32_t)CERR_LONG : 0u;
    int64_t np = 0;  // the high half of the chunk sum: masked positions, or (CODE) s
    if (CODE) {
      if (!code && (np = code_sep(P, r, na, nb)) < 0) code = CERR_CODE_ROW;
    } else if (P.C.pos && !code) {
      const uint8_t* d;
      code = static_columns(P, r, na + nb + 3, d, np);
    }
    if (code) na = nb = 0, np = 0;  // the call fails; the scan still reads defined counts
    if (lane == 0) {
      if (code) set_err(P.err, code, r);
      P.len0[r] = (uint16_t)na;
      P.len1[r] = (uint16_t)nb;
      if (P.mlm_off) P.mlm_off[r + 1] = np;
      atomicAdd(&P.chunk_sum[r / kChunk], (unsigned long long)(na + nb) | ((unsigned long long)np << 32));
    }
  }
}

template <bool CODE>
__global__ __launch_bounds__(256) void rows_scan_kernel(RowsFromStringsParams P) {
  __shared__ ChunkScanLds<2> S;
  chunk_scan_bases(S, P.n_chunks, [&](int64_t c, unsigned long long (&q)[2]) {
    const unsigned long long v = P.chunk_sum[c];
    q[0] = v & 0xFFFFFFFFull;
    q[1] = v >> 32;
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    P.totals[0] = (int64_t)S.total[0];
    P.totals[1] = (int64_t)S.total[0] + (CODE ? 2 * P.n_rows + (int64_t)S.total[1] : 3 * P.n_rows);
    P.totals[2] = (int64_t)S.total[1];
    if (P.tok_off) P.tok_off[0] = 0;
    if (P.mlm_off) P.mlm_off[0] = 0;
  }
  const int64_t lo = (int64_t)blockIdx.x * kChunk;
  int64_t carry[2] = {(int64_t)S.base[0], (int64_t)S.base[1]}, end[2];  // ids, positions (CODE: rows with s = 1)
  for (int it = 0; it < kChunk / 256; ++it) {
    const int64_t r = lo + it * 256 + threadIdx.x;
    uint32_t a = 0, b = 0, k = 0;
    if (r < P.n_rows) {
      a = P.len0[r];
      b = P.len1[r];
      if (CODE) k = code_sep(P, r, (int32_t)a, (int32_t)b) == 1;  // a row the length kernel refused counts 0
      else if (P.mlm_off) k = (uint32_t)P.mlm_off[r + 1];  // rows_len_kernel's k_r <= kMaxMask
    }
    const uint32_t v[2] = {a + b, k};
    chunk_scan_step(S, it, v, carry, end);
    if (r < P.n_rows) {
      P.src0[r] = end[0] - (a + b);  // end[0]: the ids of rows [0, r]
      P.src1[r] = end[0] - b;
      if (P.tok_off) P.tok_off[r + 1] = end[0] + (CODE ? 2 * (r + 1) + end[1] : 3 * (r + 1));
      if (P.mlm_off) P.mlm_off[r + 1] = end[1];
    }
  }
}

template <bool CODE>
__global__ __launch_bounds__(256) void rows_fill_kernel(RowsFromStringsParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const bool stat = !CODE && P.C.pos != nullptr;
  const CollateVocab& V = P.V;
  const StringColumns& C = P.C;
  {
    // a table that ends beyond a capacity: every wave leaves, nothing is written
    const int64_t last = P.n_rows - 1;
    const int64_t mend = stat ? P.mlm_off[P.n_rows] : 0;
    // (compared without adding to an offset that is not trusted: no sum can wrap)
    if (P.src0[last] > P.ids_cap - (int64_t)P.len0[last] - (int64_t)P.len1[last] || mend > P.mlm_cap) {
      if (blockIdx.x == 0 && threadIdx.x == 0) set_err(P.err, CERR_TABLE_CAP, last);
      return;
    }
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < P.n_rows; r += nw) {
    const int64_t a0 = C.a_off[r], a1 = C.a_off[r + 1], b0 = C.b_off[r], b1 = C.b_off[r + 1];
    // the row's counts again, and its spans against them and the capacities
    const int32_t na = count_tokens(C.a, a0, a1);
    const int32_t nb = count_tokens(C.b, b0, b1);
    const int64_t s0 = P.src0[r], s1 = P.src1[r];
    uint32_t code = 0;
    // s0 is bounded before anything is added to it
    if (na != (int32_t)P.len0[r] || nb != (int32_t)P.len1[r] || s0 < 0 || s0 > P.ids_cap - na - nb || s1 != s0 + na)
      code = CERR_ROW_COUNTS;
    const int32_t sep = CODE ? code_sep(P, r, na, nb) : 1;
    if (!code && sep < 0) code = CERR_CODE_ROW;
    const RowLayout S{na, na + nb + 3};  // (the static columns': BERT rows)
    const uint8_t* d = nullptr;
    int64_t np = 0, m0 = 0;
    if (stat && !code) {
      code = static_columns(P, r, S.n, d, np);
      m0 = P.mlm_off[r];
      if (!code && (m0 < 0 || m0 > P.mlm_cap - np || P.mlm_off[r + 1] != m0 + np)) code = CERR_ROW_COUNTS;
    }
    if (code) {
      if (lane == 0) set_err(P.err, code, r);
      continue;
    }
    uint16_t* oa = P.ids + s0;
    uint16_t* ob = P.ids + s1;
    scan_tokens(C.a, a0, a1, [&](int32_t k, int64_t i) {
      int64_t end;
      const int32_t id = vocab_lookup(V, C.a, i, a1, end);
      if (k < na) oa[k] = (uint16_t)id;
    });
    scan_tokens(C.b, b0, b1, [&](int32_t k, int64_t i) {
      int64_t end;
      const int32_t id = vocab_lookup(V, C.b, i, b1, end);
      if (k < nb) ob[k] = (uint16_t)id;
    });
    if (lane == 0) P.flags[r] = CODE ? (uint8_t)(sep << 1) : (uint8_t)((P.is_random_next[r] ? 1u : 0u) | 2u);
    if (stat && np > 0) {
      // the ids other lanes of this wave stored are read below: the stores are made visible, and no lane's load
      // is scheduled in front of the point all lanes have reached
      __threadfence();
      __builtin_amdgcn_wave_barrier();
      const int64_t l1 = C.lab_off[r + 1];
      scan_tokens(C.lab, C.lab_off[r], l1, [&](int32_t k, int64_t i) {
        int64_t end;
        const int32_t id = vocab_lookup(V, C.lab, i, l1, end);
        if (k >= (int32_t)np) return;
        const int32_t pos = (int32_t)d[2 * k] | ((int32_t)d[2 * k + 1] << 8);  // < n: static_columns
        const int32_t shown = S.base_id(pos, V.cls, V.sep, [&](int32_t c) {
          return (int32_t)(c <= na ? oa[c - 1] : ob[c - na - 2]);
        });
        P.mlm_pos[m0 + k] = (uint16_t)pos;
        P.mlm_label[m0 + k] = (uint16_t)id;
        P.mlm_token[m0 + k] = (uint16_t)shown;
      });
    }
  }
}

hipError_t launch_rows_from_strings_len(const RowsFromStringsParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  if (P.num_tokens) {
    hipLaunchKernelGGL(rows_len_kernel<true>, dim3(grid_rows(P.n_rows, n_cu)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(rows_scan_kernel<true>, dim3((unsigned)P.n_chunks), dim3(256), 0, s, P);
  } else {
    hipLaunchKernelGGL(rows_len_kernel<false>, dim3(grid_rows(P.n_rows, n_cu)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(rows_scan_kernel<false>, dim3((unsigned)P.n_chunks), dim3(256), 0, s, P);
  }
  return hipGetLastError();
}

hipError_t launch_rows_from_strings(const RowsFromStringsParams& P, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  if (P.num_tokens) hipLaunchKernelGGL(rows_fill_kernel<true>, dim3(grid_rows(P.n_rows, n_cu)), dim3(256), 0, s, P);
  else hipLaunchKernelGGL(rows_fill_kernel<false>, dim3(grid_rows(P.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
