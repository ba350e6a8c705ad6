// BART's full denoising collate (include/lddl_amd.h defines it: lddl_collate_denoise_rows*): the sentences of every
// segment of a row are permuted, text infilling (collate_infill.hip) runs over the permuted row, and an opened
// [MASK] may become a random id.  The decoder is teacher-forced on the row as the table holds it.  A sentence ends
// at a full-stop token, fairseq's rule; the reference's BART preprocessor stops at the text column.
//
// The permuted row has to exist before the selection runs (word starts and the draws' columns are its own), so this
// is infill's kernel with a prologue.  Work mapping: infill's, one wave per batch row, four rows per block, no
// block-wide barrier.  Per wave two uint16 slices of 2048 in LDS, 8 KiB, 32 KiB per block:
//   perm   the permuted row; before it the 32-bit sentence keys of one segment (<= 1024 x 4 B), then the
//          ordering of that segment (<= 1024 x 2 B)
//   enc    the encoder's tokens; before them two tables of 1024 x 2 B over the sentences of the row, both segments
//          in one numbering (a row of n <= 2048 columns has 1024 sentences at most): `first`, a sentence's first
//          column (11 bits) with its chosen flag in bit 15, and `slot`, rank -> sentence while a segment is ranked,
//          then a sentence's first column in the permuted row
// The steps of a row:
//   firsts   64 columns a step, lane = column: the stop ballot, shifted up by one with the step before's last bit
//            shifted in, gives end(j); the end ballot, shifted the same way, gives the columns that open a
//            sentence; a sentence's number is the running count + the ballot's bits below the lane
//   rank     per segment, lane = sentence: the keys of m <= 64 sentences stay in registers and meet through m
//            lane reads; beyond that they go to LDS and every lane counts the smaller ones over broadcast reads,
//            m * ceil(m / 64) of them (1024 sentences: 16384).  A chosen sentence (rank < K) sets its flag and
//            slot[rank]
//   order    lane = position: the k of a chosen position by the flag ballot's prefix count, its sentence slot[k];
//            the ordering goes to perm (the keys are dead).  Then the destination of position p is the running sum
//            of the lengths in front of it (a wave scan with a carry across steps), stored by sentence in slot
//            (the ranks are dead)
//   gather   the firsts walk again, lane = column: column j of sentence i goes to slot[i] + j - first[i] of perm;
//            [CLS] and the [SEP]s stay.  2-B loads from the row table, L2 hits
//   walk     infill_walk (collate_tokens.h) with perm as its token source; the replacement draw at the emit
// then the planes leave as in collate_infill.hip.  The count pass of the padding-free route runs all of it but the
// staging of enc: the selection depends on the permuted row.
//
// No input faults: the row opener's checks come first; a refused row sets the error word and is left unwritten;
// every LDS index is below the 1024 sentences or the n columns of the open row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "collate_tokens.h"
#include "wave.h"

namespace lddl {
namespace {

constexpr int kMaxSent = COLLATE_MAX_LEN / 2;
constexpr uint64_t kPermuteKey = 0x5045524D53454E54ull;  // "PERMSENT"
constexpr uint64_t kReplaceKey = 0x52414E44544F4B4Eull;  // "RANDTOKN"
constexpr uint16_t kChosen = 0x8000, kColumn = 0x07FF;

// h32 of sentence i of segment g of batch row r
__device__ __forceinline__ uint32_t sentence_key(uint64_t kp, int64_t r, int32_t g, int32_t i) {
  return (uint32_t)(splitmix64(kp + mask_idx(r, g << 11 | i)) >> 32);
}

// key t is below key i: (h32, index) in lexicographic order
__device__ __forceinline__ int32_t key_below(uint32_t kt, int32_t t, uint32_t ki, int32_t i) {
  return kt < ki || (kt == ki && t < i) ? 1 : 0;
}

// What the firsts walk carries from step to step, wave-uniform
struct FirstsWalk {
  int32_t sentences = 0, seg0 = 0;  // opened so far; those of segment 0
  uint64_t last_stop = 0, last_end = 0;
};

// One step: whether this lane's column j opens a sentence, and the ballot of that.  id: the row table's id at j.
__device__ __forceinline__ uint64_t firsts_step(const CollateDenoiseParams& P, const OpenRow& R, int32_t j, bool valid,
                                                int32_t id, FirstsWalk& w, bool& first) {
  const bool sp = !valid || R.L.special(j);
  const bool stop = !sp && id == P.full_stop_id;
  const uint64_t ms = __ballot(stop);
  // the column in front of a segment is special, no stop: fairseq's rule needs no j > lo
  const bool end = !sp && ((stop && !lane_in(ms << 1 | w.last_stop)) || R.L.special(j + 1));
  const uint64_t me = __ballot(end);
  first = !sp && (R.L.special(j - 1) || lane_in(me << 1 | w.last_end));
  const uint64_t mf = __ballot(first);
  w.seg0 += (int32_t)__popcll(mf & __ballot(j <= R.L.a));
  w.last_stop = ms >> 63;
  w.last_end = me >> 63;
  return mf;
}

// Segment [lo, hi) of the open row, sentences [og, og + m) of the row's numbering, m >= 1: ranks, ordering and
// the sentences' places in the permuted row (slot[og ..)).  g: the segment's number in the keys.
__device__ __forceinline__ void permute_segment(const CollateDenoiseParams& P, int64_t r, int32_t g, int32_t lo, int32_t hi,
                                                int32_t og, int32_t m, uint16_t* perm, uint16_t* first, uint16_t* slot) {
  const int lane = threadIdx.x & 63;
  const int32_t K = denoise_permuted(m, P.permute_ratio);
  if (K >= 2) {
    const uint64_t kp = splitmix64(mask_key(P.I.R.seed, P.I.R.counter) ^ kPermuteKey);
    if (m <= 64) {
      const uint32_t key = sentence_key(kp, r, g, lane);
      int32_t rank = 0;
      for (int32_t t = 0; t < m; ++t) rank += key_below(lane_get(key, t), t, key, lane);
      if (lane < m && rank < K) {
        slot[og + rank] = (uint16_t)(og + lane);
        first[og + lane] |= kChosen;
      }
    } else {
      uint32_t* keys = reinterpret_cast<uint32_t*>(perm);
      for (int32_t i = lane; i < m; i += 64) keys[i] = sentence_key(kp, r, g, i);
      wave_sync();
      for (int32_t ib = 0; ib < m; ib += 64) {
        const int32_t i = ib + lane;
        const uint32_t key = keys[i < m ? i : 0];
        int32_t rank = 0;
#pragma unroll 8
        for (int32_t t = 0; t < m; ++t) rank += key_below(keys[t], t, key, i);  // every lane reads one address
        if (i < m && rank < K) {
          slot[og + rank] = (uint16_t)(og + i);
          first[og + i] |= kChosen;
        }
      }
    }
  }
  wave_sync();  // the keys are dead, the flags and slot[og, og + K) are set
  // ordering[p], in the row's numbering, by position p of the segment
  int32_t k = 0;
  for (int32_t pb = 0; pb < m; pb += 64) {
    const int32_t p = pb + lane;
    const bool chosen = p < m && (first[og + p] & kChosen);
    const uint64_t mc = __ballot(chosen);
    if (p < m) perm[p] = chosen ? slot[og + k + bits_below(mc)] : (uint16_t)(og + p);
    k += (int32_t)__popcll(mc);
  }
  wave_sync();  // the ranks are dead
  int32_t dest = lo;
  for (int32_t pb = 0; pb < m; pb += 64) {
    const int32_t p = pb + lane;
    int32_t o = 0, len = 0;
    if (p < m) {
      o = perm[p];
      len = (o == og + m - 1 ? hi : (int32_t)(first[o + 1] & kColumn)) - (int32_t)(first[o] & kColumn);
    }
    const int32_t incl = wave_incl_add(len);
    if (p < m) slot[o] = (uint16_t)(dest + incl - len);
    dest += lane_get(incl, 63);
  }
  wave_sync();  // the ordering is dead: perm is free for the next segment's keys, or for the row
}

// The permuted row of open batch row r into perm[0, n); tab: the wave's other slice, clobbered
__device__ __forceinline__ void permute_row(const CollateDenoiseParams& P, const OpenRow& R, int64_t r, uint16_t* perm,
                                            uint16_t* tab) {
  const CollateRowsParams& C = P.I.R;
  const int lane = threadIdx.x & 63;
  const int32_t n = R.L.n;
  uint16_t *first = tab, *slot = tab + kMaxSent;
  FirstsWalk w;
  for (int32_t base = 0; base < n; base += 64) {
    const int32_t j = base + lane;
    bool opens;
    const uint64_t mf = firsts_step(P, R, j, j < n, j < n ? (int32_t)row_id(C, R, j) : 0, w, opens);
    const int32_t i = w.sentences + bits_below(mf);
    if (opens && i < kMaxSent) first[i] = (uint16_t)j;
    w.sentences += (int32_t)__popcll(mf);
  }
  const int32_t M = min(w.sentences, kMaxSent), m0 = min(w.seg0, M);  // (the bound holds for every row of n <= 2048)
  wave_sync();
  // segment 0 is [1, a + 1); segment 1 what lies between the inner [SEP], if there is one, and the last
  if (m0) permute_segment(P, r, 0, 1, R.L.a + 1, 0, m0, perm, first, slot);
  if (M - m0) permute_segment(P, r, R.L.s, R.L.a + 1 + R.L.s, n - 1, m0, M - m0, perm, first, slot);
  w = FirstsWalk{};
  for (int32_t base = 0; base < n; base += 64) {
    const int32_t j = base + lane;
    const int32_t id = j < n ? (int32_t)row_id(C, R, j) : 0;
    bool opens;
    const uint64_t mf = firsts_step(P, R, j, j < n, id, w, opens);
    const int32_t i = w.sentences + bits_below(mf) + (opens ? 1 : 0) - 1;  // the sentence of a column of a segment
    if (j < n) {
      int32_t to = j;
      if (!R.L.special(j) && i < M) to = (int32_t)slot[i] + j - (int32_t)(first[i] & kColumn);
      perm[to] = (uint16_t)id;
    }
    w.sentences += (int32_t)__popcll(mf);
  }
  wave_sync();
}

// permute_row, then text infilling's walk over perm: e_r, and with STAGE the encoder's tokens in enc[0, e_r)
template <bool STAGE>
__device__ __forceinline__ int32_t denoise_row(const CollateDenoiseParams& P, const OpenRow& R, int64_t r, uint16_t* perm,
                                               uint16_t* enc) {
  const CollateRowsParams& C = P.I.R;
  permute_row(P, R, r, perm, enc);
  const uint64_t kr = splitmix64(mask_key(C.seed, C.counter) ^ kReplaceKey);
  return infill_walk<STAGE>(
      C, R, r, enc, [&](int32_t k) { return (int32_t)perm[k]; },
      [&](int32_t j) {
        const uint64_t h = splitmix64(kr + mask_idx(r, j));
        return unit53(h) < P.random_ratio ? (int32_t)(((h & 0xFFFFFFFFull) * (uint64_t)C.n_random) >> 32) : C.mask_id;
      });
}

// ------------------------------------------------------------- padded batch --
__global__ __launch_bounds__(256) void denoise_rows_kernel(CollateDenoiseParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t s_tok[4][2][COLLATE_MAX_LEN];
  const CollateInfillParams& I = P.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t *perm = s_tok[w][0], *tok = s_tok[w][1];
  const int32_t L = R.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const enc[2] = {R.input_ids, R.attention_mask};
  int64_t* const dec[2] = {I.decoder_input_ids, R.labels};
  const bool wide_enc = planes_aligned(enc), wide_dec = planes_aligned(dec);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, L, S);
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    wave_sync();  // the reads of the row before are done
    const int32_t e = denoise_row<true>(P, S, r, perm, tok);  // e <= n <= L <= COLLATE_MAX_LEN
    wave_sync();
    const int64_t c0 = r * (int64_t)L;
    store_tokens<2>(enc, c0, L, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < e ? (int64_t)tok[j] : 0;
      v[1] = j < e ? 1 : 0;
    });
    const int32_t m = S.L.n - 1;
    store_tokens<2>(dec, c0, L, wide_dec, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < m ? row_id(R, S, j) : 0;
      v[1] = j < m ? row_id(R, S, j + 1) : R.ignore_index;
    });
    if (lane == 0) I.enc_len[r] = e;
  }
}

// ------------------------------------------------------- padding-free batch --
// what infill_count_kernel leaves, for launch_infill_scan
__global__ __launch_bounds__(256) void denoise_count_kernel(CollateDenoiseParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t s_tok[4][2][COLLATE_MAX_LEN];
  const CollateInfillParams& I = P.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    int32_t e = 0, m = 0;
    if (!code) {
      wave_sync();
      e = denoise_row<false>(P, S, r, s_tok[w][0], s_tok[w][1]);
      m = S.L.n - 1;
    }
    if (lane == 0) {
      if (code) set_err(R.err, code, r);
      I.cu_enc[r + 1] = e;
      I.cu_dec[r + 1] = m;
      if (!code) {  // e >= 2 and m >= 1
        uint32_t* sum = I.chunk_sum + 2 * (r / kChunk);
        atomicAdd(&sum[0], (uint32_t)e);
        atomicAdd(&sum[1], (uint32_t)m);
        atomicMax(&I.max_out[0], e);
        atomicMax(&I.max_out[1], m);
      }
    }
  }
}

__global__ __launch_bounds__(256) void denoise_unpadded_kernel(CollateDenoiseParams P) {
  __shared__ __attribute__((aligned(16))) uint16_t s_tok[4][2][COLLATE_MAX_LEN];
  const CollateInfillParams& I = P.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint16_t *perm = s_tok[w][0], *tok = s_tok[w][1];
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const enc[2] = {R.input_ids, I.position_ids};
  int64_t* const dec[3] = {I.decoder_input_ids, R.labels, I.decoder_position_ids};
  const bool wide_enc = planes_aligned(enc), wide_dec = planes_aligned(dec);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < R.n_rows; r += nw) {
    OpenRow S;
    uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    int32_t e = 0, m = 0;
    int64_t c0 = 0, d0 = 0;
    if (!code) {
      // the offsets are checked, not trusted: the decoder's against n_r - 1, the encoder's against the walk's count
      m = S.L.n - 1;
      c0 = I.cu_enc[r];
      d0 = I.cu_dec[r];
      const int64_t c1 = I.cu_enc[r + 1], d1 = I.cu_dec[r + 1];
      if (!offsets_ok(c0, c1, S.L.n, I.total_enc) || d0 < 0 || d1 - d0 != m || d0 + m > I.total_dec) {
        code = CERR_CU_SEQLENS;
      } else {
        wave_sync();  // the reads of the row before are done
        e = denoise_row<true>(P, S, r, perm, tok);
        wave_sync();
        if (e != c1 - c0) code = CERR_CU_SEQLENS;
      }
    }
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    store_tokens<2>(enc, c0, e, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = tok[j];
      v[1] = j;
    });
    store_tokens<3>(dec, d0, m, wide_dec, [&](int32_t j, int64_t(&v)[3]) {
      v[0] = row_id(R, S, j);
      v[1] = row_id(R, S, j + 1);
      v[2] = j;
    });
  }
}

}  // namespace

hipError_t launch_denoise_rows(const CollateDenoiseParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_rows_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_denoise_cu_seqlens(const CollateDenoiseParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_count_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return launch_infill_scan(P.I, s);
}

hipError_t launch_denoise_unpadded(const CollateDenoiseParams& P, int n_cu, hipStream_t s) {
  if (P.I.R.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(denoise_unpadded_kernel, dim3(grid_rows(P.I.R.n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
