// Exact-count span corruption (T5's `random_spans_noise_mask` over a WordPiece vocabulary; include/lddl_amd.h
// defines it): a row's number of noise tokens N and of noise spans S are functions of its length alone, and the
// draw is one uniformly random segmentation of its interior with exactly those counts.  Rows, sentinels and both
// streams are collate_corrupt.hip's; only the selection differs, and it is no walk with a carry: two uniform draws
// without replacement per row (S - 1 of the N - 1 gaps between noise tokens, S - 1 of the c - N - 1 gaps between
// the others) whose results interleave.  No counterpart in the reference.
//
// Work mapping as the two files beside it: one wave per batch row, four rows per block, grid_rows, no block-wide
// barrier.  Per row, four phases, each a few wave-wide steps:
//   select      both thresholds, the K-th smallest rank key of each gap set (K = S - 1; the keys are budget_key's
//               form under two keys of their own, so they are unique within a set): an MSD radix select, eight
//               bits a level, unit weights, as mask_budget.hip's but with two sets through the same pass.  One
//               256-bin uint32 histogram per set, filled 64 gaps a step by LDS atomics; lane l owns bins 4 l ..
//               4 l + 3, wave_incl_add, the crossing bin by ballot.  A set descends while its bin holds more than
//               one key and the budget is not met exactly; K = 0 (no cut) and K = all gaps (every span of length
//               1) take no level.  The hashes are computed again at every level: one splitmix64 per gap against
//               2 x 2045 x 8 B of keys per row
//   cut masks   each gap set again, 64 gaps a step: the ballot of key < thr is one 64-bit word, stored to LDS with
//               the set bits of the words before it in front
//   span table  lane = span, 64 spans a step.  The s-th set bit of a cut mask (a binary search over the word
//               prefix counts, then an in-word select by popcounts) gives the cumulative lengths A_s and B_s; span
//               s covers interior tokens [B_s + A_(s-1), B_s + A_s).  Each span toggles the bit of its first
//               column and of the column behind its last in a column-space mask of 32 words (LDS atomicOr; starts
//               and ends never coincide, every length being 1 at least); lane l < 32 then takes word l, a
//               prefix-xor within the word and a parity carry across the lanes turn the toggles into `selected`
//   walk        collate_corrupt.hip's, with the step's selected columns read from the mask (lane_get of the step's
//               word) instead of span_select: no hash and no word_column, only the ids.  The placement is the same
//               text, corrupt_step (collate_tokens.h)
// LDS: the histograms (2 KiB), the cut masks and their prefix counts (768 B) and the toggle words (256 B) are dead
// before staging begins, so they alias the wave's target slice, and the block stays at collate_corrupt.hip's two
// uint16 slices per wave, 32 KiB.  The 32 selection words live in the VGPRs of lanes 0..31 through the walk.
//
// Padding-free route: e_r = n - N + S and t_r = N + S + 1 need no selection, so the offsets pass is one thread per
// row that opens the row for its length and error code and leaves both counts, their chunk sums and maxima where
// corrupt_count_kernel leaves them; infill's scan kernel follows.  The fill checks both offset pairs against the
// capacities and the closed form before it selects, and against the walk's own counts before it stores.
//
// No input faults: the row opener's checks come first (a row index is range-checked before anything is loaded
// through it); a refused row sets the error word and is left unwritten; no row stores outside its own tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "collate_tokens.h"
#include "wave.h"

namespace lddl {
namespace {

// k_t = splitmix64(mask_key(seed, counter) ^ C_t) keys gap set t (include/lddl_amd.h): "SEGNOISE", "SEGPLAIN"
constexpr uint64_t kSegKey[2] = {0x5345474E4F495345ull, 0x534547504C41494Eull};
constexpr uint64_t kTakeAll = ~0ull;  // no key is that: its low 20 bits would be a gap of 2^20 - 1

// what the selection keeps in LDS; dead before the target is staged over it
struct SelectLds {
  uint32_t hist[2][256];
  unsigned long long cut[2][32];  // word w: gaps [64 w, 64 w + 64) that are cuts
  uint32_t pre[2][32];            // the cuts in the words before w
  unsigned long long col[32];     // the toggles of the column-space mask
};

struct alignas(16) WaveLds {
  uint16_t enc[COLLATE_MAX_LEN];
  union {
    uint16_t tgt[COLLATE_MAX_LEN];
    SelectLds sel;
  };
};
static_assert(sizeof(SelectLds) <= sizeof(uint16_t) * COLLATE_MAX_LEN, "the selection aliases the target slice");
static_assert(COLLATE_MAX_LEN <= 64 * 32, "a cut mask and the column mask are 32 words");

// thr[t]: the smallest key of gap set t (G[t] gaps) that is not among its K smallest; 0 for K = 0 and kTakeAll
// for K = G[t].  By the whole wave.
__device__ __forceinline__ void segment_thresholds(int64_t row, int32_t K, const int32_t (&G)[2], const uint64_t (&kt)[2],
                                                   uint32_t (&hist)[2][256], uint64_t (&thr)[2]) {
  const int lane = threadIdx.x & 63;
  bool live[2];
  uint64_t prefix[2] = {0, 0};  // the digits found so far
  uint32_t left[2];             // what is left of K for the gaps under the prefix
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    live[t] = K > 0 && K < G[t];
    thr[t] = K > 0 ? kTakeAll : 0;
    left[t] = (uint32_t)K;
  }
  for (int level = 0; level < 8 && (live[0] || live[1]); ++level) {
    const int shift = 56 - 8 * level;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) hist[t][4 * lane + i] = 0;
    wave_sync();
    const int32_t gmax = max(live[0] ? G[0] : 0, live[1] ? G[1] : 0);
    for (int32_t base = 0; base < gmax; base += 64) {
      const int32_t g = base + lane;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (live[t] && g < G[t]) {
          const uint64_t key = budget_key(kt[t], row, g);
          if (level == 0 || (key >> (shift + 8)) == prefix[t]) atomicAdd(&hist[t][(key >> shift) & 255u], 1u);
        }
      }
    }
    wave_sync();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (!live[t]) continue;
      // the first bin whose cumulative count passes `left`: there is one, the gaps under the prefix being more
      uint32_t cnt[4], sum = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cnt[i] = hist[t][4 * lane + i];
        sum += cnt[i];
      }
      uint32_t run = wave_incl_add(sum) - sum;
      int found = -1;
      uint32_t before = 0, in_bin = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (found < 0 && run + cnt[i] > left[t]) {
          found = i;
          before = run;
          in_bin = cnt[i];
        }
        run += cnt[i];
      }
      const uint64_t m = __ballot(found >= 0);
      if (!m) {  // not reached
        live[t] = false;
        continue;
      }
      const int l = __ffsll((long long)m) - 1;
      prefix[t] = prefix[t] << 8 | (4u * (uint32_t)l + (uint32_t)lane_get(found, l));
      before = lane_get(before, l);
      in_bin = lane_get(in_bin, l);
      if (in_bin == 1 || before == left[t]) {
        thr[t] = prefix[t] << shift;  // the bin's lowest key: the bins before hold exactly `left` keys
        live[t] = false;
      } else {
        left[t] -= before;
      }
    }
  }
}

// the gap of the s-th cut (1 <= s <= the cuts of the set) of a cut mask of nw words
__device__ __forceinline__ int32_t cut_select(const unsigned long long* word, const uint32_t* pre, int32_t nw, uint32_t s) {
  int32_t lo = 0, hi = nw - 1;  // the last word with fewer than s cuts in front of it
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (pre[mid] < s) lo = mid;
    else hi = mid - 1;
  }
  uint64_t x = word[lo];
  uint32_t rank = s - pre[lo] - 1;  // of the cut among the word's set bits, from 0
  int32_t pos = 0;
#pragma unroll
  for (int w = 32; w; w >>= 1) {
    const uint32_t below = (uint32_t)__popcll(x & ((1ull << w) - 1ull));
    if (rank >= below) {
      x >>= w;
      pos += w;
      rank -= below;
    }
  }
  return 64 * lo + pos;
}

// Lane l < 32: `selected` of columns [64 l, 64 l + 64) of batch row r (n columns, counts k); 0 on the other lanes.
// By the whole wave; L is dead when it returns.
__device__ __forceinline__ uint64_t segment_mask(const CollateSegmentParams& P, int64_t r, int32_t n, SegmentCounts k,
                                                 SelectLds& L) {
  const CollateRowsParams& C = P.C.I.R;
  const int lane = threadIdx.x & 63;
  if (k.S == 0) return 0;
  const int32_t S = k.S, K = S - 1;
  const int32_t total[2] = {k.N, n - 2 - k.N};    // noise tokens, the others: S <= each
  const int32_t G[2] = {total[0] - 1, total[1] - 1};  // K <= each
  const uint64_t key = mask_key(C.seed, C.counter);
  const uint64_t kt[2] = {splitmix64(key ^ kSegKey[0]), splitmix64(key ^ kSegKey[1])};
  uint64_t thr[2];
  segment_thresholds(r, K, G, kt, L.hist, thr);
  int32_t nw[2] = {0, 0};
  if (K > 0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint32_t cuts = 0;
      for (int32_t base = 0; base < G[t]; base += 64, ++nw[t]) {
        const int32_t g = base + lane;
        const bool cut = g < G[t] && (thr[t] == kTakeAll || budget_key(kt[t], r, g) < thr[t]);
        const uint64_t m = __ballot(cut);
        if (lane == 0) {
          L.cut[t][nw[t]] = m;
          L.pre[t][nw[t]] = cuts;
        }
        cuts += (uint32_t)__popcll(m);
      }
    }
  }
  if (lane < 32) L.col[lane] = 0;
  wave_sync();
  // the cumulative length of the first s spans' share of set t: the s-th cut is behind item number `gap`
  const auto cum = [&](int t, int32_t s) {
    return s <= 0 ? 0 : s >= S ? total[t] : cut_select(L.cut[t], L.pre[t], nw[t], (uint32_t)s) + 1;
  };
  for (int32_t s0 = 0; s0 < S; s0 += 64) {
    const int32_t s = s0 + lane + 1;
    if (s <= S) {
      const int32_t plain = cum(1, s);  // b_1 .. b_s lie in front of span s
      const int32_t first = 1 + plain + cum(0, s - 1), end = 1 + plain + cum(0, s);  // columns: [CLS] is column 0
      if (first < COLLATE_MAX_LEN) atomicOr(&L.col[first >> 6], 1ull << (first & 63));
      if (end < COLLATE_MAX_LEN) atomicOr(&L.col[end >> 6], 1ull << (end & 63));  // end <= n - 1
    }
  }
  wave_sync();
  uint64_t x = lane < 32 ? L.col[lane] : 0;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) x ^= x << w;  // bit j: the parity of the toggles at or below it
  const uint32_t odd = (uint32_t)(x >> 63);
  if ((wave_incl_add(odd) - odd) & 1u) x = ~x;  // a span that is open at the word's first column
  return x;
}

// The selection and the walk of open batch row r by its wave: the encoder's tokens in W.enc[0, e), the target in
// W.tgt[0, t).  e = n - N + S and t = N + S + 1, both <= n.
__device__ __forceinline__ CorruptLen segment_row(const CollateSegmentParams& P, const OpenRow& R, int64_t r,
                                                  SegmentCounts k, WaveLds& W) {
  const CollateRowsParams& C = P.C.I.R;
  const int lane = threadIdx.x & 63;
  const int32_t n = R.L.n;
  const uint64_t word = segment_mask(P, r, n, k, W.sel);
  const uint32_t lo = (uint32_t)word, hi = (uint32_t)(word >> 32);
  wave_sync();  // the selection's words are read: the target is staged over them
  CorruptWalk w;
  int step = 0;
  for (int32_t base = 0; base < n; base += 64, ++step) {
    const int32_t j = base + lane;
    const uint64_t ms = (uint64_t)lane_get(lo, step) | (uint64_t)lane_get(hi, step) << 32;
    const uint16_t id = j < n ? (uint16_t)row_id(C, R, j) : (uint16_t)0;
    corrupt_step<true>(P.C, ms, lane_in(ms), j < n, id, w, W.enc, W.tgt);
  }
  return corrupt_finish<true>(C.sep, w, W.tgt);
}

__device__ __forceinline__ SegmentCounts row_counts(const CollateSegmentParams& P, int32_t n) {
  return segment_counts(n, P.noise_density, P.mean_span, P.C.num_sentinels);
}

// ------------------------------------------------------------- padded batch --
__global__ __launch_bounds__(256) void segment_rows_kernel(CollateSegmentParams P) {
  __shared__ WaveLds s_w[4];
  const CollateRowsParams& R = P.C.I.R;
  const int lane = threadIdx.x & 63;
  WaveLds& W = s_w[threadIdx.x >> 6];
  const int32_t L = R.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const eo[2] = {R.input_ids, R.attention_mask};
  int64_t* const dout[2] = {P.C.I.decoder_input_ids, R.labels};
  const bool wide_enc = planes_aligned(eo), wide_dec = planes_aligned(dout);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R.n_rows; r += nw) {
    OpenRow S;
    const uint32_t code = open_row<true>(R, r, L, S);
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    wave_sync();  // the reads of the row before are done
    const CorruptLen n = segment_row(P, S, r, row_counts(P, S.L.n), W);  // e, t <= n_r <= L <= COLLATE_MAX_LEN
    wave_sync();
    const int64_t c0 = r * (int64_t)L;
    store_tokens<2>(eo, c0, L, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = j < n.e ? (int64_t)W.enc[j] : 0;
      v[1] = j < n.e ? 1 : 0;
    });
    store_tokens<2>(dout, c0, L, wide_dec, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = 0;
      v[1] = R.ignore_index;
      if (j < n.t) decoder_token(W.tgt, R.cls, j, v[0], v[1]);
    });
    if (lane == 0) {
      P.C.I.enc_len[r] = n.e;
      P.C.dec_len[r] = n.t;
    }
  }
}

// ------------------------------------------------------- padding-free batch --
// The closed-form e_r and t_r of every batch row into cu_enc[r + 1] and cu_dec[r + 1], their chunk sums and
// maxima: what infill_scan_kernel sums.  Lane = row; a wave's 64 rows lie in one chunk, so it adds its sums once.  A
// refused row sets the error word and counts 0 in both.  No selection.
__global__ __launch_bounds__(256) void segment_lengths_kernel(CollateSegmentParams P) {
  const CollateInfillParams& I = P.C.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); r0 < R.n_rows; r0 += stride) {
    const int64_t r = r0 + lane;
    uint32_t e = 0, t = 0;
    if (r < R.n_rows) {
      OpenRow S;
      const uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
      if (code) {
        set_err(R.err, code, r);
      } else {
        const SegmentCounts k = row_counts(P, S.L.n);
        e = (uint32_t)(S.L.n - k.N + k.S);
        t = (uint32_t)(k.N + k.S + 1);
      }
      I.cu_enc[r + 1] = (int32_t)e;
      I.cu_dec[r + 1] = (int32_t)t;
    }
    const uint32_t se = wave_incl_add(e), st = wave_incl_add(t), me = wave_incl_max(e), mt = wave_incl_max(t);
    if (lane == 63 && st) {  // a row that is not refused has t >= 1
      uint32_t* sum = I.chunk_sum + 2 * (r0 / kChunk);
      atomicAdd(&sum[0], se);
      atomicAdd(&sum[1], st);
      atomicMax(&I.max_out[0], (int32_t)me);
      atomicMax(&I.max_out[1], (int32_t)mt);
    }
  }
}

__global__ __launch_bounds__(256) void segment_unpadded_kernel(CollateSegmentParams P) {
  __shared__ WaveLds s_w[4];
  const CollateInfillParams& I = P.C.I;
  const CollateRowsParams& R = I.R;
  const int lane = threadIdx.x & 63;
  WaveLds& W = s_w[threadIdx.x >> 6];
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t* const eo[2] = {R.input_ids, I.position_ids};
  int64_t* const dout[3] = {I.decoder_input_ids, R.labels, I.decoder_position_ids};
  const bool wide_enc = planes_aligned(eo), wide_dec = planes_aligned(dout);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R.n_rows; r += nw) {
    OpenRow S;
    uint32_t code = open_row<true>(R, r, COLLATE_MAX_LEN, S);
    CorruptLen n{0, 0};
    int64_t c0 = 0, d0 = 0;
    if (!code) {
      // the offsets are checked, not trusted: each side against the stream's capacity and the closed form first,
      // then against the walk's own count, before anything of the row is stored
      const SegmentCounts k = row_counts(P, S.L.n);
      c0 = I.cu_enc[r];
      d0 = I.cu_dec[r];
      const int64_t c1 = I.cu_enc[r + 1], d1 = I.cu_dec[r + 1];
      if (!offsets_ok(c0, c1, S.L.n, I.total_enc) || !offsets_ok(d0, d1, S.L.n, I.total_dec) ||
          c1 - c0 != S.L.n - k.N + k.S || d1 - d0 != k.N + k.S + 1) {
        code = CERR_CU_SEQLENS;
      } else {
        wave_sync();  // the reads of the row before are done
        n = segment_row(P, S, r, k, W);
        wave_sync();
        if (n.e != c1 - c0 || n.t != d1 - d0) code = CERR_CU_SEQLENS;
      }
    }
    if (code) {
      if (lane == 0) set_err(R.err, code, r);
      continue;
    }
    store_tokens<2>(eo, c0, n.e, wide_enc, [&](int32_t j, int64_t(&v)[2]) {
      v[0] = W.enc[j];
      v[1] = j;
    });
    store_tokens<3>(dout, d0, n.t, wide_dec, [&](int32_t j, int64_t(&v)[3]) {
      decoder_token(W.tgt, R.cls, j, v[0], v[1]);
      v[2] = j;
    });
  }
}

}  // namespace

hipError_t launch_segment_rows(const CollateSegmentParams& P, int n_cu, hipStream_t s) {
  const int64_t n_rows = P.C.I.R.n_rows;
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(segment_rows_kernel, dim3(grid_rows(n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_segment_cu_seqlens(const CollateSegmentParams& P, hipStream_t s) {
  const int64_t n_rows = P.C.I.R.n_rows;
  if (n_rows <= 0) return hipSuccess;
  const int64_t blocks = (n_rows + 255) / 256;
  hipLaunchKernelGGL(segment_lengths_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, P);
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : launch_infill_scan(P.C.I, s);
}

hipError_t launch_segment_unpadded(const CollateSegmentParams& P, int n_cu, hipStream_t s) {
  const int64_t n_rows = P.C.I.R.n_rows;
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(segment_unpadded_kernel, dim3(grid_rows(n_rows, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
