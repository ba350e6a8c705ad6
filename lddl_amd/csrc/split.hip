// Rule-based sentence split on the device (kernels of lddl_split_len / lddl_split).
//
// The host front end splits a record with preprocess._rule_split (a regex walk with a running start) after
// split_id_text, strips every piece and drops the empty ones (host/split_rules.c is the same in C).  The rule is
// position-local: whether byte p starts a new sentence depends only on the bytes of p's record to its left --
//   1. p starts a non-whitespace code point and the code point before it is whitespace;
//   2. left of that whitespace run (back to w) lie closers ["')\]]* and before them a run of [.!?], maximal to
//      the left and starting at ms, all at or after the body's start b0;
//   3. the code point at p is upper case, a digit or one of " ' ( [;
//   4. if buf[ms] == '.', the whitespace-delimited word before ms (bounded by b0), lowered and stripped of
//      ( " ' [, is neither a known abbreviation nor a single alphabetic code point.
// A record's sentences start at the first non-whitespace byte of its body and at every break; each ends at the
// w of the next break, the last at the body's end stripped of whitespace.
//
// Mapping: the buffer is cut into pieces of SPLIT_PIECE bytes that ignore record boundaries; a wave owns a
// piece and takes it 64 bytes per step, a byte per lane.  A lane whose byte passes the cheap tests (3, then 1,
// then the byte before the closers) finds its record by bisection among the records that touch the piece and
// does the leftward walks itself; they read before the piece as far as the rule asks, never before b0.
//   head   a lane per record: rec_off checks, id end, b0, first sentence start, stripped end;
//   count  a wave per piece: strict UTF-8 (a sequence belongs to its lead byte), breaks per record (atomics
//          gathered per wave and record), sentence bytes; with a fill, sentence starts per piece;
//   mark   a wave per piece (fill): sentence k's start, and the end of sentence k - 1 at a break;
//   tail   a lane per record (fill): the end of its last sentence;
//   lens / copy  a lane / a wave per sentence: lengths (scanned into sent_off) and the bytes.
// UTF-8 is checked over the buffer as a whole; together with "no record starts on a continuation byte"
// (head) that is strict UTF-8 record by record, and the lowest offending record is kept by atomicMin.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "split.h"
#include "wave.h"

namespace lddl {
namespace {

__device__ __forceinline__ bool is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
__device__ __forceinline__ bool is_punct(uint32_t b) { return b == '.' || b == '!' || b == '?'; }
__device__ __forceinline__ bool is_close(uint32_t b) { return b == '"' || b == '\'' || b == ')' || b == ']'; }
__device__ __forceinline__ bool is_strip(uint32_t b) { return b == '(' || b == '"' || b == '\'' || b == '['; }

// continuation bytes a lead byte asks for; 0 for a byte that leads nothing
__device__ __forceinline__ int lead_need(uint32_t b) {
  return b >= 0xC2 && b <= 0xDF ? 1 : b >= 0xE0 && b <= 0xEF ? 2 : b >= 0xF0 && b <= 0xF4 ? 3 : 0;
}

// strict UTF-8 decode of the code point at s[i] (i < n), no byte at or past n read: its length in len, -1 when
// invalid (overlong, surrogate, > U+10FFFF, truncated, not a lead byte); split_rules.c dec()
__device__ __forceinline__ int32_t dec(const uint8_t* s, int64_t i, int64_t n, int& len) {
  const uint32_t b = s[i];
  len = 1;
  if (b < 0x80) return (int32_t)b;
  const int k = lead_need(b);
  if (k == 0 || i + k >= n) return -1;
  uint32_t c = b & (0x3Fu >> k);
  for (int j = 1; j <= k; ++j) {
    const uint32_t x = s[i + j];
    if (!is_cont(x)) return -1;
    c = (c << 6) | (x & 0x3F);
  }
  const uint32_t lo = k == 1 ? 0x80u : k == 2 ? 0x800u : 0x10000u;
  if (c < lo || c > 0x10FFFFu || (c >= 0xD800u && c <= 0xDFFFu)) return -1;
  len = k + 1;
  return (int32_t)c;
}

// the code point at [i, n) is whitespace; len = its bytes (1 when it does not decode)
__device__ __forceinline__ bool space_at(const uint8_t* s, int64_t i, int64_t n, const uint8_t* tab, int& len) {
  const int32_t c = dec(s, i, n, len);
  return c >= 0 && (tab[c] & SP_SPACE);
}

// start of the code point ending just before byte i (i > lo)
__device__ __forceinline__ int64_t back(const uint8_t* s, int64_t i, int64_t lo) {
  --i;
  for (int k = 0; k < 3 && i > lo && is_cont(s[i]); ++k) --i;
  return i;
}

// the last record of [lo, hi) that starts at or before p (rec_off[lo] <= p): the one holding byte p
__device__ __forceinline__ int64_t rec_of(const int64_t* rec_off, int64_t lo, int64_t hi, int64_t p) {
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (rec_off[m] <= p) lo = m;
    else hi = m;
  }
  return lo;
}

constexpr uint64_t abbrev_key(const char* s) {
  uint64_t k = 0;
  for (int i = 0; s[i]; ++i) k |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return k;
}
// preprocess._ABBREV, a word's bytes packed low byte first
#define A(s) abbrev_key(s)
__device__ const uint64_t ABBREV_KEYS[] = {
    A("mr"),  A("mrs"),  A("ms"),  A("dr"),  A("prof"), A("sr"),  A("jr"),  A("st"),  A("vs"),  A("etc"), A("e.g"),
    A("i.e"), A("inc"),  A("ltd"), A("co"),  A("corp"), A("jan"), A("feb"), A("mar"), A("apr"), A("jun"), A("jul"),
    A("aug"), A("sep"),  A("sept"), A("oct"), A("nov"), A("dec"), A("no"),  A("fig"), A("al"),  A("approx"),
    A("dept"), A("est"), A("gen"), A("gov"), A("lt"),   A("mt"),  A("rev"), A("sgt"), A("u.s"), A("u.k")};
#undef A
constexpr int N_ABBREV = sizeof(ABBREV_KEYS) / sizeof(ABBREV_KEYS[0]);

// the word [a, e) before a '.' is an abbreviation or a one-letter initial (split_rules.c no_break_word)
__device__ __forceinline__ bool no_break_word(const uint8_t* s, int64_t a, int64_t e, const uint8_t* tab) {
  while (a < e && is_strip(s[a])) ++a;
  while (e > a && is_strip(s[e - 1])) --e;
  if (a >= e) return false;
  int len;
  const int32_t c0 = dec(s, a, e, len);
  if (c0 >= 0 && a + len == e) return (tab[c0] & SP_ALPHA1) != 0;
  uint64_t key = 0;
  int m = 0;
  for (int64_t i = a; i < e; i += len) {
    const int32_t c = dec(s, i, e, len);
    if (c < 0 || m >= 7) return false;
    uint32_t ch;
    if (c < 0x80) ch = c >= 'A' && c <= 'Z' ? c + 32 : c;
    else if (c == 0x212A) ch = 'k';
    else return false;
    key |= (uint64_t)ch << (8 * m++);
  }
  bool hit = false;
  for (int k = 0; k < N_ABBREV; ++k) hit |= ABBREV_KEYS[k] == key;
  return hit;
}

// Byte p (0 < p < nbytes, value B) starts a new sentence of its record: where the sentence before it ends (the
// start of the whitespace run before p), else -1.  [rlo, rhi): records among which p's lies.
__device__ __forceinline__ int64_t find_break(const SentSplitParams& P, int64_t p, uint32_t B, int64_t rlo, int64_t rhi) {
  if (is_cont(B)) return -1;
  const uint8_t* const s = P.buf;
  const uint8_t* const tab = P.props;
  int len;
  const int32_t c = dec(s, p, P.nbytes, len);
  if (c < 0) return -1;
  if (!((tab[c] & (SP_UPPER | SP_DIGIT)) || c == '"' || c == '\'' || c == '(' || c == '[')) return -1;
  // the whitespace run and the closers before p, not yet bounded by the record: a walk that leaves the body
  // ends below b0 and is refused there
  int64_t w = p;
  while (w > 0) {
    const int64_t q = back(s, w, 0);
    if (!space_at(s, q, w, tab, len)) break;
    w = q;
  }
  if (w == p) return -1;
  int64_t j = w;
  while (j > 0 && is_close(s[j - 1])) --j;
  if (j == 0 || !is_punct(s[j - 1])) return -1;
  const int64_t r = rec_of(P.rec_off, rlo, rhi, p);
  const int64_t b0 = P.rec_b0[r];
  if (j <= b0) return -1;  // the punctuation at j - 1 lies before the body
  int64_t ms = j - 1;
  while (ms > b0 && is_punct(s[ms - 1])) --ms;
  if (s[ms] == '.') {
    int64_t e = ms;
    while (e > b0) {
      const int64_t q = back(s, e, b0);
      if (!space_at(s, q, e, tab, len)) break;
      e = q;
    }
    int64_t a = e;
    while (a > b0) {
      const int64_t q = back(s, a, b0);
      if (space_at(s, q, a, tab, len)) break;
      a = q;
    }
    if (no_break_word(s, a, e, tab)) return -1;
  }
  return w;
}

__device__ __forceinline__ int64_t wave_sum(int64_t x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__device__ __forceinline__ void set_err(uint32_t* err, uint32_t code) { atomicCAS(err, 0u, code); }

}  // namespace

__global__ __launch_bounds__(256) void split_head_kernel(SentSplitParams P) {
  const uint8_t* const s = P.buf;
  const uint8_t* const tab = P.props;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0 && (P.rec_off[0] != 0 || P.rec_off[P.n_rec] != P.nbytes)) set_err(P.err, SPLIT_E_RECOFF);
  int64_t bytes = 0;
  for (int64_t r = t0; r < P.n_rec; r += stride) {
    const int64_t r0 = P.rec_off[r], r1 = P.rec_off[r + 1];
    if (r0 < 0 || r1 < r0 || r1 > P.nbytes) {  // no byte of such a record is read
      set_err(P.err, SPLIT_E_RECOFF);
      P.rec_b0[r] = 0;
      P.rec_end[r] = 0;
      P.rec_cnt[r] = 0;
      if (P.id_end) P.id_end[r] = 0;
      continue;
    }
    // a record that starts inside a sequence: it is invalid, and so is the one that holds the lead byte
    if (r0 < r1 && is_cont(s[r0])) {
      atomicMin(P.bad_rec, (unsigned long long)r);
      for (int j = 1; j <= 3 && r0 - j >= 0; ++j) {
        const uint32_t x = s[r0 - j];
        if (is_cont(x)) continue;
        if (lead_need(x) >= j) atomicMin(P.bad_rec, (unsigned long long)rec_of(P.rec_off, 0, r, r0 - j));
        break;
      }
    }
    int len = 0;
    int64_t i = r0;
    if (P.mode == 0)
      while (i < r1 && !space_at(s, i, r1, tab, len)) i += len;
    if (P.id_end) P.id_end[r] = i;
    const int64_t b0 = P.mode == 0 && i < r1 ? i + len : i;
    int64_t fs = b0;
    while (fs < r1 && space_at(s, fs, r1, tab, len)) fs += len;
    int64_t e = r1;
    while (e > fs) {
      const int64_t q = back(s, e, fs);
      if (!space_at(s, q, e, tab, len)) break;
      e = q;
    }
    P.rec_b0[r] = (int32_t)b0;
    P.rec_end[r] = (int32_t)e;
    P.rec_cnt[r] = fs < r1;
    if (fs < r1) {
      bytes += e - fs;
      if (P.fsmap) atomicOr(&P.fsmap[fs >> 6], 1ull << (fs & 63));
    }
  }
  bytes = wave_sum(bytes);
  if ((threadIdx.x & 63) == 0 && bytes) atomicAdd(P.bytes, (unsigned long long)bytes);
}

// MARK false: validation, sentence counts per record, sentence bytes, (fill) sentence starts per piece;
// MARK true: the sentences' starts and the ends that breaks give
template <bool MARK>
__global__ __launch_bounds__(256) void split_piece_kernel(SentSplitParams P) {
  if (*P.err) return;  // rec_off is refused: nothing is read through it
  const int lane = threadIdx.x & 63;
  const uint8_t* const s = P.buf;
  const int64_t nw = (int64_t)gridDim.x * 4, n_pieces = split_pieces(P.nbytes);
  for (int64_t piece = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); piece < n_pieces; piece += nw) {
    const int64_t s0 = piece * SPLIT_PIECE, s1 = min(s0 + SPLIT_PIECE, P.nbytes);
    const int64_t rlo = rec_of(P.rec_off, 0, P.n_rec, s0), rhi = rec_of(P.rec_off, rlo, P.n_rec, s1 - 1) + 1;
    int64_t dbytes = 0, acc_r = -1, run = MARK ? P.piece_base[piece] : 0;
    int32_t acc_n = 0;
    for (int64_t st = s0; st < s1; st += 64) {
      const int64_t p = st + lane;
      int64_t w = -1;  // where the sentence before p ends, when p starts one
      if (p < s1) {
        const uint32_t B = s[p];
        if (!MARK && B >= 0x80) {
          bool bad;
          if (is_cont(B)) {  // covered by a lead byte at most three bytes back
            bad = true;
            for (int j = 1; j <= 3 && p - j >= 0; ++j) {
              const uint32_t x = s[p - j];
              if (is_cont(x)) continue;
              bad = lead_need(x) < j;
              break;
            }
          } else {
            int len;
            bad = dec(s, p, P.nbytes, len) < 0;
          }
          if (bad) atomicMin(P.bad_rec, (unsigned long long)rec_of(P.rec_off, rlo, rhi, p));
        }
        if (p > 0) w = find_break(P, p, B, rlo, rhi);
      }
      const bool brk = w >= 0;
      const uint64_t m = __ballot(brk);
      if (!MARK) {
        if (brk) dbytes += w - p;
        // the breaks of this step, record by record (nearly always one record), onto the wave's running count
        const int64_t r = brk ? rec_of(P.rec_off, rlo, rhi, p) : -1;
        uint64_t rest = m;
        while (rest) {
          const int64_t rr = __shfl(r, __ffsll((unsigned long long)rest) - 1);
          const uint64_t g = __ballot(brk && r == rr);
          if (rr != acc_r) {
            if (acc_n && lane == 0) atomicAdd(&P.rec_cnt[acc_r], acc_n);
            acc_r = rr;
            acc_n = 0;
          }
          acc_n += __popcll(g);
          rest &= ~g;
        }
        if (P.fsmap) run += __popcll(m | P.fsmap[st >> 6]);
      } else {
        const uint64_t sm = m | P.fsmap[st >> 6];
        const int64_t k = run + bits_below(sm);
        if (((sm >> lane) & 1) && k >= 0 && k < P.n_sent) P.sent_start[k] = (int32_t)p;
        if (brk && k >= 1 && k <= P.n_sent) P.sent_end[k - 1] = (int32_t)w;
        run += __popcll(sm);
      }
    }
    if (!MARK) {
      if (acc_n && lane == 0) atomicAdd(&P.rec_cnt[acc_r], acc_n);
      if (P.piece_cnt && lane == 0) P.piece_cnt[piece] = (int32_t)run;
      dbytes = wave_sum(dbytes);
      if (lane == 0 && dbytes) atomicAdd(P.bytes, (unsigned long long)dbytes);
    }
  }
}

__global__ __launch_bounds__(256) void split_compare_kernel(SentSplitParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= P.n_rec; i += stride)
    if (P.user_doc_sent_off[i] != P.doc_sent_off[i]) set_err(P.err, SPLIT_E_DOCOFF);
}

__global__ __launch_bounds__(256) void split_tail_kernel(SentSplitParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < P.n_rec; r += stride) {
    const int64_t a = P.doc_sent_off[r], b = P.doc_sent_off[r + 1];
    if (b > a && b >= 1 && b <= P.n_sent) P.sent_end[b - 1] = P.rec_end[r];
  }
}

__global__ __launch_bounds__(256) void split_lens_kernel(SentSplitParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < P.n_sent; k += stride) {
    const int32_t n = P.sent_end[k] - P.sent_start[k];
    P.sent_end[k] = n > 0 ? n : 0;
  }
}

// A wave per sentence, a byte per lane and step.  The span is compared with the input and the output's capacity
// before the first byte moves, by comparisons that add to no unchecked offset.
__global__ __launch_bounds__(256) void split_copy_kernel(SentSplitParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < P.n_sent; k += nw) {
    const int64_t a = P.sent_start[k], n = P.sent_end[k], o = P.sent_off[k];
    if (a < 0 || n < 0 || a > P.nbytes || n > P.nbytes - a || o < 0 || o > P.out_bytes || n > P.out_bytes - o) continue;
    for (int64_t i = lane; i < n; i += 64) P.out[o + i] = P.buf[a + i];
  }
}

static unsigned wave_grid(int64_t waves, int n_cu) {
  const int64_t cap = (int64_t)n_cu * 32;  // 32 blocks (128 waves) per CU, grid-stride beyond
  int64_t b = (waves + 3) / 4;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

static unsigned lane_grid(int64_t lanes, int n_cu) {
  const int64_t cap = (int64_t)n_cu * 16;
  int64_t b = (lanes + 255) / 256;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

hipError_t launch_split_head(const SentSplitParams& P, int n_cu, hipStream_t s) {
  hipLaunchKernelGGL(split_head_kernel, dim3(lane_grid(P.n_rec, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_count(const SentSplitParams& P, int n_cu, hipStream_t s) {
  if (P.nbytes == 0) return hipSuccess;
  hipLaunchKernelGGL(split_piece_kernel<false>, dim3(wave_grid(split_pieces(P.nbytes), n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_compare(const SentSplitParams& P, int n_cu, hipStream_t s) {
  hipLaunchKernelGGL(split_compare_kernel, dim3(lane_grid(P.n_rec + 1, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_mark(const SentSplitParams& P, int n_cu, hipStream_t s) {
  if (P.nbytes == 0) return hipSuccess;
  hipLaunchKernelGGL(split_piece_kernel<true>, dim3(wave_grid(split_pieces(P.nbytes), n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_tail(const SentSplitParams& P, int n_cu, hipStream_t s) {
  if (P.n_rec == 0) return hipSuccess;
  hipLaunchKernelGGL(split_tail_kernel, dim3(lane_grid(P.n_rec, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_lens(const SentSplitParams& P, int n_cu, hipStream_t s) {
  if (P.n_sent == 0) return hipSuccess;
  hipLaunchKernelGGL(split_lens_kernel, dim3(lane_grid(P.n_sent, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_split_copy(const SentSplitParams& P, int n_cu, hipStream_t s) {
  if (P.n_sent == 0) return hipSuccess;
  hipLaunchKernelGGL(split_copy_kernel, dim3(wave_grid(P.n_sent, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

}  // namespace lddl
