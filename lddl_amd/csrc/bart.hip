// BART sentence aggregation (device side of lddl_bart_count / _plan_len / _plan / _render).
//
// The reference cuts every document into chunks of whole sentences
// (lddl/dask/bart/pretrain.py:88-128 `_aggregate_sentences`): walking the
// sentences in order it appends " " + sentence to the chunk and adds
// len(sentence.split()) to a running count; when the count reaches
// T = target_seq_length - 3 the chunk is emitted and both reset; what is left
// after the last sentence is emitted only when its count is > 0.  Only the
// chunk text is saved (:136-152), as one Arrow string column.
//
// Three kernels over a sentence-split corpus resident in HBM:
//   count   nwords[s] = len(sentence.split()): a wave per sentence over
//           scan_tokens (collate_dev.h), 64 bytes per step;
//   plan    the threshold-reset walk, a lane per document, in two passes
//           (chunks per document -> exclusive scan -> the per-chunk arrays);
//   render  a wave per chunk: a chunk's source is one contiguous run of
//           `data`, its text that run with a space in front of every sentence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bart.h"
#include "collate_dev.h"
#include "wave.h"

namespace lddl {

__global__ __launch_bounds__(256) void bart_count_kernel(BartCountParams P) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < P.n_sent; s += nw) {
    const int64_t a = P.sent_off[s], b = P.sent_off[s + 1];
    int32_t n = 0;
    if (a < 0 || b < a || b > P.nbytes) {  // no byte of such a sentence is read
      if (lane == 0) set_err(P.err, BART_E_SENT, 0);
    } else {
      n = scan_tokens(P.data, a, b, [](int32_t, int64_t) {});
    }
    if (lane == 0) P.nwords[s] = n;
  }
}

// The walk over document d's sentences [s0, s1): emit(first sentence, sentences, num_tokens, bytes) per chunk
// in order; returns false on a sentence that runs backwards or a chunk of 2^31 bytes (the walk stops there).
template <class F>
__device__ __forceinline__ bool bart_walk(const BartPlanParams& P, int64_t s0, int64_t s1, F emit) {
  int64_t cnt = 0, bytes = 0, first = s0;
  int64_t prev = P.sent_off[s0];
  if (prev < 0) {  // (with 0 <= prev <= next below, next - prev cannot wrap)
    set_err(P.err, BART_E_SENT, 0);
    return false;
  }
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t next = P.sent_off[s + 1];
    if (next < prev || next - prev >= 0x7FFFFFFFll - bytes) {
      set_err(P.err, next < prev ? BART_E_SENT : BART_E_BYTES, 0);
      return false;
    }
    bytes += 1 + (next - prev);
    prev = next;
    cnt += P.nwords[s];
    if (cnt >= P.target) {
      emit(first, s - first + 1, cnt, bytes);
      first = s + 1;
      cnt = 0;
      bytes = 0;
    }
  }
  if (cnt > 0) emit(first, s1 - first, cnt, bytes);  // (a remainder of 0-word sentences is dropped with its text)
  return true;
}

// document d's sentence range, checked: false (nothing is read through it) when it leaves [0, n_sent]
__device__ __forceinline__ bool bart_doc(const BartPlanParams& P, int64_t d, int64_t& s0, int64_t& s1) {
  s0 = P.doc_sent_off[d];
  s1 = P.doc_sent_off[d + 1];
  if (s0 >= 0 && s0 <= s1 && s1 <= P.n_sent && s1 - s0 < 0x7FFFFFFFll) return true;
  set_err(P.err, BART_E_DOC, 0);
  return false;
}

__global__ __launch_bounds__(256) void bart_plan_len_kernel(BartPlanParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long bytes = 0;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < P.n_doc; d += stride) {
    int64_t s0, s1;
    int32_t k = 0;
    if (bart_doc(P, d, s0, s1) && s0 < s1)
      bart_walk(P, s0, s1, [&](int64_t, int64_t, int64_t, int64_t b) {
        ++k;
        bytes += (unsigned long long)b;
      });
    P.doc_nchunks[d] = k;
  }
  for (int o = 32; o > 0; o >>= 1) bytes += __shfl_xor(bytes, o);
  if ((threadIdx.x & 63) == 0 && bytes) atomicAdd(P.total_bytes, bytes);
}

__global__ __launch_bounds__(256) void bart_plan_fill_kernel(BartPlanParams P) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < P.n_doc; d += stride) {
    int64_t s0, s1;
    const int64_t c = P.doc_chunk_off[d], c1 = P.doc_chunk_off[d + 1];
    // doc_chunk_off is checked, not trusted (no store through a refused entry); entries that start at 0, run
    // forward, end at n_chunks (the host compares the last) and each span what its walk gives cover every chunk
    if (c < 0 || c1 < c || c1 > P.n_chunks || (d == 0 && c != 0)) {
      set_err(P.err, BART_E_PLAN, 0);
      continue;
    }
    int64_t k = 0;
    const int64_t room = c1 - c;
    if (bart_doc(P, d, s0, s1) && s0 < s1)
      bart_walk(P, s0, s1, [&](int64_t first, int64_t ns, int64_t cnt, int64_t b) {
        if (k < room) {
          P.chunk_sent0[c + k] = first;
          P.chunk_nsent[c + k] = (int32_t)ns;
          P.chunk_num_tokens[c + k] = (int32_t)cnt;
          P.chunk_len[c + k] = (int32_t)b;
        }
        ++k;
      });
    if (k != room) set_err(P.err, BART_E_PLAN, 0);
  }
}

// out_off[i] = chunk_off[c0 + i] - chunk_off[c0], 0 <= i <= n
__global__ __launch_bounds__(256) void bart_rebase_kernel(BartRenderParams R) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint64_t base = (uint64_t)R.chunk_off[R.c0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= R.n; i += stride)
    R.out_off[i] = (int64_t)((uint64_t)R.chunk_off[R.c0 + i] - base);
}

// A wave per chunk.  Nothing of the chunk arrays is trusted: before its first store the wave checks that the
// chunk's sentences lie in [0, n_sent), that their offsets run forward inside [0, nbytes], that bytes + spaces
// equal the chunk's length and that its span lies in [0, out_cap) -- by comparisons that never add to a value
// not yet bounded.  A refused chunk is left unwritten, its number kept (the lowest wins).
__global__ __launch_bounds__(256) void bart_render_kernel(BartRenderParams R) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const int64_t base = R.chunk_off[R.c0];
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < R.n; i += nw) {
    const int64_t c = R.c0 + i;
    const int64_t s0 = R.chunk_sent0[c], ns = R.chunk_nsent[c];
    const int64_t ob = R.chunk_off[c], oe = R.chunk_off[c + 1];
    bool ok = s0 >= 0 && ns >= 0 && s0 <= R.n_sent && ns <= R.n_sent - s0 && base >= 0 && ob >= base && oe >= ob;
    int64_t o = 0, a = 0;
    if (ok) {
      o = ob - base;  // (0 <= base <= ob <= oe: neither difference wraps)
      const int64_t len = oe - ob;
      a = R.sent_off[s0];
      const int64_t b = R.sent_off[s0 + ns];
      ok = o <= R.out_cap && len <= R.out_cap - o && a >= 0 && a <= b && b <= R.nbytes && len >= ns &&
           len - ns == b - a;
      if (ok) {
        bool bad = false;
        for (int64_t j = lane; j < ns; j += 64) {
          const int64_t x = R.sent_off[s0 + j], y = R.sent_off[s0 + j + 1];
          bad |= x < a || y < x || y > b;
        }
        ok = !__any(bad);
      }
    }
    if (!ok) {
      if (lane == 0) atomicMin(R.bad, (unsigned long long)c);
      continue;
    }
    // sentence j of the chunk: ' ' at o + (x - a) + j, its bytes behind it; the last byte lands at
    // o + (b - a) + ns - 1 = o + len - 1
    uint8_t* const dst = R.out + o;
    for (int64_t j = 0; j < ns; ++j) {
      const int64_t x = R.sent_off[s0 + j], n = R.sent_off[s0 + j + 1] - x;
      uint8_t* const q = dst + (x - a) + j;
      if (lane == 0) q[0] = ' ';
      for (int64_t k = lane; k < n; k += 64) q[1 + k] = R.data[x + k];
    }
  }
}

static unsigned wave_grid(int64_t waves, int n_cu) {
  const int64_t cap = (int64_t)n_cu * 32;  // 32 blocks (128 waves) per CU, grid-stride beyond
  int64_t b = (waves + 3) / 4;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

static unsigned lane_grid(int64_t lanes, int n_cu) {
  const int64_t cap = (int64_t)n_cu * 4;  // 16 waves per CU walk documents, grid-stride beyond
  int64_t b = (lanes + 255) / 256;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

hipError_t launch_bart_count(const BartCountParams& P, int n_cu, hipStream_t s) {
  if (P.n_sent == 0) return hipSuccess;
  hipLaunchKernelGGL(bart_count_kernel, dim3(wave_grid(P.n_sent, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_bart_plan_len(const BartPlanParams& P, int n_cu, hipStream_t s) {
  if (P.n_doc == 0) return hipSuccess;
  hipLaunchKernelGGL(bart_plan_len_kernel, dim3(lane_grid(P.n_doc, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_bart_plan_fill(const BartPlanParams& P, int n_cu, hipStream_t s) {
  if (P.n_doc == 0) return hipSuccess;
  hipLaunchKernelGGL(bart_plan_fill_kernel, dim3(lane_grid(P.n_doc, n_cu)), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_bart_rebase(const BartRenderParams& R, int n_cu, hipStream_t s) {
  hipLaunchKernelGGL(bart_rebase_kernel, dim3(lane_grid(R.n + 1, n_cu)), dim3(256), 0, s, R);
  return hipGetLastError();
}

hipError_t launch_bart_render(const BartRenderParams& R, int n_cu, hipStream_t s) {
  if (R.n == 0) return hipSuccess;
  hipLaunchKernelGGL(bart_render_kernel, dim3(wave_grid(R.n, n_cu)), dim3(256), 0, s, R);
  return hipGetLastError();
}

}  // namespace lddl
