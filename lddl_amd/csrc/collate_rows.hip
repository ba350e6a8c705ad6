// Training-time collate straight from a pack result: the rows are spans of
// the tokenizer's dense ids (lddl_row_spans), picked through a row-index list,
// so a batch goes from the packer's HBM buffers to the model's int64 inputs
// without the parquet detour (render strings, encode, decode, split, vocab
// lookup -- collate.hip's route).
//
// Reference: lddl/torch/bert.py:69-153 `_to_encoded_inputs` and :156-196
// `_mask_tokens`, as in collate.hip; the token ids are the ones the strings
// would be looked up to.  Batch row r is pack row g = rows[r] (rows NULL:
// row0 + r); a = len0[g], b = len1[g], n = a + b + 3:
//   input_ids[r]      = [CLS] ids[src0[g] .. +a) [SEP] ids[src1[g] .. +b) [SEP], 0 padded
//   token_type_ids[r] = 1 on [a + 2, n);  attention_mask[r] = 1 on [0, n)
//   next_sentence_labels[r] = flags[g] & 1
//   labels[r] by mode, as row_column (collate_row.h) has it.
// The same kernels with CODE set collate CodeBERT rows (lddl_collate_code_rows;
// pretrain_codebert.py:425-433, for which the reference has no loader): s =
// flags bit 1 says whether the first [SEP] is there, n = a + b + 2 + s, a row
// without it is one sequence (token_type_ids 0); modes 0 and 2 only, and no
// next_sentence_labels.
// The row layout, the row opener with its checks and the labelling are
// collate_row.h's, shared with collate_unpadded.hip; this file adds what
// padding needs: id 0, the attention mask and `special` on the pad columns.
//
// Work mapping: one wave per batch row, four rows per block.  A column's id is
// one 2-B load at an address known from (src, len) alone, so modes 0 and 2 need
// no staging: consecutive lanes read consecutive ids (128 B per wave
// instruction, 2 B in against 40 B out).  Loads stay 2 B wide on purpose: src0
// / src1 are arbitrary u16 offsets, a wider load would need an alignment
// prologue for a stream that is 5 % of the traffic, and a 2-B load never
// reaches past the span.  The bound is the four int64 output streams: a lane
// owns two adjacent columns and stores 16 B to each (1 KiB per wave
// instruction); an odd seq_len (alignment 1) leaves odd rows 8-B aligned only
// and takes the lane = column path with 8-B stores, as do outputs whose base
// is not 16-B aligned.  Mode 1 scatters the row's
// masked positions into a per-wave LDS row first (label | token << 16).
//
// No input faults: the row index is range-checked before anything is loaded
// through it, a row longer than seq_len, a static position >= seq_len and a
// CodeBERT row without docstring given to the BERT instantiation (flags bit 1
// clear: no [SEP] after segment 0, bert.py has no such loader) set the error
// word and leave the row unwritten; so does, with CODE, a row that has doc
// tokens and no [SEP] after them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collate.h"
#include "collate_dev.h"
#include "collate_row.h"
#include "wave.h"

namespace lddl {

// max over the batch of len0 + len1 + 2 + s: lane = row
template <bool CODE>
__global__ __launch_bounds__(256) void collate_rows_len_kernel(CollateRowsParams P) {
  const int64_t nt = (int64_t)gridDim.x * 256;
  uint32_t m = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < P.n_rows; r += nt) {
    const int64_t g = pack_row(P, r);
    if (g < 0) {
      set_err(P.err, CERR_ROW_INDEX, r);
      continue;
    }
    m = max(m, row_tokens<CODE>(P, g));
  }
  m = wave_incl_max(m);
  if ((threadIdx.x & 63) == 63 && m) atomicMax(P.max_len, (int32_t)m);
}

// SEL (mode 2 only) SEL_WORD: whole-word masking.  The select draw of a column
// is taken at the head of its word; the wave finds the heads of a step's
// columns from ballots of the word starts and carries the last one to the next
// step (word_heads), so the loops run for the whole wave and predicate the
// stores.  SEL_SPAN: span masking, the same loops with span_select's scan in
// place of word_heads.
template <int MODE, bool CODE, int SEL = SEL_TOKEN>
__global__ __launch_bounds__(256) void collate_rows_kernel(CollateRowsParams P) {
  static_assert(!(CODE && MODE == COLLATE_STATIC), "CodeBERT rows have no static masks");
  static_assert(SEL == SEL_TOKEN || MODE == COLLATE_DYNAMIC, "whole-word and span masking are dynamic masking");
  // mode 1 only: per wave, label | token << 16 of every masked column
  __shared__ uint32_t s_mlm[MODE == COLLATE_STATIC ? 4 : 1][MODE == COLLATE_STATIC ? COLLATE_MAX_LEN : 1];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  uint32_t* mlm = s_mlm[MODE == COLLATE_STATIC ? w : 0];
  const int32_t L = P.seq_len;
  const int64_t nw = (int64_t)gridDim.x * 4;
  // 16-B stores need every row of every output 16-B aligned
  const bool wide = (L & 1) == 0 && (((uintptr_t)P.input_ids | (uintptr_t)P.token_type_ids |
                                      (uintptr_t)P.attention_mask | (uintptr_t)P.labels) & 15) == 0;
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < P.n_rows; r += nw) {
    OpenRow R;
    uint32_t code = open_row<CODE>(P, r, L, R);
    if (MODE == COLLATE_STATIC && !code && !stage_static_masks(P, R.g, L, mlm)) code = CERR_POS_RANGE;
    if (code) {
      if (lane == 0) set_err(P.err, code, r);
      continue;
    }
    const int32_t n = R.L.n;
    int64_t* o_ids = P.input_ids + r * (int64_t)L;
    int64_t* o_tt = P.token_type_ids + r * (int64_t)L;
    int64_t* o_am = P.attention_mask + r * (int64_t)L;
    int64_t* o_lab = P.labels + r * (int64_t)L;
    if constexpr (SEL != SEL_TOKEN) {
      StepCarry carry;
      if (wide) {
        for (int32_t base = 0; base < L; base += 128) {
          const int32_t j = base + 2 * lane;  // L is even: j < L means j + 1 < L
          const WordColumn wc[2] = {word_column(P, R, j, j < L, j >= n), word_column(P, R, j + 1, j < L, j + 1 >= n)};
          int32_t pick[2];
          row_picks<SEL, 2>(P, r, base, wc, carry, pick);
          if (j < L) {
            const RowColumn c0 = row_column_picked<SEL>(P, R, r, j, wc[0], pick[0]);
            const RowColumn c1 = row_column_picked<SEL>(P, R, r, j + 1, wc[1], pick[1]);
            *reinterpret_cast<longlong2*>(o_ids + j) = make_longlong2(c0.id, c1.id);
            *reinterpret_cast<longlong2*>(o_tt + j) = make_longlong2(c0.tt, c1.tt);
            *reinterpret_cast<longlong2*>(o_am + j) = make_longlong2(j < n ? 1 : 0, j + 1 < n ? 1 : 0);
            *reinterpret_cast<longlong2*>(o_lab + j) = make_longlong2(c0.lab, c1.lab);
          }
        }
      } else {
        for (int32_t base = 0; base < L; base += 64) {
          const int32_t j = base + lane;
          const WordColumn wc[1] = {word_column(P, R, j, j < L, j >= n)};
          int32_t pick[1];
          row_picks<SEL, 1>(P, r, base, wc, carry, pick);
          if (j < L) {
            const RowColumn c = row_column_picked<SEL>(P, R, r, j, wc[0], pick[0]);
            o_ids[j] = c.id;
            o_tt[j] = c.tt;
            o_am[j] = j < n ? 1 : 0;
            o_lab[j] = c.lab;
          }
        }
      }
    } else if (wide) {
      // two columns and one 16-B store per lane and output
      for (int32_t j = 2 * lane; j < L; j += 128) {
        const RowColumn c0 = row_column<MODE>(P, R, mlm, r, j, j >= n);
        const RowColumn c1 = row_column<MODE>(P, R, mlm, r, j + 1, j + 1 >= n);
        *reinterpret_cast<longlong2*>(o_ids + j) = make_longlong2(c0.id, c1.id);
        *reinterpret_cast<longlong2*>(o_tt + j) = make_longlong2(c0.tt, c1.tt);
        *reinterpret_cast<longlong2*>(o_am + j) = make_longlong2(j < n ? 1 : 0, j + 1 < n ? 1 : 0);
        *reinterpret_cast<longlong2*>(o_lab + j) = make_longlong2(c0.lab, c1.lab);
      }
    } else {
      for (int32_t j = lane; j < L; j += 64) {
        const RowColumn c = row_column<MODE>(P, R, mlm, r, j, j >= n);
        o_ids[j] = c.id;
        o_tt[j] = c.tt;
        o_am[j] = j < n ? 1 : 0;
        o_lab[j] = c.lab;
      }
    }
    if (!CODE && lane == 0) P.next_sentence_labels[r] = R.flags & 1u;
  }
}

hipError_t launch_collate_rows_len(const CollateRowsParams& P, bool code, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  int64_t g = (P.n_rows + 255) / 256;
  if (g > (int64_t)n_cu * 8) g = (int64_t)n_cu * 8;
  if (code) hipLaunchKernelGGL(collate_rows_len_kernel<true>, dim3((int)g), dim3(256), 0, s, P);
  else hipLaunchKernelGGL(collate_rows_len_kernel<false>, dim3((int)g), dim3(256), 0, s, P);
  return hipGetLastError();
}

hipError_t launch_collate_rows(const CollateRowsParams& P, bool code, int32_t mode, int n_cu, hipStream_t s) {
  if (P.n_rows <= 0) return hipSuccess;
  const dim3 grid(grid_rows(P.n_rows, n_cu)), block(256);
  const int sel = mode == COLLATE_DYNAMIC ? collate_sel(P.cont, P.span) : SEL_TOKEN;
  if (sel == SEL_SPAN) {
    if (code) hipLaunchKernelGGL((collate_rows_kernel<COLLATE_DYNAMIC, true, SEL_SPAN>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_rows_kernel<COLLATE_DYNAMIC, false, SEL_SPAN>), grid, block, 0, s, P);
  } else if (sel == SEL_WORD) {
    if (code) hipLaunchKernelGGL((collate_rows_kernel<COLLATE_DYNAMIC, true, SEL_WORD>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((collate_rows_kernel<COLLATE_DYNAMIC, false, SEL_WORD>), grid, block, 0, s, P);
  } else if (code) {
    dispatch_code_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_rows_kernel<decltype(m)::value, true>), grid, block, 0, s, P);
    });
  } else {
    dispatch_mode(mode, [&](auto m) {
      hipLaunchKernelGGL((collate_rows_kernel<decltype(m)::value, false>), grid, block, 0, s, P);
    });
  }
  return hipGetLastError();
}

}  // namespace lddl
