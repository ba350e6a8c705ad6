// What the readers of a pack result share about a row, written once: the bin
// of a length (the packers' binning loops too), the partition of a row, the
// row's binned position and record, the row descriptor the copies work from,
// the per-row outputs and the masking reference.  Used by pack.hip
// (materialize, materialize2, row spans, the two masked-LM kernels),
// pack_wave.hip (bin_of) and render.hip (row_docs_kernel).  Every function is
// one level of the dependent-load chain partition -> bases -> binned index ->
// record -> segment starts.  The wave packers resolve that chain once, while
// a partition's records are hot, into a SpanRec per binned position
// (span_rec): lddl_row_spans streams those.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pack.h"

namespace lddl {

// binning.py:63-93: bin = (num_tokens - 1) // bin_size, clamped to the last bin
__device__ __forceinline__ int32_t bin_of(int32_t num_tokens, int32_t bin_size, int32_t nbins) {
  const int32_t b = (num_tokens - 1) / bin_size;
  return b > nbins - 1 ? nbins - 1 : b;
}

// ------------------------------------------------- the partition of a row --
// the last p with pair_base[p] <= g (an empty partition shares its base with
// the next one: the last of equals holds the row) by binary search, uniform
// when g is (materialize2: a wave's first row)
__device__ __forceinline__ int64_t part_of_row(const PackView& V, int64_t g) {
  int64_t plo = 0, phi = V.n_part - 1;
  while (plo < phi) {
    const int64_t mid = (plo + phi + 1) >> 1;
    if (V.pair_base[mid] <= g) plo = mid;
    else phi = mid - 1;
  }
  return plo;
}

// the same from a partition p at or before the row's (that of an earlier row
// of the wave): partitions of < 64 pairs, and empty ones, are walked over
__device__ __forceinline__ int64_t part_walk(const PackView& V, int64_t p, int64_t g) {
  while (V.pair_base[p + 1] <= g) ++p;
  return p;
}

// ------------------------------------------------ the record behind a row --
// first slot of partition p's pair arrays (pairs, binned, tok_local, mref, mloc)
__device__ __forceinline__ int64_t part_first_pair(const PackView& V, int64_t p) {
  return (int64_t)V.dup * V.doc_sent_off[V.part_doc_off[p]];
}

struct RowRef {
  int64_t i, pb;  // row g is binned position pb + i of its partition
  int64_t rec;    // its record: pairs[rec], mref[rec]
};

// index of the record at binned position pb + i
__device__ __forceinline__ int64_t row_rec(const PackView& V, int64_t pb, int64_t i) { return pb + V.binned[pb + i]; }

__device__ __forceinline__ RowRef row_ref(const PackView& V, int64_t p, int64_t g) {
  RowRef w;
  w.i = g - V.pair_base[p];
  w.pb = part_first_pair(V, p);
  w.rec = row_rec(V, w.pb, w.i);
  return w;
}

__device__ __forceinline__ RowRef pair_of_row(const PackView& V, int64_t p, int64_t g, PairRec& r) {
  const RowRef w = row_ref(V, p, g);
  r = V.pairs[w.rec];
  return w;
}

// first output token of the row
__device__ __forceinline__ int64_t row_tok_off(const PackView& V, int64_t p, const RowRef& w) {
  return V.tok_base[p] + V.tok_local[w.pb + w.i];
}

// ------------------------------------------------------ the row descriptor --
// Row = [CLS] A [SEP] (B [SEP]); a segment is n consecutive filtered sentences
// cut to [lo, hi): in the dense id array (sentences' ids back to back) that is
// ONE run starting at fs_dense[fs] + lo.
struct RowDesc {
  int64_t src0, src1;       // source start of segment A / B (0 when empty)
  int32_t l0, b1, l1, nt;   // |A|, first position of B, |B|, row length
};

// the two runs of record r, d0 / d1 = fs_dense[r.fs0] / fs_dense[r.fs1]: the
// one place a record's windows become offsets into the dense ids
__device__ __forceinline__ SpanRec span_rec(const PairRec& r, int64_t d0, int64_t d1) {
  SpanRec x;
  x.len0 = (uint16_t)(r.hi0 - r.lo0);
  x.len1 = (uint16_t)(r.hi1 - r.lo1);
  x.src0 = x.len0 > 0 ? d0 + r.lo0 : 0;
  x.src1 = x.len1 > 0 ? d1 + r.lo1 : 0;
  x.flags = r.flags;
  x.num_tokens = r.num_tokens;
  return x;
}

__device__ __forceinline__ RowDesc row_desc(const SpanRec& t) {
  RowDesc x;
  x.l0 = t.len0;
  x.l1 = t.len1;
  x.src0 = t.src0;
  x.src1 = t.src1;
  x.b1 = 1 + x.l0 + ((t.flags & 2) != 0);  // (bit 1: a [SEP] follows segment 0)
  x.nt = t.num_tokens;
  return x;
}

__device__ __forceinline__ RowDesc row_desc(const PackView& V, const PairRec& r) {
  return row_desc(span_rec(r, V.fs_dense[r.fs0], V.fs_dense[r.fs1]));
}

// the per-row outputs of materialize / row spans; out_tok_off is optional
// (lddl_row_spans): tok_off() is asked for the row's offset only when it is
// wanted, and the last row writes the total behind it
template <class TokOff>
__device__ __forceinline__ void store_row_meta(const MatParams& M, int64_t g, int64_t p, uint32_t flags,
                                               const RowDesc& x, int64_t total, TokOff tok_off) {
  if (M.out_tok_off) {
    const int64_t off = tok_off();
    M.out_tok_off[g] = off;
    if (g == total - 1) M.out_tok_off[total] = off + x.nt;
  }
  M.out_len0[g] = (uint16_t)x.l0;
  M.out_len1[g] = (uint16_t)x.l1;
  M.out_flags[g] = (uint8_t)flags;
  M.out_bin[g] = (uint8_t)bin_of(x.nt, M.V.bin_size, M.V.nbins);
  M.out_part[g] = p;
}

// --------------------------------------------- the masking reference of a row --
struct MaskRef {
  int nm;        // masked entries of the row
  int64_t aoff;  // marena[aoff .. aoff + nm): position | new id << 16, by position
  int64_t ooff;  // its first entry in the global position / label lists
};

__device__ __forceinline__ MaskRef mask_ref(const MlmParams& M, int64_t p, const RowRef& w) {
  const int64_t ref = M.mref[w.rec];
  MaskRef m;
  m.nm = (int)((uint64_t)ref >> 48);
  m.aoff = ref & ((int64_t(1) << 48) - 1);
  m.ooff = M.mask_base[p] + M.mloc[w.pb + w.i];
  return m;
}

// out_off[g], and behind the last row the total
__device__ __forceinline__ void store_mask_off(const MlmParams& M, int64_t g, int64_t total, const MaskRef& m) {
  M.out_off[g] = m.ooff;
  if (g == total - 1) M.out_off[total] = m.ooff + m.nm;
}

}  // namespace lddl
