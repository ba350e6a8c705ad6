/*
 * lddl_amd -- C-ABI of the MI355X (gfx950) preprocessing hot path.
 *
 * The reference (alvin-zyl/LDDL) is pure Python; its hot path sits behind
 * three seams, each replaced here by an entry point of liblddl_amd.so:
 *
 *   lddl_create / lddl_destroy
 *       replaces transformers.BertTokenizerFast(vocab_file)
 *       (lddl/dask/bert/pretrain.py:584-587, pretrain_codebert.py:617 --
 *       the latter substituted by WordPiece over codebert_52000/vocab.txt).
 *   lddl_tokenize
 *       replaces the per-sentence tokenizer.tokenize(s, max_length=512,
 *       truncation=True) of _get_documents._to_document
 *       (pretrain.py:79-80, :82-95) and _get_code_pairs (pretrain_codebert.py:
 *       123-124), batched over every sentence of a shard.
 *   lddl_pack_bert / lddl_pack_codebert / lddl_materialize / lddl_masked_lm
 *       replace _get_pairs._to_partition_pairs (pretrain.py:386-402 with
 *       create_pairs_from_document :241-365 and, with --masking,
 *       create_masked_lm_predictions :182-238; pretrain_codebert.py:460-477
 *       with :343-442) and the binned writer's grouping
 *       (binning.py:63-93 _to_dataframe_binned).  A pack call writes its
 *       result into a caller-owned lddl_pack (lddl_pack_new; NULL = the
 *       ctx's own) that the post-pack calls then name explicitly.
 *   lddl_bin
 *       replaces _to_dataframe_binned's grouping (binning.py:63-93) on its
 *       own, for any column of row lengths.
 *
 * Conventions: every pointer named d_* is a DEVICE pointer on the ctx's
 * device; work is enqueued on `stream` (a hipStream_t, NULL = default) and is
 * asynchronous.  Inputs need only be ready in stream order on `stream`, and
 * outputs are ready in stream order on `stream`.  Return value 0 = ok, < 0 = LDDL_E* (message: lddl_last_error,
 * thread-local).  One call at a time per ctx (the ctx owns scratch).
 * Input text must be valid UTF-8 (Python str.encode output).
 */
#ifndef LDDL_AMD_H_
#define LDDL_AMD_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDDL_EINVAL -1
#define LDDL_EIO -2
#define LDDL_EFORMAT -3
#define LDDL_ENOMEM -4
#define LDDL_EHIP -5
#define LDDL_ECAPACITY -6
/* pretrain_codebert.py:421 _truncate_seq(code, max_num - len(doc)) with a
 * negative budget raises IndexError in the reference; reported as this code */
#define LDDL_EINDEX -7
/* pretrain.py:330-331 / pretrain_codebert.py:423 assert len(...) >= 1 */
#define LDDL_EASSERT -8

typedef struct lddl_ctx lddl_ctx;
/* The result of one lddl_pack_bert / lddl_pack_codebert call: pair records,
 * their shuffled and binned order, per-partition counts, the masking draws.
 * lddl_materialize / lddl_row_spans / lddl_masked_lm[_spans] / lddl_row_docs
 * read the result they are given, so several results can be live at once
 * (e.g. one shard set packed while the previous one is written).  Every call
 * taking a `pack` accepts NULL = the ctx's own result.  A pack result's
 * device buffers grow on demand and are reused by the next pack into it;
 * a failed pack leaves it empty (post-pack calls return LDDL_EINVAL). */
typedef struct lddl_pack lddl_pack;

const char *lddl_last_error(void);

/* vocab.txt: line i -> id i (reference: BertTokenizerFast(vocab_file)).
 * table_path: lddl_amd/data/unicode_table.bin. */
int lddl_create(const char *vocab_path, const char *table_path, int device, lddl_ctx **out);
void lddl_destroy(lddl_ctx *ctx);
int lddl_vocab_size(const lddl_ctx *ctx);
/* ids of [PAD] [UNK] [CLS] [SEP] [MASK] */
int lddl_special_ids(const lddl_ctx *ctx, int32_t out[5]);
/* NUL-terminated vocab entry `id` into buf; returns its length */
int lddl_vocab_token(const lddl_ctx *ctx, int32_t id, char *buf, int64_t cap);

/* Tokenise n_sent sentences (bytes [d_sent_off[s], d_sent_off[s+1])) into
 * the dense CSR layout: sentence s's ids are
 * d_out_ids[d_out_tok_off[s] .. d_out_tok_off[s+1]), d_out_ntok[s] = their
 * count = min(#tokens, max_tok), d_out_tok_off[n_sent] = the total
 * (d_out_tok_off: n_sent + 1 entries).  out_cap = entries of d_out_ids: ids
 * past it are not written, the offsets are still complete, so a caller that
 * finds d_out_tok_off[n_sent] > out_cap calls again with a larger buffer;
 * out_cap >= nbytes always suffices (#tokens <= #bytes).  nbytes must be >=
 * d_sent_off[n_sent] - d_sent_off[0]; 1 <= max_tok <= 65534.  d_bytes:
 * 4-byte aligned.  The scan reads from the 16-byte boundary at or below
 * d_bytes + d_sent_off[s], which for a d_bytes that is not 16-byte aligned
 * lies up to 12 bytes in front of d_bytes: a stated property, harmless
 * because an allocation starts 16-byte aligned, so such a d_bytes is always
 * interior to one.  d_sent_off[0] need not be 0; d_out_ids may be NULL when
 * out_cap is 0.  lddl_pack_* / lddl_materialize read d_out_ids with 16-B
 * loads: keep it 16-B aligned with 16 entries of padding past the total. */
int lddl_tokenize(lddl_ctx *ctx, const uint8_t *d_bytes, int64_t nbytes, const int64_t *d_sent_off,
                  int64_t n_sent, int32_t max_tok, uint16_t *d_out_ids, int64_t out_cap, int32_t *d_out_ntok,
                  int64_t *d_out_tok_off, void *stream);

/* Per-kernel timing of lddl_tokenize (diagnostics / bench): with timing on,
 * every call records HIP events around its kernels on the call's stream;
 * lddl_tokenize_stats (synchronises on them) returns out[0..5] = scan,
 * WordPiece and finish (serial-path tiles + counts + offset scan + dense
 * expand) milliseconds of the last call (summed over its segments), the
 * number of WordPiece records it ran, the number of segments (launches of
 * each kernel) and the number of tiles sent to the serial path. */
int lddl_set_timing(lddl_ctx *ctx, int on);
int lddl_tokenize_stats(lddl_ctx *ctx, double *out, int n);

/* With on != 0, every following lddl_tokenize also records which sentences
 * hold a [CLS] / [SEP] token (pretrain.py:187-190 excludes those tokens
 * from the masking candidates); a masked lddl_pack_bert over the same
 * d_out_ids / d_out_ntok buffers then reuses the flags instead of a pass
 * over the ids.  Off by default (the unmasked path does not need them). */
int lddl_set_special_flags(lddl_ctx *ctx, int on);

/* The tokenizer algorithm of the following lddl_tokenize calls (A/B and
 * tests; every algorithm gives identical ids): 5 = the split tokenizer (the
 * default), 0 = every tile through the exact serial path.  The split
 * tokenizer falls back to 0 for loaded tables it does not model.
 * *out_algo (may be NULL) receives the one selected.  Scratch is kept across
 * a switch; each call allocates what its algorithm reads. */
int lddl_set_tokenize_algo(lddl_ctx *ctx, int algo, int *out_algo);

/* A new, empty pack result on ctx's device (free with lddl_pack_free, before
 * or after the ctx).  lddl_pack_rows: #rows of its last successful pack, -1
 * when none. */
int lddl_pack_new(lddl_ctx *ctx, lddl_pack **out);
void lddl_pack_free(lddl_pack *pack);
int lddl_pack_rows(const lddl_pack *pack, int64_t *out_npairs);

/* Pack every partition of a tokenised shard set into `pack`.
 * Partition p = docs [d_part_doc_off[p], d_part_doc_off[p+1]); doc d =
 * sentences [d_doc_sent_off[d], d_doc_sent_off[d+1]); d_ids / d_ntok /
 * d_tok_off / d_sent_off are lddl_tokenize's output / input (d_ids may be
 * NULL unless masking; all of them must stay live until lddl_materialize;
 * every d_ntok count <= 65535, as any lddl_tokenize output with max_tok <=
 * 65535 -- the packers keep the counts as u16).  Partition p is packed exactly like the reference's
 * _to_partition_pairs (pretrain.py:386-402) after random.seed(seed + p):
 * duplicate_factor passes of create_pairs_from_document (:241-365), then
 * random.shuffle, then (bin_size > 0) the stable bin grouping of
 * binning.py:63-93.  Synchronises the stream once and returns
 * out_totals[4] = {#pairs, #tokens (with [CLS]/[SEP]), nbins, #masked}.
 * masking != 0: static MLM masking, create_masked_lm_predictions
 * (:182-238) with vocab_words = the vocab file's tokens in file order
 * (target_seq_length <= 1024); the rows are then written by
 * lddl_materialize and masked by lddl_masked_lm. */
int lddl_pack_bert(lddl_ctx *ctx, lddl_pack *pack, const uint16_t *d_ids, const int32_t *d_ntok, const int64_t *d_tok_off,
                   const int64_t *d_sent_off, int64_t n_sent, const int64_t *d_doc_sent_off, int64_t n_doc,
                   const int64_t *d_part_doc_off, int64_t n_part, int32_t target_seq_length, double short_seq_prob,
                   int32_t duplicate_factor, int32_t masking, double masked_lm_ratio, uint64_t seed, int32_t bin_size,
                   int64_t *out_totals,
                   void *stream);

/* CodeBERT docstring/code packing (pretrain_codebert.py:343-442, :460-477).
 * Doc d's first d_doc_nseg_doc[d] sentences are its docstring segments, the
 * rest its code segments (one per source line, pretrain_codebert.py:126-159). */
int lddl_pack_codebert(lddl_ctx *ctx, lddl_pack *pack, const int32_t *d_ntok, const int64_t *d_tok_off, const int64_t *d_sent_off,
                       int64_t n_sent, const int64_t *d_doc_sent_off, const int32_t *d_doc_nseg_doc, int64_t n_doc,
                       const int64_t *d_part_doc_off, int64_t n_part, int32_t target_seq_length,
                       double short_seq_prob, int32_t duplicate_factor, uint64_t seed, int32_t bin_size,
                       int64_t *out_totals, void *stream);

/* MLM-only packing: single-segment rows without NSP, [CLS] s_i .. s_j [SEP]
 * over consecutive sentences of one document (what RoBERTa-style recipes
 * train on).  The reference has no such mode; the draw order reuses its
 * seams: random.seed(seed + p) per partition; per kept document (>= 1
 * non-empty sentence; corpus order, duplicate_factor passes) the
 * short_seq_prob draw of create_pairs_from_document (pretrain.py:259-265:
 * target = target_seq_length - 2, or randint(2, that) when random() <
 * short_seq_prob); sentences accumulate until the chunk holds >= target tokens
 * or the document ends; a chunk longer than target_seq_length - 2 loses one
 * token per random() coin, front when < 0.5 else back (:161-179); then
 * random.shuffle of the partition's rows (:401) and the stable binning of
 * binning.py:63-93.  Arguments, checks and out_totals as lddl_pack_codebert
 * without d_doc_nseg_doc (out_totals[3] = 0); every d_ntok count <= 32768.
 * There is no error path.  A row is the CodeBERT packer's docstring-less
 * row: len0 = 0, flags = 0, the tokens in segment 1, so lddl_materialize
 * ([CLS] tokens [SEP]), lddl_row_spans, lddl_row_docs and the render calls
 * read it unchanged; lddl_masked_lm[_spans] refuse it (dynamic masking in the
 * collate calls covers these rows). */
int lddl_pack_mlm(lddl_ctx *ctx, lddl_pack *pack, const int32_t *d_ntok, const int64_t *d_tok_off, const int64_t *d_sent_off,
                  int64_t n_sent, const int64_t *d_doc_sent_off, int64_t n_doc, const int64_t *d_part_doc_off,
                  int64_t n_part, int32_t target_seq_length, double short_seq_prob, int32_t duplicate_factor,
                  uint64_t seed, int32_t bin_size, int64_t *out_totals, void *stream);

/* Sentence-order packing (SOP, ALBERT's binary head): both segments of a row
 * are consecutive sentences of ONE document, and is_random_next says whether
 * they were exchanged.  The reference has no such mode; the draw order reuses
 * its seams: random.seed(seed + p) per partition; per kept document (>= 2
 * non-empty sentences; a document with fewer gives no row and consumes no
 * draw; corpus order, duplicate_factor passes) the short_seq_prob draw of
 * create_pairs_from_document (pretrain.py:259-265: target =
 * target_seq_length - 3, or randint(2, that) when random() < short_seq_prob);
 * sentences accumulate into a chunk that is flushed at the document's last
 * sentence or once it holds >= target tokens and >= 2 sentences (no sentence
 * is put back; a flushed chunk of one sentence, a document's trailing one,
 * gives no row and no draw); per chunk of n sentences a_end = randint(1,
 * n - 1) (:285-286, drawn for n == 2 too), swap = random() < 0.5, A =
 * chunk[:a_end] and B = chunk[a_end:] exchanged when swap, then
 * _truncate_seq_pair(A, B, target_seq_length - 3) on the post-swap pair
 * (:161-176: the longer side, B on a tie, loses one token per random() coin,
 * front when < 0.5); then random.shuffle of the partition's rows (:401) and
 * the stable binning of binning.py:63-93.  Arguments, checks and out_totals
 * as lddl_pack_mlm (out_totals[3] = 0); every d_ntok count <= 32768.  There
 * is no error path.  A row is an lddl_pack_bert row ([CLS] A [SEP] B [SEP],
 * flags bit0 = swap, bit1 set), so lddl_materialize, lddl_row_spans,
 * lddl_row_docs and the render calls read it unchanged;
 * lddl_masked_lm[_spans] refuse it (dynamic masking in the collate calls
 * covers these rows). */
int lddl_pack_sop(lddl_ctx *ctx, lddl_pack *pack, const int32_t *d_ntok, const int64_t *d_tok_off, const int64_t *d_sent_off,
                  int64_t n_sent, const int64_t *d_doc_sent_off, int64_t n_doc, const int64_t *d_part_doc_off,
                  int64_t n_part, int32_t target_seq_length, double short_seq_prob, int32_t duplicate_factor,
                  uint64_t seed, int32_t bin_size, int64_t *out_totals, void *stream);

/* d_ids: the dense ids lddl_tokenize wrote (and the pack call read).
 * Write the rows of `pack` in output order (partition-major,
 * bin-major, shuffled order within a bin = the reference's part.{p}.parquet_{b}
 * row order).  Row g: d_out_tokens[d_out_tok_off[g] .. d_out_tok_off[g+1]) =
 * [CLS] A [SEP] B [SEP] (CodeBERT: [CLS] doc [SEP] code [SEP], or
 * [CLS] code [SEP] when the document has no docstring); len0/len1 = len(A),
 * len(B); flags bit0 = is_random_next, bit1 = segment 0 is followed by [SEP];
 * bin = bin id; part = partition.  d_bin_count (optional) receives
 * int64[n_part][nbins] row counts. */
int lddl_materialize(lddl_ctx *ctx, lddl_pack *pack, const uint16_t *d_ids, uint16_t *d_out_tokens, int64_t *d_out_tok_off,
                     uint16_t *d_out_len0, uint16_t *d_out_len1, uint8_t *d_out_flags, uint8_t *d_out_bin,
                     int64_t *d_out_part, int64_t *d_bin_count, void *stream);

/* The rows of `pack` as SPANS of the dense ids, in
 * lddl_materialize's row order, without copying a token: each segment of a
 * row is one contiguous run of lddl_tokenize's d_out_ids (a document's
 * sentences are contiguous there and a segment is a window of consecutive
 * sentences), so row g = [CLS] ids[src0[g], src0[g] + len0[g]) [SEP]
 * ids[src1[g], src1[g] + len1[g]) [SEP] (CodeBERT: the [SEP] after segment 0
 * only when flags bit1) -- the same rows as lddl_materialize (binning.py:63-93,
 * pretrain.py:348-353) for consumers that read the ids through the spans
 * (lddl_render_strings RENDER_SPAN: the parquet writer's string columns).
 * len0/len1/flags/bin/part/bin_count as lddl_materialize; d_out_tok_off
 * (optional, NULL = not written) = the materialised layout's row offsets.
 * The dense ids must stay live while the spans are read. */
int lddl_row_spans(lddl_ctx *ctx, lddl_pack *pack, int64_t *d_out_src0, int64_t *d_out_src1, int64_t *d_out_tok_off,
                   uint16_t *d_out_len0, uint16_t *d_out_len1, uint8_t *d_out_flags, uint8_t *d_out_bin,
                   int64_t *d_out_part, int64_t *d_bin_count, void *stream);

/* After lddl_pack_bert(masking=1) + lddl_materialize: apply the masking to
 * the materialised rows in place (A/B become output_tokens[1:1+len(A)] /
 * [2+len(A):...], pretrain.py:232-233) and write, per row g,
 * d_out_mlm_pos[d_out_mlm_off[g] .. d_out_mlm_off[g+1]) = masked_lm_positions
 * (ascending, row coordinates incl. [CLS]) and d_out_mlm_label[...] =
 * masked_lm_labels as token ids (pretrain.py:225-238, :340-361).  Reads
 * the rows and their partitions (d_out_tokens, d_out_tok_off, d_out_part)
 * of that lddl_materialize call, which must still be live. */
int lddl_masked_lm(lddl_ctx *ctx, lddl_pack *pack, int64_t *d_out_mlm_off, uint16_t *d_out_mlm_pos, uint16_t *d_out_mlm_label,
                   void *stream);

/* After lddl_pack_bert(masking=1) + lddl_row_spans (no rows materialised):
 * the static masking of the rows the spans describe.  Per row g,
 * d_out_mlm_off / _pos / _label exactly as lddl_masked_lm, and
 * d_out_mlm_token[k] = the token the masked row shows at position
 * d_out_mlm_pos[k] (the replacement id, or the label when the 10 % "keep"
 * branch left it, pretrain.py:212-225) -- what lddl_render_masked puts into
 * the A / B strings.  d_ids = the dense ids; d_src0 / d_src1 / d_len0 /
 * d_part = that lddl_row_spans call's outputs. */
int lddl_masked_lm_spans(lddl_ctx *ctx, lddl_pack *pack, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                         const uint16_t *d_len0, const int64_t *d_part, int64_t *d_out_mlm_off,
                         uint16_t *d_out_mlm_pos, uint16_t *d_out_mlm_label, uint16_t *d_out_mlm_token,
                         void *stream);

/* Render one string column of rows [row0, row0 + n_rows) as Arrow string
 * data: d_out_off[0..n_rows] (int64, d_out_off[0] = 0) and the UTF-8 bytes of
 * ' '.join(vocab[t] for t in segment) per row -- the reference's
 * 'A'/'B' (pretrain.py:348-353), 'masked_lm_labels' (:356-360),
 * 'doc'/'code' (pretrain_codebert.py:425-432) columns, which to_parquet
 * writes as pa.string() (pretrain.py:457-471).  segment: 0 = first segment
 * (A / doc: row tokens [1, 1 + len0)), 1 = second (B / code, after the [SEP];
 * codebert != 0: a [SEP] follows the doc segment only when flags bit1),
 * 2 = the whole row (d_row_off only; masked_lm labels from lddl_masked_lm),
 * 3 = a span (lddl_row_spans): row r = d_tokens[d_row_off[r], d_row_off[r] +
 * d_len0[r]) with d_tokens = the dense ids, d_row_off = src0 or src1, d_len0 =
 * len0 or len1 (d_row_off then has n rows, not n + 1 offsets).
 * Two-phase: *out_nbytes receives the byte count (the stream is synchronised
 * once); with d_out_bytes == NULL that is all (size query), else out_cap
 * must be >= it (LDDL_ECAPACITY) and the bytes are written asynchronously. */
int lddl_render_strings(lddl_ctx *ctx, const uint16_t *d_tokens, const int64_t *d_row_off, const uint16_t *d_len0,
                        const uint16_t *d_len1, const uint8_t *d_flags, int64_t row0, int64_t n_rows,
                        int32_t segment, int32_t codebert, int64_t *d_out_off, uint8_t *d_out_bytes,
                        int64_t out_cap, int64_t *out_nbytes, void *stream);

/* The masked rows' A (segment 0) or B (segment 1) strings from the spans:
 * lddl_render_strings' span rendering (d_src / d_len = src0 / len0 or src1 /
 * len1 of lddl_row_spans over d_ids) where a row position listed in
 * d_mlm_pos[d_mlm_off[r] .. d_mlm_off[r+1]) shows d_mlm_token instead
 * (lddl_masked_lm_spans; A's token k sits at row position 1 + k, B's at
 * len0 + 2 + k): the 'A' / 'B' of pretrain.py:232-233, 348-353 with --masking.
 * Same two-phase size query / capacity rules as lddl_render_strings. */
int lddl_render_masked(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src, const uint16_t *d_len,
                       const uint16_t *d_len0, int32_t segment, const int64_t *d_mlm_off, const uint16_t *d_mlm_pos,
                       const uint16_t *d_mlm_token, int64_t row0, int64_t n_rows, int64_t *d_out_off,
                       uint8_t *d_out_bytes, int64_t out_cap, int64_t *out_nbytes, void *stream);

/* The 'masked_lm_positions' column (pretrain.py:356-360: serialize_np_array
 * of the row's uint16 positions = np.save bytes, lddl/utils.py:98-102) of
 * rows [row0, row0 + n_rows) as Arrow binary data: row r's k =
 * d_mlm_off[r+1] - d_mlm_off[r] positions d_mlm_pos[d_mlm_off[r] ..] (from
 * lddl_masked_lm[_spans], absolute row numbering) become header k + the k
 * values little-endian, where d_hdr holds the np.save header of a uint16[k]
 * array for every k in [0, kmax], hdr_len bytes each (np.save pads every 1-D
 * header to the same length; even).  A row with more than kmax positions is
 * LDDL_EINVAL.  Same two-phase size query / capacity rules as
 * lddl_render_strings. */
int lddl_render_npy(lddl_ctx *ctx, const int64_t *d_mlm_off, const uint16_t *d_mlm_pos, int64_t row0,
                    int64_t n_rows, const uint16_t *d_hdr, int32_t hdr_len, int32_t kmax, int64_t *d_out_off,
                    uint8_t *d_out_bytes, int64_t out_cap, int64_t *out_nbytes, void *stream);

/* Document index (into the corpus' documents) of every row of `pack`, in lddl_materialize's row order: the row's own document (seg0's; a
 * CodeBERT row without docstring: its code's) -- feeds CodeBERT's 'id'
 * column = document._id (pretrain_codebert.py:425-426). */
int lddl_row_docs(lddl_ctx *ctx, lddl_pack *pack, int64_t *d_out_doc, void *stream);

/* Group n rows by length bin exactly as binning.py:63-93
 * _to_dataframe_binned: row i goes to bin (num_tokens[i] - 1) // bin_size
 * (Python floor division), capped at nbins - 1; a negative bin indexes the
 * bins from the end as the reference's seqs[bin_id] does (length 0 -> the
 * last bin), below -nbins is the reference's IndexError (LDDL_EINDEX).
 * d_out_perm[0..n) = the row indices bin-major, ascending within a bin (the
 * row order of the concatenated per-bin frames); d_out_bin_counts[0..nbins)
 * = rows per bin.  1 <= nbins <= 1024, bin_size >= 1.  Synchronises the
 * stream once (the IndexError check). */
int lddl_bin(lddl_ctx *ctx, const int64_t *d_num_tokens, int64_t n, int32_t bin_size, int32_t nbins,
             int64_t *d_out_perm, int64_t *d_out_bin_counts, void *stream);

/* ---- training-time collate -------------------------
 * Replaces lddl/torch/bert.py:69-153 `_to_encoded_inputs` (+ :156-196
 * `_mask_tokens`) for a batch of parquet rows.  Columns arrive as Arrow-style
 * string columns on the device: bytes + int64 offsets[n_rows + 1].
 *
 * lddl_collate_seq_len: the batch's padded length = max over rows of
 * len(A.split()) + len(B.split()) + 3, rounded up to seq_align
 * (bert.py:94-101).  Synchronises the stream (the length shapes the outputs). */
int lddl_collate_seq_len(lddl_ctx *ctx, const uint8_t *d_a, const int64_t *d_a_off, const uint8_t *d_b,
                         const int64_t *d_b_off, int64_t n_rows, int32_t seq_align, int64_t *out_seq_len,
                         void *stream);

/* Fill the [n_rows, seq_len] int64 outputs (bert.py:102-152): input_ids
 * ([CLS] A [SEP] B [SEP], tokens -> ids via the vocab, [UNK] for a miss, 0
 * padding), token_type_ids, attention_mask, next_sentence_labels[n_rows] and
 * d_labels by mode:
 *   0  special_tokens_mask (bert.py:117-122; dynamic masking left to
 *      lddl_mask_tokens);
 *   1  static masking labels: ignore_index except labels[positions] =
 *      ids(labels.split()), positions = the row's np.save uint16 bytes
 *      (d_pos / d_pos_off, d_lab / d_lab_off required);
 *   2  dynamic masking fused: mode 0 then lddl_mask_tokens with the same seed
 *      and counter (identical result).
 * Errors: LDDL_ECAPACITY (a row longer than seq_len, seq_len > 2048),
 * LDDL_EINDEX (a masked position >= seq_len: bert.py:113's IndexError),
 * LDDL_EFORMAT (positions not np.save bytes, or count != label count). */
int lddl_collate_bert(lddl_ctx *ctx, const uint8_t *d_a, const int64_t *d_a_off, const uint8_t *d_b,
                      const int64_t *d_b_off, const uint8_t *d_is_random_next, const uint8_t *d_pos,
                      const int64_t *d_pos_off, const uint8_t *d_lab, const int64_t *d_lab_off, int64_t n_rows,
                      int64_t seq_len, int32_t mode, int64_t ignore_index, double mlm_probability, uint64_t seed,
                      uint64_t counter, int64_t *d_input_ids, int64_t *d_token_type_ids,
                      int64_t *d_attention_mask, int64_t *d_labels, int64_t *d_next_sentence_labels,
                      void *stream);

/* Dynamic MLM masking in place (bert.py:156-196 `_mask_tokens`): a column
 * with special_tokens_mask == 0 is selected with probability
 * mlm_probability; selected -> [MASK] (p 0.8), else a uniform id in
 * [0, vocab size) (p 0.5), else kept; labels = the original id where
 * selected, ignore_index elsewhere.  Draws are a counter-based hash of
 * (seed, counter, row, column): the reference's distribution, not torch's
 * CPU generator stream.
 *
 * The draw, in uint64 arithmetic that wraps (tests/mask_model.py is this in
 * numpy; every entry point with a dynamic mode draws the same way):
 *   sm(x)   = splitmix64's output function: x += 0x9E3779B97F4A7C15;
 *             x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *             x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31
 *   unit(h) = (double)(h >> 11) * 2^-53, exact, in [0, 1)
 *   key   k = sm(seed ^ sm(counter))
 *   index i = ((row << 20) | column) * 3, row = the row of the batch (not of
 *             a row table), column < 2^20
 *   selected  iff special_tokens_mask == 0 and unit(sm(k + i)) < mlm_probability
 *   [MASK]    iff selected and unit(sm(k + i + 1)) < 0.8
 *   otherwise, with g = sm(k + i + 2): the id ((g & 0xFFFFFFFF) * vocab size) >> 32
 *             iff unit(g) < 0.5, else the input id unchanged.
 * Ids and labels pass through as 64-bit values. */
int lddl_mask_tokens(lddl_ctx *ctx, int64_t *d_inputs, const int64_t *d_special_tokens_mask, int64_t *d_labels,
                     int64_t n_rows, int64_t seq_len, double mlm_probability, int64_t ignore_index, uint64_t seed,
                     uint64_t counter, void *stream);

/* Whole-word dynamic masking (BERT-WWM): with on != 0, lddl_mask_tokens and
 * mode 2 of every collate call of the ctx (lddl_collate_bert,
 * lddl_collate_rows[_unpadded], lddl_collate_code_rows[_unpadded]) select
 * words instead of tokens.  Off by default; modes 0 and 1 ignore it; a
 * vocabulary without "##" entries is accepted (every token is then a word).
 * The reference has no counterpart.  For one row, with id_j the unmasked id
 * of column j, V the vocabulary size and special(j) what the call uses
 * without the switch ([CLS], each [SEP] and the padding in the collates, the
 * caller's special_tokens_mask in lddl_mask_tokens):
 *   cont(id)   iff 0 <= id < V and vocabulary entry id begins with the two
 *              bytes "##" (ids outside [0, V), which only lddl_mask_tokens can
 *              meet, are no continuations)
 *   start(j)   iff !special(j) and (j == 0 or special(j - 1) or !cont(id_j)):
 *              a segment's first token starts a word even when it is a "##"
 *              piece (_truncate_seq_pair can leave one there), and a word
 *              never crosses a [SEP]
 *   head(j)    for a non-special j: the largest h <= j with start(h)
 *   selected   iff !special(j) and unit(sm(k + i(row, head(j)))) <
 *              mlm_probability: lddl_mask_tokens' select draw taken at the
 *              word's head column, k and i as there
 *   a selected j has label id_j and its own second and third draws
 *   (i(row, j) + 1, + 2) decide [MASK] / random id / kept, unchanged; an
 *   unselected j keeps its id and has label ignore_index.
 * row and column are what they are without the switch (on the padding-free
 * calls the column is the token's position in its row).  A row in which every
 * token heads its own word is masked bit for bit as without the switch, and
 * a token is selected with probability mlm_probability either way.
 * tests/wwm_model.py is this in numpy. */
int lddl_set_whole_word_mask(lddl_ctx *ctx, int on);

/* Span dynamic masking (ALBERT's n-gram masking, SpanBERT's span masking, the
 * n-gram option of Megatron-style BERT pipelines): contiguous runs of whole
 * words are selected.  The reference has no counterpart.  Parameters:
 * max_span L in [1, 16], geo_p g in (0, 1] and the call's mlm_probability p.
 *
 * Length law (SpanBERT's clipped geometric, renormalised):
 *   P(len = l) = g (1 - g)^(l - 1) / (1 - (1 - g)^L)  for l = 1 .. L
 *   cdf[t] = P(len <= t) for t = 1 .. L, cdf[L] = 1 exactly
 *   S_0 = 1, S_t = 1 - cdf[t]
 * Start probability q, chosen so that an interior word (one with L - 1 words
 * of its segment in front of it) is covered with probability p:
 *   L == 1: q = p exactly; otherwise q is the root in [0, p] of
 *   1 - prod_{t = 0 .. L-1} (1 - q S_t) = p  (0 at q = 0, at least p at q = p,
 *   monotone), by 64 bisection steps in double on the host: the upper end of
 *   the last interval, which is 0 for p = 0 and 1 for p = 1.
 *
 * Per row, with special(j), cont(id), start(j), head(j), k, i(row, col), sm
 * and unit as in the whole-word definition above:
 *   a segment  is a maximal run of non-special columns; spans live inside one
 *              segment, so a span never covers or crosses a [SEP], [CLS], pad
 *              column or caller-marked special column
 *   w(j)       the number of start columns of j's segment at or before j
 *   ks         = sm(k ^ 0x5350414E4D41534B)
 *   open(h)    for a start column h: iff unit(sm(k + i(row, h))) < q, the
 *              select draw of lddl_mask_tokens taken at the head h
 *   len(h)     = 1 + #{t in [1, L - 1] : unit(sm(ks + i(row, h))) >= cdf[t]}
 *   selected   iff !special(j) and there is a start column h <= j in j's
 *              segment with open(h) and w(j) - w(h) < len(h)
 *   a selected j has label id_j and its own second and third draws
 *   (i(row, j) + 1, + 2) decide [MASK] / random id / kept, exactly as without
 *   the switch: replacement stays per token, as with whole words (SpanBERT
 *   replaces per span: all of a span's tokens alike); an unselected j keeps
 *   its id and has label ignore_index.
 * Consequences: with L = 1 the result is bit for bit whole-word masking.
 * Overlapping spans simply union.  The first L - 1 words of a segment are
 * covered slightly less often than p, because fewer heads lie in front of
 * them.  A span that would run past its segment's end is clipped there.
 * tests/span_model.py is this in numpy.
 *
 * lddl_span_params: q and cdf for (max_span, geo_p, mlm_probability), on the
 * host (no ctx, no GPU).  out_cdf[t - 1] = cdf[t] for t = 1 .. L, 1.0 behind
 * them.  The one place they are computed: every collate call of a ctx with
 * the switch on takes them from here at call time, from its own
 * mlm_probability.  LDDL_EINVAL: max_span outside [1, 16], geo_p outside
 * (0, 1], mlm_probability outside [0, 1], a NULL output. */
int lddl_span_params(int32_t max_span, double geo_p, double mlm_probability, double *out_q, double out_cdf[16]);

/* The switch: max_span == 0 turns span masking off (the default; geo_p is
 * then ignored).  While it is on, lddl_mask_tokens and mode 2 of every collate
 * call of the ctx (lddl_collate_bert, lddl_collate_rows[_unpadded | _fixed],
 * lddl_collate_code_rows[_unpadded | _fixed]) select as defined above, and
 * the whole-word switch is ignored; modes 0 and 1 ignore it; a vocabulary
 * without "##" entries is accepted (every token is then a word).
 * LDDL_EINVAL: max_span outside [0, 16] or geo_p outside (0, 1]; the switch
 * then stays as it was. */
int lddl_set_span_mask(lddl_ctx *ctx, int32_t max_span, double geo_p);

/* ---- collate straight from a pack result ---------------------------------
 * The same lddl/torch/bert.py:69-153 `_to_encoded_inputs` (+ :156-196
 * `_mask_tokens`) for rows that never became parquet: batch row r is row
 * g = d_rows[r] (d_rows NULL: g = row0 + r) of a pack result's spans
 * (lddl_row_spans over the dense ids), 0 <= g < n_total; any order, repeats
 * allowed.  For users who pack and train in one job; the token ids are the
 * ones lddl_collate_bert would look the rendered strings up to.
 *
 * lddl_collate_rows_seq_len: the batch's padded length = max over its rows of
 * len0[g] + len1[g] + 3, rounded up to seq_align (bert.py:94-101; d_len0 /
 * d_len1 = lddl_row_spans' outputs).  Synchronises the stream.  A row index
 * outside [0, n_total) is LDDL_EINDEX (checked before any load through it),
 * n_rows == 0 LDDL_EINVAL. */
int lddl_collate_rows_seq_len(lddl_ctx *ctx, const uint16_t *d_len0, const uint16_t *d_len1, const int64_t *d_rows,
                              int64_t row0, int64_t n_rows, int64_t n_total, int32_t seq_align,
                              int64_t *out_seq_len, void *stream);

/* Fill the [n_rows, seq_len] int64 outputs of lddl_collate_bert
 * (bert.py:102-152) from the spans: with a = len0[g], b = len1[g],
 * n = a + b + 3, input_ids[r] = [CLS] d_ids[src0[g] .. +a) [SEP]
 * d_ids[src1[g] .. +b) [SEP] padded with 0, token_type_ids 1 on [a + 2, n),
 * attention_mask 1 on [0, n), next_sentence_labels[r] = flags[g] & 1, and
 * d_labels by mode, numbered as in lddl_collate_bert:
 *   0  special_tokens_mask (columns 0, a + 1 and >= n - 1);
 *   1  static masking from lddl_masked_lm_spans' arrays (required; NULL in the
 *      other modes): for k in [mlm_off[g], mlm_off[g+1]) input_ids[r,
 *      mlm_pos[k]] = mlm_token[k], labels[r, mlm_pos[k]] = mlm_label[k],
 *      ignore_index elsewhere (bert.py:113-116);
 *   2  mode 0 then lddl_mask_tokens (bert.py:156-196) with row = r: bit for
 *      bit lddl_collate_bert mode 2 on the same rows, seed and counter.
 * d_ids .. d_flags: the dense ids (with their 16 entries of padding) and
 * lddl_row_spans' outputs, [n_total] each.  Synchronises the stream.
 * Errors, first one wins, none faults: LDDL_EINDEX (a row index outside
 * [0, n_total), checked before any load through it; a static position >=
 * seq_len), LDDL_ECAPACITY (a row longer than seq_len, seq_len > 2048),
 * LDDL_EINVAL (a row whose flags lack bit 1: a CodeBERT row without
 * docstring has no [SEP] after segment 0, and bert.py has no CodeBERT
 * loader; lddl_collate_code_rows takes such rows). */
int lddl_collate_rows(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                      const uint16_t *d_len0, const uint16_t *d_len1, const uint8_t *d_flags, const int64_t *d_rows,
                      int64_t row0, int64_t n_rows, int64_t n_total, const int64_t *d_mlm_off,
                      const uint16_t *d_mlm_pos, const uint16_t *d_mlm_label, const uint16_t *d_mlm_token,
                      int64_t seq_len, int32_t mode, int64_t ignore_index, double mlm_probability, uint64_t seed,
                      uint64_t counter, int64_t *d_input_ids, int64_t *d_token_type_ids, int64_t *d_attention_mask,
                      int64_t *d_labels, int64_t *d_next_sentence_labels, void *stream);

/* ---- padding-free collate straight from a pack result ---------------------
 * The same batch for a model with variable-length attention: the rows
 * concatenated into one token stream, batch row r at tokens [cu_seqlens[r],
 * cu_seqlens[r + 1]), no pad columns and no attention_mask.  Rows are picked
 * as in lddl_collate_rows: batch row r is row g = d_rows[r] (d_rows NULL:
 * g = row0 + r) of a pack result's spans, 0 <= g < n_total; any order,
 * repeats allowed; for users who pack and train in one job.  This output has
 * no counterpart in the reference (lddl/torch/bert.py:69-153 pads every
 * batch): it is defined as lddl_collate_rows at the same seed and counter
 * with every column j >= n_r = len0[g] + len1[g] + 3 of row r dropped, bit
 * for bit in all three modes (the dynamic draw is keyed by (seed, counter, r,
 * j), not by seq_len).
 *
 * lddl_collate_rows_cu_seqlens: d_cu_seqlens[0] = 0, d_cu_seqlens[r + 1] =
 * d_cu_seqlens[r] + n_r as int32 [n_rows + 1] on the device (what varlen
 * attention kernels take); *out_total = the batch's tokens T =
 * cu_seqlens[n_rows], *out_max_seqlen = max over its rows of n_r.
 * Synchronises the stream.  A row index outside [0, n_total) is LDDL_EINDEX
 * (checked before any load through it), n_rows == 0 LDDL_EINVAL, a batch of
 * 2^31 tokens or more LDDL_ECAPACITY (summed in 64 bits; d_cu_seqlens is then
 * left unwritten). */
int lddl_collate_rows_cu_seqlens(lddl_ctx *ctx, const uint16_t *d_len0, const uint16_t *d_len1,
                                 const int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                 int32_t *d_cu_seqlens, int64_t *out_total, int64_t *out_max_seqlen, void *stream);

/* Fill the int64 outputs: for t = cu_seqlens[r] + j, 0 <= j < n_r,
 * input_ids[t], token_type_ids[t] and d_labels[t] are column j of row r of
 * lddl_collate_rows (d_labels by mode 0 / 1 / 2 as there; the static arrays
 * required in mode 1, NULL otherwise), position_ids[t] = j, and
 * next_sentence_labels[r] = flags[g] & 1.  The four token outputs are
 * [total] (total = the T of lddl_collate_rows_cu_seqlens, or more),
 * next_sentence_labels [n_rows]; d_cu_seqlens is that call's output and is
 * checked, not trusted.  The caller's sequence_length_alignment has no
 * meaning here.  Synchronises the stream.
 * Errors, first one wins, none faults, the row is left unwritten and no row
 * stores outside its own tokens: LDDL_EINVAL (a row with cu_seqlens[r] < 0,
 * cu_seqlens[r + 1] - cu_seqlens[r] != n_r or cu_seqlens[r] + n_r > total; a
 * row whose flags lack bit 1, a CodeBERT row; mode not in 0..2), LDDL_EINDEX
 * (a row index outside [0, n_total), checked before any load through it; a
 * static position >= n_r -- stricter than lddl_collate_rows' >= seq_len,
 * since a position in [n_r, seq_len) would land in the next row here),
 * LDDL_ECAPACITY (a row longer than 2048 tokens, total >= 2^31). */
int lddl_collate_rows_unpadded(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                               const uint16_t *d_len0, const uint16_t *d_len1, const uint8_t *d_flags,
                               const int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                               const int64_t *d_mlm_off, const uint16_t *d_mlm_pos, const uint16_t *d_mlm_label,
                               const uint16_t *d_mlm_token, const int32_t *d_cu_seqlens, int64_t total, int32_t mode,
                               int64_t ignore_index, double mlm_probability, uint64_t seed, uint64_t counter,
                               int64_t *d_input_ids, int64_t *d_token_type_ids, int64_t *d_position_ids,
                               int64_t *d_labels, int64_t *d_next_sentence_labels, void *stream);

/* ---- fixed-shape padding-free collate --------------------------------------
 * The padding-free batch in outputs whose sizes do not depend on the batch,
 * offsets and fill in one call, one launch and one synchronise: for a trainer
 * that wants every tensor of a step at a fixed shape (one hipBLASLt problem
 * size, a step that is captured or compiled once).  No counterpart in the
 * reference (lddl/torch/bert.py:69-153 pads rows, never the stream).  Three
 * capacities: tok_cap = T tokens, seq_cap = N sequence slots, max_seqlen = S,
 * the longest sequence the attention call is told about.  The four token
 * outputs are [T], d_cu_seqlens is an output, int32 [N + 1], and
 * next_sentence_labels is [N].  With the n = n_rows rows picked as in
 * lddl_collate_rows_unpadded, n_r tokens each, total = sum of n_r:
 *
 * Real rows.  Outputs [0, total), cu_seqlens[0 .. n] and
 * next_sentence_labels[0 .. n) are those of lddl_collate_rows_cu_seqlens +
 * lddl_collate_rows_unpadded for the same rows, mode, ignore_index,
 * mlm_probability, seed, counter and whole-word switch, bit for bit.
 *
 * Slack.  [total, T) is cut into p = ceil((T - total) / S) pad sequences in
 * slots n .. n + p - 1, each of S tokens but possibly the last, so that no
 * token of the stream lies outside a sequence.  A pad token at offset j of its
 * pad sequence has input_ids 0, token_type_ids 0, position_ids j and labels
 * ignore_index (mode 0: special_tokens_mask 1, as on the pad columns of
 * lddl_collate_rows).  Slots n + p .. N - 1 are empty: cu_seqlens[r] = T for
 * n + p <= r <= N; cu_seqlens[N] is always T.  next_sentence_labels[r] =
 * ignore_index for r >= n.
 *
 * *out_total = total, *out_n_rows = n, *out_n_seqs = n + p; d_status, int32
 * [4] on the device, receives {total, n, n + p, S} for a trainer that reads
 * them without the host.  Synchronises the stream.
 *
 * Errors, a row's before the capacities' and among rows the first one wins,
 * none faults, and nothing is stored outside the capacities in any case:
 * LDDL_ECAPACITY (total > T, with total in
 * *out_total, and the rows that would pass T left unwritten; a row longer than
 * S, left unwritten; n + p > N; n > N; S not in [3, 2048]; T > INT32_MAX;
 * N not in [1, 2^20]), LDDL_EINDEX (a row index outside [0, n_total), checked
 * before any load through it; a static position >= n_r), LDDL_EINVAL
 * (n_rows <= 0, null pointers, mode not in 0..2, mlm_probability not in
 * [0, 1], a row whose flags lack bit 1: a CodeBERT row). */
int lddl_collate_rows_fixed(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                            const uint16_t *d_len0, const uint16_t *d_len1, const uint8_t *d_flags,
                            const int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                            const int64_t *d_mlm_off, const uint16_t *d_mlm_pos, const uint16_t *d_mlm_label,
                            const uint16_t *d_mlm_token, int32_t *d_cu_seqlens, int64_t tok_cap, int64_t seq_cap,
                            int64_t max_seqlen, int32_t mode, int64_t ignore_index, double mlm_probability,
                            uint64_t seed, uint64_t counter, int64_t *d_input_ids, int64_t *d_token_type_ids,
                            int64_t *d_position_ids, int64_t *d_labels, int64_t *d_next_sentence_labels,
                            int32_t *d_status, int64_t *out_total, int64_t *out_n_rows, int64_t *out_n_seqs,
                            void *stream);

/* ---- collate CodeBERT rows straight from a pack result ----------------------
 * The four calls above for the rows of lddl_pack_codebert (or of
 * lddl_code_rows_from_strings): the row pretrain_codebert.py:425-433 saves as
 * doc / code / num_tokens.  The reference has no loader for it
 * (lddl/torch/bert.py only knows A / B / is_random_next); the layout is what a
 * BERT tokenizer gives for a pair and for a single sequence.  Row g has
 * a = len0[g] doc tokens, b = len1[g] code tokens, s = (flags[g] >> 1) & 1
 * (1 when the document has docstring segments, pretrain_codebert.py:356) and
 * n = a + b + 2 + s columns:
 *   s = 1:  0 [CLS] | [1, a] doc | a + 1 [SEP] | [a + 2, n - 2] code | n - 1 [SEP]
 *   s = 0:  0 [CLS] | [1, n - 2] code | n - 1 [SEP]              (a must be 0)
 * a = 0 with s = 1 is a regular row, [CLS] [SEP] code [SEP].  token_type_ids
 * is 1 on [a + 2, n) when s = 1 and 0 on every column when s = 0;
 * attention_mask 1 on [0, n); the special_tokens_mask 1 on [CLS], each [SEP]
 * and the pad columns.  There is no next_sentence_labels (the rows carry no
 * NSP label) and no static mode (the CodeBERT preprocessor ignores masking):
 * mode 0 is the special_tokens_mask, mode 2 is mode 0 followed by
 * lddl_mask_tokens' draw keyed by (seed, counter, row of the batch, column),
 * with the vocabulary size of the ctx, bit for bit.  For s = 1 rows the
 * outputs are those of lddl_collate_rows on the same rows.  Rows are picked as
 * there: batch row r is row g = d_rows[r] (d_rows NULL: g = row0 + r),
 * 0 <= g < n_total, any order, repeats allowed.  All four synchronise the
 * stream, and an empty batch (n_rows <= 0) is LDDL_EINVAL in each.
 *
 * lddl_collate_code_rows_seq_len: the batch's padded length = max over its
 * rows of a + b + 2 + s, rounded up to seq_align; d_flags is read as well.
 * A row index outside [0, n_total) is LDDL_EINDEX (checked before any load
 * through it). */
int lddl_collate_code_rows_seq_len(lddl_ctx *ctx, const uint16_t *d_len0, const uint16_t *d_len1,
                                   const uint8_t *d_flags, const int64_t *d_rows, int64_t row0, int64_t n_rows,
                                   int64_t n_total, int32_t seq_align, int64_t *out_seq_len, void *stream);

/* Fill the [n_rows, seq_len] int64 outputs of a padded batch of CodeBERT rows
 * (pretrain_codebert.py:425-433; no loader in the reference), pad columns
 * with id 0, attention 0 and special 1.  d_labels by mode 0 / 2 as above.
 * Errors, first one wins, none faults, a refused row is left unwritten:
 * LDDL_EINDEX (a row index outside [0, n_total), checked before any load
 * through it), LDDL_EINVAL (n_rows <= 0; a mode other than 0 or 2: CodeBERT
 * has no static masks; a row with s = 0 and a > 0, which the packer never
 * makes), LDDL_ECAPACITY (a row longer than seq_len, seq_len > 2048). */
int lddl_collate_code_rows(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                           const uint16_t *d_len0, const uint16_t *d_len1, const uint8_t *d_flags,
                           const int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t n_total, int64_t seq_len,
                           int32_t mode, int64_t ignore_index, double mlm_probability, uint64_t seed, uint64_t counter,
                           int64_t *d_input_ids, int64_t *d_token_type_ids, int64_t *d_attention_mask,
                           int64_t *d_labels, void *stream);

/* lddl_collate_rows_cu_seqlens for CodeBERT rows (pretrain_codebert.py:425-433;
 * no loader in the reference): d_cu_seqlens is the exclusive scan of
 * n_r = a + b + 2 + s as int32 [n_rows + 1], *out_total = T, *out_max_seqlen =
 * max n_r; d_flags is read as well.  LDDL_EINDEX (a row index outside
 * [0, n_total)), LDDL_EINVAL (n_rows <= 0), LDDL_ECAPACITY (T >= 2^31, summed
 * in 64 bits; d_cu_seqlens is then left unwritten). */
int lddl_collate_code_rows_cu_seqlens(lddl_ctx *ctx, const uint16_t *d_len0, const uint16_t *d_len1,
                                      const uint8_t *d_flags, const int64_t *d_rows, int64_t row0, int64_t n_rows,
                                      int64_t n_total, int32_t *d_cu_seqlens, int64_t *out_total,
                                      int64_t *out_max_seqlen, void *stream);

/* The padding-free batch of CodeBERT rows (pretrain_codebert.py:425-433; no
 * loader in the reference): lddl_collate_code_rows at the same seed and
 * counter with every column j >= n_r dropped, bit for bit in modes 0 and 2.
 * For t = cu_seqlens[r] + j: input_ids[t], token_type_ids[t], d_labels[t] are
 * column j of row r, position_ids[t] = j; the four outputs are [total].
 * d_cu_seqlens is checked, not trusted.  Errors, first one wins, none faults,
 * the row is left unwritten and no row stores outside its own tokens:
 * LDDL_EINDEX (a row index outside [0, n_total)), LDDL_EINVAL (n_rows <= 0; a
 * mode other than 0 or 2: CodeBERT has no static masks; a row with s = 0 and
 * a > 0; a row with cu_seqlens[r] < 0, cu_seqlens[r + 1] - cu_seqlens[r] !=
 * n_r or cu_seqlens[r] + n_r > total), LDDL_ECAPACITY (a row longer than 2048
 * tokens, total >= 2^31). */
int lddl_collate_code_rows_unpadded(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0,
                                    const int64_t *d_src1, const uint16_t *d_len0, const uint16_t *d_len1,
                                    const uint8_t *d_flags, const int64_t *d_rows, int64_t row0, int64_t n_rows,
                                    int64_t n_total, const int32_t *d_cu_seqlens, int64_t total, int32_t mode,
                                    int64_t ignore_index, double mlm_probability, uint64_t seed, uint64_t counter,
                                    int64_t *d_input_ids, int64_t *d_token_type_ids, int64_t *d_position_ids,
                                    int64_t *d_labels, void *stream);

/* lddl_collate_rows_fixed for CodeBERT rows (pretrain_codebert.py:425-433; no
 * loader in the reference): the real part is lddl_collate_code_rows_cu_seqlens +
 * lddl_collate_code_rows_unpadded, bit for bit in modes 0 and 2; the slack, the
 * cu_seqlens tail, d_status and the three counts as there.  No static arrays
 * and no next_sentence_labels.  Errors as there, with max_seqlen in [2, 2048],
 * a mode other than 0 or 2 LDDL_EINVAL, and LDDL_EINVAL for a row with s = 0
 * and a > 0 in place of the CodeBERT-row refusal. */
int lddl_collate_code_rows_fixed(lddl_ctx *ctx, const uint16_t *d_ids, const int64_t *d_src0, const int64_t *d_src1,
                                 const uint16_t *d_len0, const uint16_t *d_len1, const uint8_t *d_flags,
                                 const int64_t *d_rows, int64_t row0, int64_t n_rows, int64_t n_total,
                                 int32_t *d_cu_seqlens, int64_t tok_cap, int64_t seq_cap, int64_t max_seqlen,
                                 int32_t mode, int64_t ignore_index, double mlm_probability, uint64_t seed,
                                 uint64_t counter, int64_t *d_input_ids, int64_t *d_token_type_ids,
                                 int64_t *d_position_ids, int64_t *d_labels, int32_t *d_status, int64_t *out_total,
                                 int64_t *out_n_rows, int64_t *out_n_seqs, void *stream);

/* ---- compact MLM targets ----------------------------------------------------
 * The masked positions of a batch and their labels, in order: what a trainer
 * gathers the hidden states at before the LM head, so that the vocabulary
 * projection and its loss run over the ~15 % of the tokens that are selected.
 * The static shards carry these lists per row (masked_lm_positions /
 * masked_lm_labels, scattered by bert.py:113-116); with dynamic masking they
 * never exist.  d_labels is the int64 [total] labels of any collate call of
 * this header or of lddl_mask_tokens; its rows are given by one of
 *   padded   d_cu_seqlens NULL: row r is [r * seq_len, (r + 1) * seq_len),
 *            total = n_rows * seq_len;
 *   offsets  d_cu_seqlens int32 [n_rows + 1] on the device: row r is
 *            [cu[r], cu[r + 1]) inside [0, total); seq_len is not read; an empty
 *            row (cu[r] == cu[r + 1]) is legal, and tokens of d_labels that lie
 *            in no row are ignored.
 * With F the ascending list of the flat indices t that lie inside a row and
 * have d_labels[t] != ignore_index, and M its length:
 *   d_positions[k] = F[k], d_target_labels[k] = d_labels[F[k]]   for k < M
 *   d_positions[k] = 0,    d_target_labels[k] = ignore_index     for M <= k < capacity
 *   d_offsets[r] = the selected tokens of the rows before r, d_offsets[n_rows] = M
 * d_positions and d_target_labels are int64 [capacity], d_offsets int32
 * [n_rows + 1]; labels pass through as 64-bit values.  The padded tail is
 * harmless to a loss that honours ignore_index and gives fixed shapes.  The
 * order is fixed: no result depends on the arrival order of an atomic.
 * Synchronises the stream; *out_count = M on every return that got as far as
 * counting, a device error included (it is left alone before that).
 * Errors, first one wins, none faults: LDDL_EINVAL (a NULL ctx, output or
 * out_count, NULL d_labels with total > 0; n_rows <= 0; ignore_index >= 0, which
 * could be a label; total or capacity < 0; padded with seq_len < 1 or total !=
 * n_rows * seq_len), LDDL_ECAPACITY (total or n_rows >= 2^31: d_offsets is
 * int32), then from the device LDDL_EINVAL (a row with cu[r] < 0,
 * cu[r + 1] < cu[r] or cu[r + 1] > total: d_cu_seqlens is checked, not trusted;
 * such a row counts 0 and is never read through, and the three outputs are
 * unspecified), LDDL_ECAPACITY (M > capacity: the three outputs are
 * unspecified but never written out of bounds, and *out_count holds M, so the
 * caller can resize). */
int lddl_mlm_targets(lddl_ctx *ctx, const int64_t *d_labels, int64_t n_rows, int64_t seq_len,
                     const int32_t *d_cu_seqlens, int64_t total, int64_t ignore_index, int64_t capacity,
                     int64_t *d_positions, int64_t *d_target_labels, int32_t *d_offsets, int64_t *out_count,
                     void *stream);

/* ---- a row table from the shards on disk ----------------------------------
 * The bridge from parquet shards to lddl_collate_rows[_unpadded]: the string
 * columns of a shard (A, B, is_random_next and, with static masking,
 * masked_lm_positions / masked_lm_labels; the layout lddl_collate_bert takes)
 * become what lddl_row_spans + lddl_masked_lm_spans leave behind for a pack
 * result, once per shard instead of once per batch per epoch.  This is the
 * decode-and-lookup half of the reference's loader: lddl/torch/bert.py:42-60
 * `_decode_record_batch`, :83-89 and :109-124 (`split()` and
 * `convert_tokens_to_ids`) and lddl/utils.py `deserialize_np_array`; the
 * padding half (bert.py:90-149) stays in lddl_collate_rows[_unpadded].
 * d_pos .. d_lab_off are all four NULL without static masking, and then so
 * are the d_*mlm_* arrays; anything in between is LDDL_EINVAL.
 *
 * lddl_rows_from_strings_len: per row r, d_out_len0[r] = a = tokens of
 * A.split(), d_out_len1[r] = b = tokens of B.split(); with n_r = a + b + 3 and
 * k_r = the row's positions, the exclusive scans (64-bit) d_out_src0[r] =
 * sum of a + b over the rows before r, d_out_src1[r] = d_out_src0[r] + a,
 * d_out_tok_off (optional, [n_rows + 1]) of n_r and d_out_mlm_off (static
 * masking, [n_rows + 1]) of k_r.  out_totals = {ids = sum of a + b, masked
 * entries = sum of k_r, row tokens = sum of n_r}.  Synchronises the stream
 * once.
 * Errors, first one wins, none faults: LDDL_ECAPACITY (a segment of more than
 * 65535 tokens: len0 / len1 are 16 bits, so no row exceeds 2 * 65535 + 3
 * tokens; more positions than that), LDDL_EFORMAT (positions that are not
 * np.save bytes of a uint16 array, a label count different from the position
 * count), LDDL_EINDEX (a position >= n_r: lddl_collate_bert refuses only
 * >= seq_len, which depends on the batch; a table has no batch and takes the
 * stricter rule of lddl_collate_rows_unpadded), LDDL_EINVAL (n_rows <= 0, a
 * NULL required pointer, static outputs without static inputs or the reverse,
 * a vocabulary of more than 65536 entries: an id would not fit 16 bits). */
int lddl_rows_from_strings_len(lddl_ctx *ctx, const uint8_t *d_a, const int64_t *d_a_off, const uint8_t *d_b,
                               const int64_t *d_b_off, const uint8_t *d_pos, const int64_t *d_pos_off,
                               const uint8_t *d_lab, const int64_t *d_lab_off, int64_t n_rows, uint16_t *d_out_len0,
                               uint16_t *d_out_len1, int64_t *d_out_src0, int64_t *d_out_src1, int64_t *d_out_tok_off,
                               int64_t *d_out_mlm_off, int64_t out_totals[3], void *stream);

/* Fill the table (same seam: bert.py:83-89, :109-124): d_out_ids[src0[r] ..
 * + a) = the ids of A's tokens, d_out_ids[src1[r] .. + b) = of B's ([UNK] for
 * a miss), d_out_flags[r] = (is_random_next[r] ? 1 : 0) | 2, and with static
 * masking for j < k_r at e = mlm_off[r] + j: d_out_mlm_pos[e] = the j-th
 * position, d_out_mlm_label[e] = the id of the j-th label token,
 * d_out_mlm_token[e] = what the row shows there ([CLS], [SEP] or the A / B
 * id: A and B of a masked shard hold the masked tokens already).  d_len0 ..
 * d_mlm_off are lddl_rows_from_strings_len's outputs and are checked, not
 * trusted: every row's tokens are counted again.  ids_cap / mlm_cap: the
 * entries of d_out_ids / of each d_out_mlm_* array that may be written, at
 * least that call's totals.  The caller keeps d_out_ids 16-B aligned with 16
 * zeroed entries behind the total (not counted in ids_cap, never written
 * here): lddl_collate_rows expects that padding.  Synchronises the stream.
 * Errors as lddl_rows_from_strings_len, and: LDDL_ECAPACITY (the table ends
 * beyond ids_cap or mlm_cap: nothing is written), LDDL_EINVAL (a row whose
 * len0 / len1 / src0 / src1 / mlm_off are not what its strings give, or whose
 * span leaves the capacities).  A refused row is left unwritten and a row
 * stores only inside [src0[r], src0[r] + a + b) and [mlm_off[r], mlm_off[r +
 * 1]) as given, within the capacities; a src0 altered to another value inside
 * the capacity is not detected (a row cannot know the running sum). */
int lddl_rows_from_strings(lddl_ctx *ctx, const uint8_t *d_a, const int64_t *d_a_off, const uint8_t *d_b,
                           const int64_t *d_b_off, const uint8_t *d_pos, const int64_t *d_pos_off, const uint8_t *d_lab,
                           const int64_t *d_lab_off, const uint8_t *d_is_random_next, int64_t n_rows,
                           const uint16_t *d_len0, const uint16_t *d_len1, const int64_t *d_src0, const int64_t *d_src1,
                           const int64_t *d_mlm_off, uint16_t *d_out_ids, int64_t ids_cap, uint8_t *d_out_flags,
                           uint16_t *d_out_mlm_pos, uint16_t *d_out_mlm_label, uint16_t *d_out_mlm_token,
                           int64_t mlm_cap, void *stream);

/* ---- a row table from CodeBERT shards ---------------------------------------
 * The two calls above for the shards of the CodeBERT preprocessor: the row
 * pretrain_codebert.py:425-433 saves as id / doc / code / num_tokens (the
 * reference has no loader for it; the id column is not read).  d_doc /
 * d_code: Arrow bytes + int64 offsets [n_rows + 1]; d_num_tokens: uint16
 * [n_rows] on the device.  Per row a = tokens of doc.split(), b = tokens of
 * code.split(), s = num_tokens - a - b - 2 (1 when a [SEP] follows the doc
 * segment), flags = s << 1.
 *
 * lddl_code_rows_from_strings_len: d_out_len0[r] = a, d_out_len1[r] = b,
 * d_out_src0[r] = the sum of a + b over the rows before r, d_out_src1[r] =
 * d_out_src0[r] + a, d_out_tok_off (optional, [n_rows + 1]) the exclusive scan
 * of a + b + 2 + s; out_totals = {ids = sum of a + b, row tokens}.
 * Synchronises the stream once.  Errors, first one wins, none faults:
 * LDDL_ECAPACITY (a segment of more than 65535 tokens), LDDL_EFORMAT (a
 * num_tokens that is not a + b + 2 or a + b + 3, or is a + b + 2 with a > 0:
 * doc tokens with no [SEP] to end them), LDDL_EINVAL (n_rows <= 0, a NULL
 * pointer, a vocabulary of more than 65536 entries). */
int lddl_code_rows_from_strings_len(lddl_ctx *ctx, const uint8_t *d_doc, const int64_t *d_doc_off,
                                    const uint8_t *d_code, const int64_t *d_code_off, const uint16_t *d_num_tokens,
                                    int64_t n_rows, uint16_t *d_out_len0, uint16_t *d_out_len1, int64_t *d_out_src0,
                                    int64_t *d_out_src1, int64_t *d_out_tok_off, int64_t out_totals[2],
                                    void *stream);

/* Fill the table from a CodeBERT shard (pretrain_codebert.py:425-433; no
 * loader in the reference): d_out_ids[src0[r] .. + a) = the ids of doc's
 * tokens, d_out_ids[src1[r] .. + b) = of code's ([UNK] for a miss),
 * d_out_flags[r] = s << 1.  d_len0 .. d_src1 are the length call's outputs and
 * are checked, not trusted: every row is counted again, and its num_tokens
 * checked again, before anything is stored.  ids_cap and the padding behind
 * d_out_ids as in lddl_rows_from_strings.  Synchronises the stream.  Errors as
 * the length call, and: LDDL_ECAPACITY (the table ends beyond ids_cap: nothing
 * is written), LDDL_EINVAL (a row whose len0 / len1 / src0 / src1 are not what
 * its strings give, or whose span leaves the capacity).  A refused row is
 * left unwritten and a row stores only inside [src0[r], src0[r] + a + b). */
int lddl_code_rows_from_strings(lddl_ctx *ctx, const uint8_t *d_doc, const int64_t *d_doc_off, const uint8_t *d_code,
                                const int64_t *d_code_off, const uint16_t *d_num_tokens, int64_t n_rows,
                                const uint16_t *d_len0, const uint16_t *d_len1, const int64_t *d_src0,
                                const int64_t *d_src1, uint16_t *d_out_ids, int64_t ids_cap, uint8_t *d_out_flags,
                                void *stream);

/* ---- BART: sentence aggregation --------------------------------------------
 * The reference's third preprocessor (lddl/dask/bart/pretrain.py) cuts every
 * document into chunks of whole sentences and saves one string column,
 * `sentences`.  Input: the sentence-split corpus of lddl_tokenize (d_data,
 * d_sent_off [n_sent + 1], d_doc_sent_off [n_doc + 1]); a document is one
 * input line taken whole (the reference does not split off a leading id here,
 * pretrain.py:82-86, so the id is part of the first sentence), its sentences
 * stripped and the empty ones dropped by the front end.  No vocabulary is
 * read and nothing is drawn at random.  The offsets are checked, not trusted:
 * none of these calls loads or stores through an offset outside its array.
 *
 * lddl_bart_count: d_out_nwords[s] = len(sentence.split()) of bytes
 * [sent_off[s], sent_off[s + 1]) as int32 (pretrain.py:113), with Python's
 * whitespace rule for str (the characters str.isspace() accepts).  A
 * sentence's first character starts a word whenever it is not whitespace,
 * whatever byte precedes it in d_data; no byte outside the sentence is read.
 * Synchronises the stream.  LDDL_EINVAL: a NULL pointer, a negative count, a
 * sentence whose offsets run backwards or leave [0, nbytes] (its count is 0). */
int lddl_bart_count(lddl_ctx *ctx, const uint8_t *d_data, int64_t nbytes, const int64_t *d_sent_off, int64_t n_sent,
                    int32_t *d_out_nwords, void *stream);

/* The chunk plan, length pass (pretrain.py:88-128 `_aggregate_sentences`):
 * with T = target_seq_length - 3, a document's sentences are walked in order;
 * each adds its d_nwords to a running count, and when the count reaches >= T
 * the chunk closes and the count restarts at 0; after the last sentence the
 * remainder is a chunk only when its count is > 0 (a remainder of 0-word
 * sentences is dropped with its text; a document of only such sentences, or
 * of none, yields nothing unless T <= 0, where every sentence closes a chunk
 * as the reference's `>=` has it).  d_out_doc_chunk_off [n_doc + 1] (int64) =
 * the chunks per document in exclusive-scan form; out_totals = {n_chunks, the
 * bytes of all chunk texts}, a chunk's bytes being the sum of 1 + len(sentence)
 * over its sentences (pretrain.py:112), summed in 64 bits.  Synchronises the
 * stream once.  LDDL_EINVAL: a NULL pointer, a negative count, d_doc_sent_off
 * not ending at n_sent, a document or sentence whose offsets run backwards or
 * leave their array; LDDL_ECAPACITY: a chunk of 2^31 bytes or more. */
int lddl_bart_plan_len(lddl_ctx *ctx, const int32_t *d_nwords, const int64_t *d_sent_off,
                       const int64_t *d_doc_sent_off, int64_t n_doc, int64_t n_sent, int32_t target_seq_length,
                       int64_t *d_out_doc_chunk_off, int64_t out_totals[2], void *stream);

/* The chunk plan, fill pass: per chunk c (document-major, in the reference's
 * order) d_out_chunk_sent0[c] = its first sentence (int64), d_out_chunk_nsent[c]
 * = its sentences, d_out_chunk_num_tokens[c] = the reference's num_tokens
 * (pretrain.py:115-119; int32 both), and d_out_chunk_off [n_chunks + 1] = the
 * Arrow offsets of the chunk texts (int64).  d_doc_chunk_off and n_chunks are
 * lddl_bart_plan_len's and are checked against the walk, not trusted.
 * Synchronises the stream.  Errors as lddl_bart_plan_len, and LDDL_EINVAL when
 * d_doc_chunk_off / n_chunks are not what that call gives. */
int lddl_bart_plan(lddl_ctx *ctx, const int32_t *d_nwords, const int64_t *d_sent_off, const int64_t *d_doc_sent_off,
                   const int64_t *d_doc_chunk_off, int64_t n_doc, int64_t n_sent, int32_t target_seq_length,
                   int64_t n_chunks, int64_t *d_out_chunk_sent0, int32_t *d_out_chunk_nsent,
                   int32_t *d_out_chunk_num_tokens, int64_t *d_out_chunk_off, void *stream);

/* The `sentences` column of chunks [c0, c0 + n) (pretrain.py:112 `chunk += " "
 * + sentence`, :136-147): d_out_off [n + 1] = their Arrow offsets rebased to
 * 0, d_out_bytes = each chunk's sentences with one space in front of every
 * sentence.  Two-phase like lddl_render_strings: with d_out_bytes == NULL only
 * d_out_off and *out_nbytes are produced; out_cap < *out_nbytes is
 * LDDL_ECAPACITY with no byte written.  The chunk arrays (n_chunks entries,
 * d_chunk_off n_chunks + 1) are checked, not trusted: before it stores, a
 * chunk checks that its sentences lie in [0, n_sent), that their offsets run
 * forward inside [0, nbytes], that bytes + spaces equal chunk_off[c + 1] -
 * chunk_off[c] and that its span lies in [0, out_cap).  A refused chunk is
 * left unwritten, no chunk stores outside its own span, and the call returns
 * LDDL_EINVAL naming the lowest refused chunk.  Synchronises the stream. */
int lddl_bart_render(lddl_ctx *ctx, const uint8_t *d_data, int64_t nbytes, const int64_t *d_sent_off, int64_t n_sent,
                     const int64_t *d_chunk_sent0, const int32_t *d_chunk_nsent, const int64_t *d_chunk_off,
                     int64_t n_chunks, int64_t c0, int64_t n, int64_t *d_out_off, uint8_t *d_out_bytes,
                     int64_t out_cap, int64_t *out_nbytes, void *stream);

/* ---- Sentence split: raw records to the sentence-split corpus ---------------
 * The corpus lddl_tokenize and lddl_bart_* read (d_data, d_sent_off,
 * d_doc_sent_off) made on the device from raw records: d_buf [nbytes] holds
 * the records back to back, record r = bytes [rec_off[r], rec_off[r + 1]),
 * document r of the result.  The split is the front end's rule-based one
 * (preprocess._rule_split; the reference calls nltk.sent_tokenize at
 * pretrain.py:82-97 `_to_document` and bart/pretrain.py:82-86), each piece
 * stripped of whitespace and the empty ones dropped, with Python's str
 * semantics per code point.  mode 0 (BERT) first splits the id off as
 * readers.py:142-147 does: the id ends at the first whitespace character,
 * the body starts one character after it; mode 1 (BART) splits the whole
 * record.  No byte outside [0, nbytes) is read (no padding is needed), no
 * record reads into its neighbour, and every record must be strict UTF-8.
 *
 * lddl_set_split_props: the code point properties the rules read, one byte
 * per code point (bit 0 str.isspace, 1 isupper, 2 isdigit, 3 "lowers to one
 * alphabetic character"), copied to the device; n must be 0x110000.
 * LDDL_EINVAL otherwise. */
int lddl_set_split_props(lddl_ctx *ctx, const uint8_t *host_tab, int64_t n);

/* The length call (replaces the host's pretrain.py:82-97 / bart/pretrain.py:82-86
 * and readers.py:142-147 seams): d_out_doc_sent_off [n_rec + 1] (int64) = the
 * sentences per record in exclusive-scan form, d_out_id_end [n_rec] (int64;
 * may be NULL in mode 1) = where each record's id ends in d_buf (its id is
 * [rec_off[r], id_end[r]); rec_off[r] in mode 1), out_totals = {n_sent, the
 * sentences' bytes}.  Synchronises the stream once.  LDDL_EINVAL: a NULL
 * pointer, a negative count, a mode other than 0 or 1, no property table,
 * d_rec_off not starting at 0, running backwards or not ending at nbytes;
 * LDDL_ECAPACITY: nbytes >= 2^31; LDDL_EFORMAT: a record that is not strict
 * UTF-8, *out_bad_rec = the lowest such record (-1 otherwise) and the outputs
 * undefined. */
int lddl_split_len(lddl_ctx *ctx, const uint8_t *d_buf, int64_t nbytes, const int64_t *d_rec_off, int64_t n_rec,
                   int32_t mode, int64_t *d_out_doc_sent_off, int64_t *d_out_id_end, int64_t out_totals[2],
                   int64_t *out_bad_rec, void *stream);

/* The fill call: d_out_data [out_bytes + 16] = the sentences back to back and
 * 16 zero bytes (lddl_tokenize's padding), d_out_sent_off [n_sent + 1] (int64)
 * their offsets from 0.  d_doc_sent_off, n_sent and out_bytes are
 * lddl_split_len's for the same input; nothing of that call is kept in the
 * ctx, so its passes run again and the three are compared with what they
 * give before anything is stored: a difference is LDDL_EINVAL with nothing
 * written, and no store leaves [0, out_bytes + 16) / [0, n_sent].
 * Synchronises the stream once (before the stores, which are queued on it).
 * Other errors as lddl_split_len. */
int lddl_split(lddl_ctx *ctx, const uint8_t *d_buf, int64_t nbytes, const int64_t *d_rec_off, int64_t n_rec,
               int32_t mode, const int64_t *d_doc_sent_off, int64_t n_sent, int64_t out_bytes, uint8_t *d_out_data,
               int64_t *d_out_sent_off, void *stream);

#ifdef __cplusplus
}
#endif
#endif
