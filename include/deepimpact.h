/*
 * deepimpact.h -- C ABI of libdeepimpact_hip.so, the MI355X-native (gfx950)
 * DeeperImpact encode-and-retrieve path.
 *
 * The reference (Tommachilez/improving-learned-index) has no FFI layer: its
 * boundary is a set of Python protocols and file formats.  Each
 * entry point below names the reference interface it replaces (path:line,
 * relative to the reference repository root).  The Python host side
 * (improving-learned-index_amd/) binds these through ctypes; INTEGRATION.md
 * shows the binding a maintainer would add to the reference itself.
 *
 * Conventions
 *   - Every function returns DI_OK (0) or a negative DI_E* code; the message of
 *     the last failure on the calling thread is di_last_error().  No C++
 *     exception crosses the ABI.
 *   - Array arguments are borrowed for the duration of the call.  Unless the
 *     DI_F_DEVICE_PTRS flag is given they are host pointers; with it they are
 *     device pointers on the handle's device (inputs already resident in HBM).
 *   - Outputs are caller-allocated; their sizes are known before the call.
 *   - One handle per device.  A handle is not thread-safe; different handles
 *     may be used concurrently.  Each handle owns one HIP stream (replaceable
 *     with di_*_set_stream); calls are synchronous at return unless
 *     DI_F_ASYNC is given together with DI_F_DEVICE_PTRS.
 */
#ifndef DEEPIMPACT_H
#define DEEPIMPACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DI_OK 0
#define DI_EINVAL (-1)   /* bad argument                                   */
#define DI_ENOMEM (-2)   /* host or device allocation failed                */
#define DI_EHIP (-3)     /* HIP runtime error                               */
#define DI_ERANGE (-4)   /* a documented size limit was exceeded            */
#define DI_ENODEV (-5)   /* no HIP device                                   */
#define DI_EIO (-6)      /* file could not be read                          */
#define DI_EFORMAT (-7)  /* file content does not follow the reference format */

#define DI_F_DEVICE_PTRS 0x1u /* array arguments are device pointers           */
#define DI_F_ASYNC 0x2u       /* do not synchronise the stream before return   */
#define DI_F_TIMING 0x4u      /* record HIP events around every kernel         */
#define DI_F_LISTS_MAJOR 0x8u /* di_topk_merge: keys are [list][query][k]       */

/* Limits of the retrieval kernels (documented in DESIGN.md). */
#define DI_SHORT_QUERY_TERMS 256 /* queries up to this many known terms use the compact key */
#define DI_MAX_QUERY_TERMS 4096  /* known terms per query of the quantized scorer; longer
                                    than DI_SHORT_QUERY_TERMS: wide keys, shard docs < 2^24 */
#define DI_MAX_TOPK 4096
#define DI_MAX_SPARSE_QUERY_TERMS 4096 /* float search: known terms per query (chunked) */
#define DI_MAX_SPARSE_DOCS 16777215u /* float index: doc ids embedded in 24 bits   */

const char *di_last_error(void);
int di_version(void); /* (major << 16) | minor */
int di_device_count(int *n);

/* Per-kernel timing collected under DI_F_TIMING (HIP events on the launching
 * stream).  `name` is the kernel's short name, e.g. "score_blocks".  Returns the
 * summed milliseconds and the number of launches since the last reset. */
typedef struct di_timing {
    double ms;
    int64_t launches;
} di_timing;

/* ======================================================================
 * On-disk quantized index: build and score                  (A11, A12)
 * ====================================================================== */
typedef struct di_index di_index;

/* Replaces InvertedIndexCreator (src/deep_impact/inverted_index/create.py:12-55)
 * as the producer of the device index, and InvertedIndex.__init__
 * (src/deep_impact/inverted_index/inverted_index.py:18-20).
 * Input: postings in the reference file order -- term-major, value descending,
 * doc ascending -- as CSR: term_off[n_terms+1] (posting index), pdoc[], pval[].
 * Postings from the first zero value of a term on are dropped, exactly as
 * InvertedIndex.term_docs stops there (inverted_index.py:50-51).
 * Only docs in [doc_lo, doc_hi) are kept (one shard of a doc-id-sharded index);
 * doc ids stay global.  doc_hi = 0 means "max doc + 1".                        */
int di_index_create(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                    const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, int device,
                    di_index **out);

/* di_index_create with the blocked device layout built on the GPU: the same index, byte
 * for byte (di_index_export), from the same arguments.  With DI_F_DEVICE_PTRS term_off,
 * pdoc and pval are device pointers (e.g. di_index_builder_postings' device output) and only
 * status words and sizes are read back; host pointers are copied to the device first.
 * term_off is checked on the device (DI_EINVAL through an error word read once); the other
 * errors are di_index_create's.  One deviation: a group of more than 2048 postings -- a doc
 * repeated inside a term so that one 2048-doc wave segment of a block overfills, or
 * DI_WLONG_MIN above 2049 with such a short sublist -- is DI_EINVAL here, where
 * di_index_create takes it silently.  Runs on hip_stream and waits for it; its scratch (two
 * 16-byte records per kept posting) is freed at return.  DI_F_TIMING (read with
 * di_index_timing): "il_check", "il_input", "il_count", "il_scan", "il_compact", "il_hist",
 * "il_scatter", "il_heads", "il_entries", "il_long", "il_segment", "il_deal". */
int di_index_create_device(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                           const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, int device,
                           void *hip_stream, uint32_t flags, di_index **out);

/* The device layout read back, of an index from either route (the counterpart of
 * di_sparse_export).  di_index_layout: the (term, block) entries, the long sublists, the docs
 * per block and whether the flat posting array exists; with di_index_info's n_terms and
 * n_postings they size di_index_export's host arrays: post and post_flat [n_postings]
 * (post_flat only when *has_flat), tb_start [n_terms + 1], eblk [n_ent], epos [n_ent + 1],
 * seg [8 n_ent], lid [n_ent], wmeta [128 n_long], emax [n_ent], wmax [16 n_long].  Any
 * pointer may be NULL. */
int di_index_layout(const di_index *ix, int64_t *n_ent, int64_t *n_long, int32_t *block_docs,
                    int32_t *has_flat);
int di_index_export(const di_index *ix, uint32_t *post, uint32_t *post_flat, uint32_t *tb_start,
                    uint16_t *eblk, uint32_t *epos, uint16_t *seg, uint32_t *lid, uint16_t *wmeta,
                    uint8_t *emax, uint8_t *wmax);

/* Native host builder of the reference files: replaces InvertedIndexCreator.run
 * (create.py:53-55) reading the collection like DeepImpactCollection
 * (src/deep_impact/indexing/deep_impact_collection.py:6-33).  Writes
 * <out_dir>/vocab.txt, inverted_index.idx, inverted_index.dat byte-identical to
 * the reference.  Malformed lines fail with DI_EFORMAT where the reference raises. */
int di_build_reference_index(const char *collection_path, const char *out_dir);

/* Reads <dir>/inverted_index.idx and <dir>/inverted_index.dat (create.py:45-51,
 * formats src/utils/defaults.py:22-37).  vocab.txt stays on the host side.  The files are
 * parsed on host threads; the parsed CSR goes to di_index_create_device, or, with
 * DI_INDEX_LAYOUT=host in the environment, to di_index_create (the same index). */
int di_index_load_reference(const char *dir, uint32_t doc_lo, uint32_t doc_hi, int device,
                            di_index **out);

/* Replaces InvertedIndex.score (inverted_index.py:55-62) for a batch of queries.
 * q_terms: term ids of all queries in iteration order (the reference iterates a
 * Python set; its order is the tie order), CSR by cu_q[n_q+1].  For each query
 * the top-k (doc, score) pairs are written in the reference's order -- score
 * descending, ties in first-touch order -- to out_doc/out_score[q*k ...] and the
 * count to out_n[q].  out_key (may be NULL) receives the 64-bit merge keys used
 * to combine shards (di_topk_merge; wide keys for queries of more than
 * DI_SHORT_QUERY_TERMS terms, see di_key_doc_wide).  A query over a kernel limit
 * (more than DI_MAX_QUERY_TERMS terms; a long query on a shard reaching doc 2^24;
 * an unknown term id) fails the call with DI_ERANGE / DI_EINVAL for host pointers,
 * and gets out_n[q] = -1 with DI_F_DEVICE_PTRS (the caller must check).          */
int di_index_search(di_index *ix, const uint32_t *q_terms, const int32_t *cu_q, int32_t n_q,
                    int32_t k, uint32_t *out_doc, uint32_t *out_score, int32_t *out_n,
                    uint64_t *out_key, uint32_t flags);

/* Pre-allocates device workspace for batches of up to max_q queries at top-k. */
int di_index_reserve(di_index *ix, int32_t max_q, int32_t k);
int di_index_info(const di_index *ix, int64_t *n_terms, int64_t *n_postings, uint32_t *n_docs,
                  int32_t *n_blocks);
/* Query-time impact pruning (BASELINE configs[4], the QPS-vs-recall@1000 sweep): score
 * only the postings with value >= 2^floor(log2 min_impact) -- a prefix of every
 * (term, block) sublist, which the index keeps grouped by impact class.  1 (the
 * default) scores every posting: exactly InvertedIndex.score (inverted_index.py:55-62);
 * anything larger is an approximation whose recall bench tools measure.  No reference
 * counterpart (the reference scores exhaustively).                                  */
int di_index_set_min_impact(di_index *ix, int32_t min_impact);
/* Block-max skipping (BASELINE configs[4]): per (term, block) and per (long sublist, wave
 * segment of 2048 docs) the largest value is kept at build time; a segment whose bound
 * (the sum over the query terms of those maxima) stays below the query's running top-k
 * threshold is not scored.  factor 0: off (default); 1: exact -- the same ranking as
 * InvertedIndex.score (inverted_index.py:55-62); in (1, 16]: skips segments below
 * factor x threshold, an approximation (QPS vs recall@1000).  Queries of at most 64
 * terms, with the shared threshold (>= 8 blocks).  Long sublists: >= 128 postings in a
 * block.  di_index_timing("bm_segments" / "bm_segments_skipped") counts the evaluated
 * and skipped segments.  Items run block-major; DI_BLOCK_ORDER=1 (environment, at index
 * creation) runs each query's blocks in descending bound order instead. */
int di_index_set_block_max(di_index *ix, float factor);
/* Packed (block-compressed) postings -- BASELINE configs[4]: on != 0 builds (once, from
 * the device layout) a second copy of the postings in which every run (a short
 * (term, block) sublist, or one scorer wave segment's run of a long one) is sorted by doc
 * and cut into frames of up to 512 postings, each bit-packed with its own widths (doc
 * deltas in bd bits, value - vmin in bv bits, decoded in registers by the scorer), and
 * scores queries of at most 64 terms from it, alone or with block-max skipping; the
 * ranking is unchanged (same keys).  Exact scoring only: with impact pruning
 * (di_index_set_min_impact > 1) the plain layout is used.  *packed_bytes (optional)
 * receives the packed size (headers + data).  on = 0: the plain layout again. */
int di_index_set_packed(di_index *ix, int32_t on, int64_t *packed_bytes);
int di_index_set_stream(di_index *ix, void *hip_stream);
int di_index_sync(di_index *ix);
/* Per-kernel HIP-event time ("score_blocks", "merge_topk") accumulated over DI_F_TIMING
 * searches; also the block-max counters "bm_segments" (wave segments evaluated) and
 * "bm_segments_skipped" (segments not scored), returned in out->launches (ms = 0),
 * accumulated since the last reset (reading them synchronises the stream). */
int di_index_timing(di_index *ix, const char *name, di_timing *out, int reset);
int di_index_destroy(di_index *ix);

/* Combine per-shard top-k lists (from di_index_search out_key, or the sparse
 * index) into the global top-k: keys[(q*n_lists + l)*k + i], counts[q*n_lists+l]
 * (with DI_F_LISTS_MAJOR: keys[(l*n_q + q)*k + i], counts[l*n_q + q] -- the layout
 * an all-gather of per-shard results produces).
 * The keys are unique and totally ordered, so the result equals a single-shard
 * search over the whole collection.  Device pointers when DI_F_DEVICE_PTRS.
 * Replaces nothing in the reference (it has no sharded retrieval). */
int di_topk_merge(const uint64_t *keys, const int32_t *counts, int32_t n_q, int32_t n_lists,
                  int32_t k, uint64_t *out_key, int32_t *out_n, int device, void *hip_stream,
                  uint32_t flags);

/* The local steps of the pruned exact exchange of per-shard top-k lists between ranks
 * (parallel.exchange_topk; the collectives between them are the caller's all_gathers).
 * keys [n_q][k] descending merge keys (> 0), counts [n_q] (negative: rejected query).
 * Device pointers only, asynchronous on hip_stream.  Replaces nothing in the reference
 * (it has no sharded retrieval); the result feeds di_topk_merge, whose
 * output equals the merge of the full lists (ranker.py:43-48 keeps the global top-k).
 *   sample:  samples [n_q][k/g] = keys at positions g-1, 2g-1, ... (0 past counts[q]);
 *   count:   gathered_samples [world][n_q][k/g] -> T_q = the ceil(k/g)-th largest
 *            sample, ec [2][n_q] = (this rank's keys >= T_q, counts);
 *   offsets: gathered_ec [world][2][n_q] -> offsets [world][n_q] (exclusive scans of the
 *            key counts), totals [world];
 *   pack:    ec / offsets of this rank -> buf (its keys >= T_q back to back);
 *   unpack:  gathered [world][emax] -> out_keys [world][n_q][k], out_n [world][n_q]
 *            (the layout of a plain all_gather; DI_F_LISTS_MAJOR for di_topk_merge). */
int di_xchg_sample(const uint64_t *keys, const int32_t *counts, int32_t n_q, int32_t k,
                   int32_t g, uint64_t *samples, int device, void *hip_stream);
int di_xchg_count(const uint64_t *gathered_samples, int32_t world, const uint64_t *keys,
                  const int32_t *counts, int32_t n_q, int32_t k, int32_t g, int32_t *ec,
                  int device, void *hip_stream);
int di_xchg_offsets(const int32_t *gathered_ec, int32_t world, int32_t n_q, int64_t *offsets,
                    int64_t *totals, int device, void *hip_stream);
int di_xchg_pack(const uint64_t *keys, const int32_t *ec, const int64_t *offsets, int32_t n_q,
                 int32_t k, uint64_t *buf, int device, void *hip_stream);
int di_xchg_unpack(const uint64_t *gathered, int64_t emax, const int32_t *gathered_ec,
                   const int64_t *offsets, int32_t world, int32_t n_q, int32_t k,
                   uint64_t *out_keys, int32_t *out_n, int device, void *hip_stream);

/* ======================================================================
 * In-memory float index of the NanoBEIR evaluator           (A14, A15)
 * ====================================================================== */
typedef struct di_sparse di_sparse;

/* Replaces SparseSearch._build_inverted_index (nano_beir_evaluator.py:78-101):
 * per term, postings (doc = corpus position, float32 impact) in corpus order;
 * impacts <= 0 are dropped (:98).  n_docs <= DI_MAX_SPARSE_DOCS.
 * Precondition: among the kept postings of one term every doc occurs at most once
 * (the reference would add both impacts; the scorer applies a term's postings in
 * parallel); a term that repeats a doc fails the call with DI_EINVAL. */
int di_sparse_create(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                     const float *pimp, uint32_t n_docs, int device, di_sparse **out);

/* Replaces SparseSearch.search's scoring (nano_beir_evaluator.py:113-133):
 * float32 sums formed in the reference's order (bit-exact under numpy >= 2),
 * top-k by score with ties in first-touch order.  out_key: merge keys
 * (score bits << 32 | (255 - first term) << 24 | (0xFFFFFF - doc)). */
int di_sparse_search(di_sparse *sp, const uint32_t *q_terms, const int32_t *cu_q, int32_t n_q,
                     int32_t k, uint32_t *out_doc, float *out_score, int32_t *out_n,
                     uint64_t *out_key, uint32_t flags);
/* The same search with float64 accumulation: the reference's pinned numpy 1.25.1,
 * where `0.0 + np.float32` is an np.float64 (nano_beir_evaluator.py:113-121, SURVEY
 * App. B.4).  f64 sums formed in the reference's order, top-k by f64 score with
 * ties in first-touch order; out_score: the f64 scores (the reference's float()). */
int di_sparse_search_f64(di_sparse *sp, const uint32_t *q_terms, const int32_t *cu_q,
                         int32_t n_q, int32_t k, uint32_t *out_doc, double *out_score,
                         int32_t *out_n, uint32_t flags);
int di_sparse_info(const di_sparse *sp, int64_t *n_terms, int64_t *n_postings, uint32_t *n_docs,
                   int32_t *n_blocks);
int di_sparse_timing(di_sparse *sp, const char *name, di_timing *out, int reset);
int di_sparse_destroy(di_sparse *sp);

/* ---- float index builder: the same index from (term id, impact) pairs per document,
 * e.g. di_encode's device output, assembled on the device ---- */
typedef struct di_sparse_builder di_sparse_builder;

int di_sparse_builder_create(int device, di_sparse_builder **out);
/* Room for n_docs documents and n_pairs kept pairs in all (optional: the pair buffers
 * grow by reallocation). */
int di_sparse_builder_reserve(di_sparse_builder *b, int64_t n_docs, int64_t n_pairs);
/* Appends n_docs documents; document d holds (term_ids[i], impacts[i]) for i in
 * [cu_terms[d], cu_terms[d + 1]) and gets corpus position *first_doc + d (append order).
 * Pairs whose impact is not > 0 (-0.0, 0.0, negatives, NaN) are dropped
 * (nano_beir_evaluator.py:98).  Arguments and flags as di_term_store_append: with
 * DI_F_DEVICE_PTRS the three arrays are device pointers (impacts = the buffer di_encode
 * wrote) and only cu_terms is read back.  Runs on hip_stream and waits for it.
 * cu_terms not starting at 0 or decreasing: DI_EINVAL; more than DI_MAX_SPARSE_DOCS
 * documents in all: DI_ERANGE (checked before any array is read); after an error the
 * builder is as it was before the call.  Term ids are checked by finish.
 * DI_F_TIMING: "sb_append". */
int di_sparse_builder_append(di_sparse_builder *b, const uint32_t *term_ids,
                             const float *impacts, const int32_t *cu_terms, int32_t n_docs,
                             int64_t *first_doc, void *hip_stream, uint32_t flags);
int di_sparse_builder_info(const di_sparse_builder *b, int64_t *n_docs, int64_t *n_pairs);
/* The index of everything appended, over terms 0 .. n_terms - 1 (ids used as given; a
 * term without a kept pair has an empty row): its four device arrays hold the bytes
 * di_sparse_create uploads for the same postings.  The builder is left unchanged.
 * Among the kept pairs, a term id >= n_terms or the same term twice in one document
 * (a repeated (term, doc) posting, as di_sparse_create rejects it): DI_EINVAL (an error
 * word set on the device and read once at the end, as di_encode reports a bad term
 * index); no index is returned then.  Runs on hip_stream and waits for it.
 * DI_F_TIMING: "sb_count", "sb_scan", "sb_scatter", "sb_order" (and the appends'
 * "sb_append") through di_sparse_timing of the returned index. */
int di_sparse_builder_finish(di_sparse_builder *b, int64_t n_terms, void *hip_stream,
                             uint32_t flags, di_sparse **out);
int di_sparse_builder_destroy(di_sparse_builder *b);

/* Copies the device layout to the host (any pointer may be NULL): term_start[n_terms],
 * blk_off[n_terms * (n_blocks + 1)], pdoc[n_postings] (doc % 16384), pimp[n_postings];
 * sizes from di_sparse_info.  Term t's postings of block b are
 * [term_start[t] + blk_off[t * (n_blocks + 1) + b], term_start[t] + blk_off[.. + b + 1]),
 * docs ascending. */
int di_sparse_export(const di_sparse *sp, int64_t *term_start, uint32_t *blk_off,
                     uint16_t *pdoc, float *pimp);

/* ======================================================================
 * Quantized index from the encoder's device output          (A10, A11)
 * ====================================================================== */
/* ---- term table: term strings (UTF-8) numbered in order of first appearance ---- */
typedef struct di_term_table di_term_table;

int di_term_table_create(di_term_table **out);
/* ids[i] = the id of term i of the batch, blob[term_off[i] .. term_off[i + 1]) (the
 * packed form the tokenizer workers return); a new term gets the next id.  A term the
 * text route would parse differently -- empty, with leading or trailing whitespace
 * (str.strip's), or holding ', ', ': ' or a line break (quantize.py:21-22,
 * deep_impact_collection.py:20-27) -- is DI_EFORMAT and the table is as before the
 * call; a bare ',' ':' or '|' inside a term is fine. */
int di_term_table_intern(di_term_table *t, const char *blob, const int64_t *term_off, int64_t n,
                         uint32_t *ids);
int di_term_table_info(const di_term_table *t, int64_t *n_terms, int64_t *n_bytes);
/* Every term in id order: blob[n_bytes], term_off[n_terms + 1]. */
int di_term_table_export(const di_term_table *t, char *blob, int64_t *term_off);
/* term_row[id] = the row of every term with term_count[id] > 0 when those are sorted
 * by their UTF-8 bytes -- sorted() on str, the order of vocab.txt (create.py:24-27) --
 * and -1 for every other term; *n_rows = the terms that have a row. */
int di_term_table_rows(const di_term_table *t, const int64_t *term_count, int32_t *term_row,
                       int64_t *n_rows);
/* di_term_table_rows over the single terms and the pair terms of
 * di_index_builder_pair_terms: term_row[id] for the n_terms ids of the table, then
 * term_row[n_terms + u] for pair u, whose name is term[first_id[u]] + '|' +
 * term[second_id[u]] (pairwise_impact.py:120-124); rows = sorted() over the UTF-8 bytes of
 * every single term with term_count > 0 and every pair name (the pair names are sorted on
 * DI_HOST_THREADS threads).  Two entries with the same name -- a single term 'x|y' beside
 * the pair ('x', 'y'), or ('x|y', 'z') beside ('x', 'y|z') -- are DI_EFORMAT naming the
 * term: the text route merges them into one vocabulary line (create.py:24-41), this route
 * does not, so build such a collection by the text route.  An id of a pair not below
 * n_terms: DI_EINVAL; more than 2^31 - 1 rows: DI_ERANGE. */
int di_term_table_rows_pairwise(const di_term_table *t, const int64_t *term_count,
                                int64_t n_pair_terms, const uint32_t *first_id,
                                const uint32_t *second_id, int32_t *term_row, int64_t *n_rows);
int di_term_table_destroy(di_term_table *t);

/* ---- device builder: documents as (term id, impact) pairs, e.g. di_encode's device
 * output, to the CSR di_index_create takes ---- */
typedef struct di_index_builder di_index_builder;

#define DI_INDEX_BUILD_TILE 4096 /* pairs / postings one workgroup counts and places */

int di_index_builder_create(int device, di_index_builder **out);
/* Room for n_pairs pairs in all (optional: the pair buffers grow by reallocation). */
int di_index_builder_reserve(di_index_builder *b, int64_t n_docs, int64_t n_pairs);
/* Appends n_docs documents; document d holds (term_ids[i], impacts[i]) for i in
 * [cu_terms[d], cu_terms[d + 1]) and gets doc id *first_doc + d (append order = the line
 * number of the impact TSV).  impacts: the DI_F_ROUND3 values, the ones the TSV holds.
 * Every pair is kept whatever its value (12 bytes: term id, doc, impact), pair i of the
 * call at end + i; a document without a pair is remembered by its doc id.  Arguments and
 * flags as di_sparse_builder_append: with DI_F_DEVICE_PTRS the three arrays are device
 * pointers and only cu_terms is read back.  Runs on hip_stream and waits for it.
 * cu_terms not starting at 0 or decreasing: DI_EINVAL; more than 2^32 - 1 documents in
 * all: DI_ERANGE; after an error the builder is as it was before the call.  An append
 * discards the result of an earlier quantize.  DI_F_TIMING: "ib_append". */
int di_index_builder_append(di_index_builder *b, const uint32_t *term_ids, const float *impacts,
                            const int32_t *cu_terms, int32_t n_docs, int64_t *first_doc,
                            void *hip_stream, uint32_t flags);
/* Appends n_docs documents of the pairwise model (DeepPairwiseImpact.compute_term_impacts,
 * pairwise_impact.py:98-129) from di_encode_pairwise's unrounded outputs: term_ids,
 * single (n_terms entries) and cu_terms as di_index_builder_append takes them, the terms in
 * token order inside a document; pair[n_pairs] and cu_pairs (int64) the pair scores, pair
 * j of a T-term document d being the combination (a < b) at
 * cu_pairs[d] + a(2T - a - 1)/2 + (b - a - 1).  The call applies DI_F_ROUND3's round3 to
 * both.  The singles are appended as di_index_builder_append appends their rounded values;
 * a pair is kept iff its rounded score is not zero (:122) and becomes one record
 * (id(t_a), id(t_b), doc, rounded score), 16 bytes, in document order -- the posting of the
 * term t_a + '|' + t_b (:120-124), whose identity is the pair of ids.  Placement is by
 * tile counts, a scan and ballots: no atomic hands out a slot.  n_pairs of
 * di_index_builder_info counts the singles only.  With DI_F_DEVICE_PTRS the five arrays
 * are device pointers and only cu_terms and cu_pairs are read back.  Runs on hip_stream
 * and waits for it.  cu_terms or cu_pairs not starting at 0 or decreasing, cu_pairs not
 * ending at n_pairs, or a document with cu_pairs[d + 1] - cu_pairs[d] != T(T - 1)/2:
 * DI_EINVAL; more than 2^32 - 1 documents in all: DI_ERANGE; a document without terms is
 * remembered (DI_EFORMAT at quantize) and a non-finite score is reported at quantize, as
 * for di_index_builder_append.  After an error the builder is as it was before the call.
 * An append discards the result of an earlier quantize.  The pair buffers grow by
 * reallocation.  DI_F_TIMING: "ib_append", "ib_pair_append", "ib_scan". */
int di_index_builder_append_pairwise(di_index_builder *b, const uint32_t *term_ids,
                                     const float *single, const float *pair,
                                     const int32_t *cu_terms, const int64_t *cu_pairs,
                                     int32_t n_docs, int64_t n_pairs, int64_t *first_doc,
                                     void *hip_stream, uint32_t flags);
int di_index_builder_info(const di_index_builder *b, int64_t *n_docs, int64_t *n_pairs);
/* quantize_file (quantize.py:13-47) on everything appended: max_val <= 0 means the
 * maximum over all pairs, starting from 0 (:17-24); scale = 255 / max_val in fp64;
 * val = int(double(impact) * scale), truncating (:37-45, di_quantize's arithmetic); a
 * pair is kept iff val > 0 (:46).  term_count[t] (host, n_terms entries) = the kept pairs
 * of term id t; *n_kept = their sum; *max_used = the maximum used.  Errors are the text
 * route's for the same data: a remembered document without a pair (quantize_file raises
 * on its empty line) DI_EFORMAT, naming it; a non-finite impact DI_EFORMAT; maximum 0
 * with no max_val DI_EINVAL, as di_quantize; a value above 255 (struct.pack('B') fails,
 * create.py:45) DI_ERANGE; a term id >= n_terms DI_EINVAL (device-side conditions: an
 * error word read once per step).  After an error the builder is as it was before the
 * call, the result of an earlier quantize included.  May be called again with another
 * max_val: the float impacts stay.  Runs on hip_stream and waits for it.
 * DI_F_TIMING: "ib_quantize", "ib_scan", "ib_compact".
 * On a builder that holds pair records (di_index_builder_append_pairwise) the maximum
 * runs over singles and pairs, the pair records are quantized by the same arithmetic
 * with the same errors (either id >= n_terms: DI_EINVAL), and the kept ones are numbered:
 * a stable radix sort by the key (id_a << 32) | id_b (ceil(bits(n_terms - 1) / 8) passes a
 * half, so a key's records stay in ascending doc order), run heads flagged and scanned,
 * pair number u = the rank of the distinct key.  Pair u is term id n_terms + u of the kept
 * records: *n_kept counts singles and pairs, di_index_builder_postings then takes
 * term_row[n_terms + n_pair_terms], and di_index_builder_pair_terms gives the keys.
 * n_terms + n_pair_terms above 2^31 - 1: DI_ERANGE.  DI_F_TIMING adds "ib_pair_quantize",
 * "ib_pair_compact", "ib_pair_hist", "ib_pair_scatter", "ib_pair_number". */
int di_index_builder_quantize(di_index_builder *b, int64_t n_terms, double max_val,
                              void *hip_stream, uint32_t flags, double *max_used,
                              int64_t *term_count, int64_t *n_kept);
/* The distinct pair keys that kept a posting in the last quantize, in ascending order of
 * (first_id, second_id), and their kept postings: *n_pair_terms, and first_id, second_id,
 * count [n_pair_terms] (host; any of the three may be NULL, e.g. to ask for the size).
 * Before a quantize: DI_EINVAL. */
int di_index_builder_pair_terms(const di_index_builder *b, int64_t *n_pair_terms,
                                uint32_t *first_id, uint32_t *second_id, int64_t *count);
/* The kept postings in the reference file order -- row-major by term_row (host,
 * n_terms entries, -1 = no row), value descending, doc ascending (create.py:41, a stable
 * sort of a doc-ordered list) -- as the input of di_index_create: term_off[n_rows + 1],
 * pdoc[n_kept], pval[n_kept]; host pointers, or device pointers with DI_F_DEVICE_PTRS.
 * A term with kept postings and no row, a row >= n_rows, or two terms on one row:
 * DI_EINVAL.  The builder is left unchanged: the same call gives the same bytes.
 * Runs on hip_stream and waits for it.  DI_F_TIMING: "ib_hist", "ib_scan", "ib_scatter",
 * "ib_extract". */
int di_index_builder_postings(di_index_builder *b, const int32_t *term_row, int64_t n_rows,
                              void *hip_stream, uint32_t flags, int64_t *term_off,
                              uint32_t *pdoc, uint8_t *pval);
int di_index_builder_timing(di_index_builder *b, const char *name, di_timing *out, int reset);
int di_index_builder_destroy(di_index_builder *b);

/* vocab.txt, inverted_index.idx and inverted_index.dat in out_dir from
 * di_index_builder_postings' host arrays and the table's rows: the bytes
 * di_build_reference_index writes for the same collection (create.py:45-51). */
int di_write_reference_index(const char *out_dir, const di_term_table *table,
                             const int32_t *term_row, int64_t n_rows, const int64_t *term_off,
                             const uint32_t *pdoc, const uint8_t *pval);
/* The same with pair terms: term_row[n_terms + n_pair_terms] as
 * di_term_table_rows_pairwise numbers them, and pair u's line of vocab.txt is
 * term[first_id[u]] + '|' + term[second_id[u]].  A row out of range, given twice or
 * without a term, or a pair id not below n_terms: DI_EINVAL. */
int di_write_reference_index_pairwise(const char *out_dir, const di_term_table *table,
                                      int64_t n_pair_terms, const uint32_t *first_id,
                                      const uint32_t *second_id, const int32_t *term_row,
                                      int64_t n_rows, const int64_t *term_off,
                                      const uint32_t *pdoc, const uint8_t *pval);

/* ======================================================================
 * Encoder: DeepImpact forward + first-occurrence gather     (A2, A5-A9)
 * ====================================================================== */
typedef struct di_encoder di_encoder;

#define DI_VARIANT_XLMR 0 /* RoBERTa / XLM-R: positions pad_id+1+i (xlmr_original.py) */
#define DI_VARIANT_BERT 1 /* BERT / CoCondenser: absolute positions (soyuj/deeper-impact) */
#define DI_ACT_SOFTPLUS 0 /* nn.Softplus() head (xlmr_original.py:34-38)               */
#define DI_ACT_RELU 1     /* nn.ReLU() head (original.py:44-47)                        */
#define DI_PREC_BF16 0    /* bf16 MFMA, f32 accumulate/softmax/LayerNorm (fast)        */
#define DI_PREC_FP32 1    /* f32 MFMA throughout (parity with the f32 reference)       */
#define DI_PREC_BF16X3 2  /* fp32-faithful fast mode: split-bf16 GEMMs (3 bf16 MFMA
                             products per f32 product, f32 accumulate), f32 attention
                             and LayerNorm; hidden 768 / 1024                           */
#define DI_DTYPE_F32 0
#define DI_DTYPE_BF16 1

#define DI_F_ROUND3 0x10u        /* di_encode: apply round(impact, 3) (indexer.py:132)  */
#define DI_F_TOKEN_IMPACTS 0x20u /* di_encode: write per-token impacts [n_tokens]       */

typedef struct di_encoder_cfg {
    int32_t variant, activation, precision;
    int32_t vocab_size, hidden, layers, heads, intermediate, max_positions, type_vocab, pad_id;
    float layer_norm_eps;
} di_encoder_cfg;

/* One checkpoint tensor: the reference's state-dict key (ModelCheckpoint layout,
 * src/utils/checkpoint.py:72-77: "bert.embeddings...", "bert.encoder.layer.N...",
 * "impact_score_encoder.0.weight"), host data, row-major. */
typedef struct di_tensor {
    const char *name;
    const void *data;
    int32_t dtype; /* DI_DTYPE_* */
    int32_t ndim;
    int64_t shape[4];
} di_tensor;

/* Replaces DeepImpact.load + .to(cuda).eval() (xlmr_original.py:191-203,
 * indexer.py:22-24).  Strict like load_state_dict (checkpoint.py:117): a missing
 * or unexpected key is DI_EINVAL; "embeddings.position_ids" and "pooler.*" are
 * ignored.  Head dim must be 64; hidden <= 1024.  Optional: the pair head of
 * DeepPairwiseImpact, "pairwise_impact_score_encoder.0.weight" / ".0.bias" (see
 * di_encode_pairwise). */
int di_encoder_create(const di_encoder_cfg *cfg, const di_tensor *weights, int32_t n_weights,
                      int device, di_encoder **out);

/* Replaces DeepImpact.forward (xlmr_original.py:41-85) + compute_term_impacts
 * (:205-225) [+ round(.,3) of indexer.py:132 with DI_F_ROUND3] for a batch.
 * tok_ids: the documents' token ids packed without padding, CSR by
 * cu_seqlens[n_docs+1] (each doc = what the tokenizer emitted incl. <s>/</s>).
 * term_tok[cu_terms[d] .. cu_terms[d+1]): token index (within doc d) of the
 * first token of each kept term, in term order.  out[cu_terms[d] + i] = impact.
 * With DI_F_TOKEN_IMPACTS out[n_tokens] = impact of every token (no gather).
 * n_tokens/max_len/n_terms are required with DI_F_DEVICE_PTRS (no host read of
 * device arrays) and recomputed from the arrays otherwise. */
int di_encode(di_encoder *enc, const int32_t *tok_ids, const int32_t *cu_seqlens, int32_t n_docs,
              int64_t n_tokens, int32_t max_len, const int32_t *term_tok, const int32_t *cu_terms,
              int64_t n_terms, float *out, uint32_t flags);

/* Replaces DeepPairwiseImpact.forward (src/deep_impact/models/pairwise_impact.py:20-95)
 * with pairwise_indices = combinations(sorted(map_.values()), 2) per document -- the
 * call src/deep_impact/indexing/indexer.py:49-54 holds in a comment -- for a batch.
 * The encoder must have been created with the two optional tensors
 * "pairwise_impact_score_encoder.0.weight" [1, 2H+1] and ".0.bias" [1] (one without the
 * other, or a wrong shape, fails di_encoder_create with DI_EINVAL; without them
 * everything else is unchanged) in precision fp32 or bf16x3: a bf16 encoder, or one
 * without the pair head, gets DI_EINVAL here.
 * tok_ids .. n_terms: as di_encode; term_tok must be strictly ascending inside each
 * document (the sorted order), else DI_EINVAL.  cu_pairs[n_docs+1] (int64):
 * cu_pairs[d+1] - cu_pairs[d] = T_d (T_d - 1) / 2 for the T_d terms of document d, else
 * DI_EINVAL; n_pairs is required with DI_F_DEVICE_PTRS (then both checks run on the
 * device and are reported with di_encode's error bits).
 * out_single[n_terms]: exactly what di_encode writes for the same arrays.
 * out_pair[n_pairs]: for the terms a < b (positions within the document's term list)
 *   relu(w[0] attn(a,b) + w[1:H+1] h_a + w[H+1:2H+1] h_b + bias),
 *   attn(a,b) = max over layers of max(mean_h P[h,a,b], mean_h P[h,b,a]),
 * at cu_pairs[d] + a (2 T_d - a - 1) / 2 + (b - a - 1): itertools.combinations order.
 * out_pair_attn[n_pairs] (may be NULL): attn(a,b), the forward's third result.
 * Flags: DI_F_ROUND3 (singles and pairs), DI_F_DEVICE_PTRS, DI_F_ASYNC, DI_F_TIMING
 * ("pair_attn", "pair_score", "pair_prep" beside di_encode's kernels).  Limits
 * (DI_ERANGE): documents of up to 1232 tokens -- the LDS of the 16 term rows' score
 * panel, head sums and term columns, sized for T = n terms of the longest document's n
 * tokens: (16 (16 ceil(n / 16) + 4) + 17 n) 4 bytes <= 160 KiB, which 1232 meets and
 * 1233 does not; sum of T_d^2 over the batch <= 2^32. */
int di_encode_pairwise(di_encoder *enc, const int32_t *tok_ids, const int32_t *cu_seqlens,
                       int32_t n_docs, int64_t n_tokens, int32_t max_len,
                       const int32_t *term_tok, const int32_t *cu_terms, int64_t n_terms,
                       const int64_t *cu_pairs, int64_t n_pairs, float *out_single,
                       float *out_pair, float *out_pair_attn /* may be NULL */, uint32_t flags);

/* Entries of one LDS sort of di_pairwise_order (128 KiB of 64-bit keys): a document of up
 * to this many entries is ordered by one workgroup, a longer one in runs of this many
 * that merge passes combine. */
#define DI_PAIR_ORDER_LDS_KEYS 16384
/* Terms per document of di_pairwise_order: a key holds the entry's position in 21 bits
 * and a term's rank in 11 (T (T + 1) / 2 < 2^21).  di_encode_pairwise's own limit of 1232
 * tokens is below it. */
#define DI_PAIR_ORDER_MAX_TERMS 2047

/* Replaces the ordering of DeepPairwiseImpact.compute_term_impacts
 * (src/deep_impact/models/pairwise_impact.py:98-129) for a batch, on the device: per
 * document the entries are its T terms and the pairs whose score does not round to 0.000
 * (fl32(rint(fl32(x * 1000)) / 1000) != 0, the round(impact, 3) of
 * src/deep_impact/indexing/indexer.py:62-68), sorted by raw score descending (-0.0 equals
 * +0.0), equal scores by position: a term's position is its place in the document's map,
 * pair j's is T + j.  NaN scores are outside the contract.
 * single[n_terms], pair[n_pairs], cu_terms[n_docs+1] (int32), cu_pairs[n_docs+1] (int64):
 * di_encode_pairwise's outputs and offsets -- the terms sorted by token index, the pairs
 * in combination order -- checked as that call checks them (DI_EINVAL; n_terms and
 * n_pairs are required with DI_F_DEVICE_PTRS and recomputed otherwise).
 * single_pos[n_terms] (may be NULL = identity): the position in the document's map of its
 * r-th sorted term (the identity for first-occurrence maps; a permutation for bert_legacy
 * maps); a value outside [0, T) is DI_EINVAL.
 * out_cu[n_docs+1]: offsets of the documents' entries.  Entry e: out_first[e] =
 * cu_terms[d] + r, the global index of a sorted term, out_second[e] = -1 for a term, or the
 * two terms of a pair (first < second); out_score[e] its raw score, or the rounded one
 * with DI_F_ROUND3 (the order always uses the raw score).  *n_out (host) = the entries.
 * If they exceed out_cap the call writes out_cu and *n_out, no entry, and returns
 * DI_ERANGE.  Documents of up to DI_PAIR_ORDER_MAX_TERMS terms (DI_ERANGE for host
 * pointers, DI_EINVAL from the device check).  Runs on hip_stream and waits for it. */
int di_pairwise_order(const float *single, const float *pair, const int32_t *cu_terms,
                      const int64_t *cu_pairs, const int32_t *single_pos /* may be NULL */,
                      int32_t n_docs, int64_t n_terms, int64_t n_pairs, int64_t *out_cu,
                      int32_t *out_first, int32_t *out_second, float *out_score,
                      int64_t out_cap, int64_t *n_out, int device, void *hip_stream,
                      uint32_t flags);

/* di_encode_pairwise followed by di_pairwise_order on the encoder's stream: the forward
 * runs unrounded into the encoder's workspace, the entries are ordered there, and only
 * out_cu and the *n_out entries are copied out -- the pair scores never reach the host.
 * tok_ids .. n_pairs: as di_encode_pairwise; single_pos, out_*: as di_pairwise_order
 * (DI_F_ROUND3 rounds out_score only).  Always synchronous at return.  DI_F_TIMING adds
 * "pair_count", "pair_order" and "pair_merge" to di_encode_pairwise's names. */
int di_encode_pairwise_entries(di_encoder *enc, const int32_t *tok_ids,
                               const int32_t *cu_seqlens, int32_t n_docs, int64_t n_tokens,
                               int32_t max_len, const int32_t *term_tok, const int32_t *cu_terms,
                               int64_t n_terms, const int64_t *cu_pairs, int64_t n_pairs,
                               const int32_t *single_pos /* may be NULL */, int64_t *out_cu,
                               int32_t *out_first, int32_t *out_second, float *out_score,
                               int64_t out_cap, int64_t *n_out, uint32_t flags);
int di_encoder_reserve(di_encoder *enc, int64_t max_tokens, int32_t max_docs, int64_t max_terms);
int di_encoder_set_stream(di_encoder *enc, void *hip_stream);
int di_encoder_sync(di_encoder *enc);
int di_encoder_timing(di_encoder *enc, const char *name, di_timing *out, int reset);
int di_encoder_destroy(di_encoder *enc);

/* ======================================================================
 * Cross-encoder reranking: pairs packed on the device, scored, ranked
 * ====================================================================== */
#define DI_MAX_PAIR_SPECIALS 4 /* special tokens in front of / behind a pair's content */

/* The single-sequence template of the tokenizer's post-processor ("<s> $A </s>",
 * "[CLS] $A [SEP]") and the truncation length of enable_truncation(max_length). */
typedef struct di_pair_format {
    int32_t prefix[DI_MAX_PAIR_SPECIALS];
    int32_t n_prefix;
    int32_t suffix[DI_MAX_PAIR_SPECIALS];
    int32_t n_suffix;
    int32_t max_length;
} di_pair_format;

/* Replaces process_cross_encoder_documents_and_query's encode_batch of
 * f'{document} [SEP] {query}' (src/deep_impact/models/cross_encoder.py:39-51) for a
 * batch of pairs whose two parts were tokenized once each (no special tokens):
 * doc_tok / qry_tok are token stores, CSR by doc_off[n_docs+1] / qry_off[n_q+1];
 * pair p joins passage pair_doc[p] and query part pair_qry[p].  Sequence p =
 * prefix ++ the first max_length - n_prefix - n_suffix tokens of (doc ++ qry) ++
 * suffix -- the tokenizer's right truncation of a single sequence; the cut may fall
 * inside the passage (no query token survives) or inside the query part.
 * Writes tok_ids (capacity tok_cap tokens; n_pairs * max_length always suffices) and
 * cu_seqlens[n_pairs+1] in di_encode's layout, and *n_tokens / *max_len on the host.
 * Host pointers, or device pointers with DI_F_DEVICE_PTRS (fmt, n_tokens and max_len
 * are always host).  Runs on hip_stream and waits for it once, to read the sizes back;
 * with DI_F_DEVICE_PTRS | DI_F_ASYNC the copy into tok_ids is still in flight at
 * return.  A pair index outside its store: DI_EINVAL (an error bit set on the device,
 * as di_encode reports a bad term index); *n_tokens > tok_cap: DI_ERANGE with
 * *n_tokens set. */
int di_pairs_pack(const int32_t *doc_tok, const int64_t *doc_off, int32_t n_docs,
                  const int32_t *qry_tok, const int64_t *qry_off, int32_t n_q,
                  const int32_t *pair_doc, const int32_t *pair_qry, int32_t n_pairs,
                  const di_pair_format *fmt, int32_t *tok_ids, int64_t tok_cap,
                  int32_t *cu_seqlens, int64_t *n_tokens, int32_t *max_len, int device,
                  void *hip_stream, uint32_t flags);

/* Replaces DeepImpactCrossEncoder.forward (src/deep_impact/models/cross_encoder.py:9-23:
 * the impact head on last_hidden_state[:, 0, :]) over the sequences of di_pairs_pack,
 * i.e. one batch step of CrossEncoderReRanker.rerank
 * (src/deep_impact/evaluation/cross_encoder_reranker.py:41-60): packs into the
 * encoder's workspace and runs di_encode's forward with token 0 of every sequence as
 * its only kept row, so the bf16 / bf16x3 pruned last layer computes n_pairs rows.
 * out_scores[n_pairs].  Token-type ids are no input: the reference's forward never
 * passes them on (src/deep_impact/models/original.py:79-84).  max_length <=
 * max_positions.  Flags: DI_F_DEVICE_PTRS, DI_F_ASYNC (the size read-back still waits
 * once), DI_F_TIMING ("pairs_scan", "pairs_copy" beside di_encode's kernels). */
int di_encode_pairs(di_encoder *enc, const int32_t *doc_tok, const int64_t *doc_off,
                    int32_t n_docs, const int32_t *qry_tok, const int64_t *qry_off, int32_t n_q,
                    const int32_t *pair_doc, const int32_t *pair_qry, int32_t n_pairs,
                    const di_pair_format *fmt, float *out_scores, uint32_t flags);

/* Replaces sorted(zip(top_k_pids, scores), key=lambda x: x[1], reverse=True)
 * (src/deep_impact/evaluation/cross_encoder_reranker.py:62) for n_seg queries at once:
 * scores CSR by cu_seg[n_seg+1]; out_pos[cu_seg[s] + r] = the position (within segment
 * s) of its rank-r candidate -- score descending, equal scores in input order (-0.0
 * equals +0.0).  NaN scores are outside the contract.  Segments of up to DI_MAX_TOPK
 * scores; a longer one fails the call with DI_ERANGE (with DI_F_DEVICE_PTRS its out_pos
 * entries are -1).  Waits for hip_stream before returning. */
int di_segment_order(const float *scores, const int32_t *cu_seg, int32_t n_seg, int32_t *out_pos,
                     int device, void *hip_stream, uint32_t flags);

/* ======================================================================
 * Re-ranking with the impact model: a device store of term impacts    (F3)
 * ====================================================================== */
typedef struct di_term_store di_term_store;

/* (term id, impact) pairs of one passage of the store; a longer passage is DI_ERANGE. */
#define DI_TERM_STORE_MAX_TERMS 2048

/* Replaces ReRanker.__init__'s per-pid cache (src/deep_impact/evaluation/reranker.py:13-41):
 * an empty store on `device`.  A handle is not thread-safe.  Every call below runs on the
 * hip_stream it is given and waits for it before returning (the device error word is read
 * back): DI_F_ASYNC is accepted and has no effect. */
int di_term_store_create(int device, di_term_store **out);
/* Capacity for n_docs passages and n_terms pairs in all (never shrinks). */
int di_term_store_reserve(di_term_store *ts, int64_t n_docs, int64_t n_terms);

/* Replaces ReRanker.save (reranker.py:48-50): appends n_docs passages; passage d holds the
 * pairs (term_ids[i], impacts[i]), i in [cu_terms[d], cu_terms[d+1]).  Term ids are whatever
 * the caller assigns to distinct term strings.  *first_doc (host) receives the store index
 * of the first appended passage; the others follow it.  On the device each passage's pairs
 * are kept sorted by term id.  With DI_F_DEVICE_PTRS the three arrays are device pointers
 * (e.g. impacts = the buffer di_encode wrote with DI_F_DEVICE_PTRS: the impacts never visit
 * the host); ordering between the stream that produced them and hip_stream is the
 * caller's business.  An empty passage is legal.  Appending past the reservation grows the
 * buffers; earlier passages keep their indices and contents.
 * Errors, after which nothing is appended and the store is as before: a passage of more
 * than DI_TERM_STORE_MAX_TERMS pairs, DI_ERANGE; cu_terms not starting at 0 or decreasing,
 * DI_EINVAL; the same term id twice in one passage, DI_EINVAL (found on the device after
 * the sort and reported through an error word, as di_encode reports a bad term index).
 * DI_F_TIMING: "ts_sort". */
int di_term_store_append(di_term_store *ts, const uint32_t *term_ids, const float *impacts,
                         const int32_t *cu_terms, int32_t n_docs, int64_t *first_doc,
                         void *hip_stream, uint32_t flags);
/* Passages and pairs held, and the bytes of the two device buffers that hold them. */
int di_term_store_info(const di_term_store *ts, int64_t *n_docs, int64_t *n_terms,
                       int64_t *device_bytes);

/* Replaces ReRanker.score (reranker.py:52-53) for every candidate of n_q queries:
 * q_terms CSR by cu_q[n_q+1] (the query's terms in the iteration order of its Python
 * set), candidates cand_doc[c] (store indices), c in [cu_cand[q], cu_cand[q+1]).  For
 * candidate c of query q: acc = +0.0f; for j in [cu_q[q], cu_q[q+1]) in that order, if
 * passage cand_doc[c] holds q_terms[j], acc = acc + impact -- plain f32 round-to-nearest
 * adds in the query's order, a term that occurs twice adds twice.  out_score[c] = acc,
 * out_match[c] = the number of adds: the reference's sum() is the int 0 (written "0")
 * when nothing matched and a float (written "0.0" even if it is zero) otherwise.
 * Queries of up to DI_MAX_QUERY_TERMS terms (DI_ERANGE).  A candidate index outside the
 * store: DI_EINVAL through the error word; its score and match count are written 0 and
 * nothing is read out of bounds.  Host pointers, or device pointers with DI_F_DEVICE_PTRS
 * (then the limits are checked on the device).  DI_F_TIMING: "ts_score". */
int di_term_store_score(di_term_store *ts, const uint32_t *q_terms, const int32_t *cu_q,
                        int32_t n_q, const int32_t *cand_doc, const int32_t *cu_cand,
                        float *out_score, int32_t *out_match, void *hip_stream, uint32_t flags);
/* HIP-event time of "ts_sort" / "ts_score" over the DI_F_TIMING calls since the last reset. */
int di_term_store_timing(di_term_store *ts, const char *name, di_timing *out, int reset);
int di_term_store_destroy(di_term_store *ts);

/* ======================================================================
 * 8-bit quantizer                                          (A10)
 * ====================================================================== */
/* Replaces quantize_file's arithmetic (src/deep_impact/indexing/quantize.py:13-47):
 * max_val <= 0 means "compute max(0, impacts)"; scale = (2^bits-1)/max_val in
 * fp64; out[i] = int(impacts[i] * scale) (truncation).  impacts are the values
 * the impact TSV holds (3-decimal float32).  *max_used receives the max. */
int di_quantize(const float *impacts, int64_t n, double max_val, int32_t bits, int32_t *out,
                double *max_used, int device, void *hip_stream, uint32_t flags);

/* quantize_file (quantize.py:27-47) end to end: parse the impact TSV exactly as
 * the reference (line.strip().split(', '), t.strip().split(': '), float()),
 * quantize on the GPU in fp64, write the quantized TSV.  Empty / malformed
 * lines fail with DI_EFORMAT where the reference raises ValueError.
 * output_path NULL: only *max_used = the file's max impact (find_max_value,
 * quantize.py:17-24) -- the doc-sharded quantizer all-reduces it (MAX) across ranks. */
int di_quantize_file(const char *input_path, const char *output_path, double max_val,
                     int32_t bits, int device, double *max_used);

/* ======================================================================
 * Impact TSV text                                          (A9)
 * ====================================================================== */
/* Replaces the formatting loop of Indexer.index (indexer.py:62-68): for each doc
 * the terms (UTF-8, terms + term_off[i]..term_off[i+1]) and impacts (already
 * rounded, DI_F_ROUND3) become ', '.join(f'{term}: {impact}') + '\n', numbers
 * printed as Python's repr of the float64 value.  Writes *out_len bytes; returns
 * DI_ERANGE (with *out_len = bytes needed) if out_cap is too small. */
int di_format_impact_lines(const char *terms, const int64_t *term_off, const float *impacts,
                           const int64_t *cu_doc_terms, int32_t n_docs, char *out,
                           int64_t out_cap, int64_t *out_len);

/* The same lines (indexer.py:62-68) for the entries of di_pairwise_order, whose names
 * DeepPairwiseImpact.compute_term_impacts builds (pairwise_impact.py:98-129): entry e of
 * document d (out_cu[d] <= e < out_cu[d+1]) is written as term[first[e]], or
 * term[first[e]] '|' term[second[e]] when second[e] >= 0, then ": " and the repr of the
 * float64 value of score[e]; entries joined by ", ", every document ended by '\n' (a
 * document without entries is "\n").  terms / term_off[n_terms+1]: the batch's terms as
 * in di_format_impact_lines; first / second index them (an index outside [0, n_terms) is
 * DI_EINVAL).  Byte-identical to di_format_impact_lines over the joined names; the same
 * DI_ERANGE contract.  Formatted on DI_HOST_THREADS threads over ranges of documents. */
int di_format_entry_lines(const char *terms, const int64_t *term_off, int64_t n_terms,
                          const int32_t *first, const int32_t *second, const float *score,
                          const int64_t *out_cu, int32_t n_docs, char *out, int64_t out_cap,
                          int64_t *out_len);

/* Replaces RunFile.writelines (src/utils/datasets.py:305-324) over a batch: appends
 * to `path`, for each query q (its id qids[qid_off[q] .. qid_off[q+1]), UTF-8) and rank
 * i < counts[q], "qid\tpid\trank\tscore\n" with pid = docs[q*k + i], rank = i + 1,
 * score = scores[q*k + i] (integers: the quantized index). */
int di_append_run_lines(const char *path, const char *qids, const int64_t *qid_off,
                        int32_t n_q, const uint32_t *docs, const uint32_t *scores,
                        const int32_t *counts, int32_t k);

/* ======================================================================
 * Bench / test data (not a reference interface)
 * ====================================================================== */
/* Seeded MS MARCO-shaped quantized collection (SURVEY §8d generator: per doc the
 * first max_terms unique values of `draws` draws of min(zipf(zipf_a), v_terms),
 * impacts float32(softplus(N(-0.5, 1.5))), round3 + fp64 8-bit quantize, zeros
 * dropped), returned as reference-order postings (term_off[v_terms + 1], then per
 * term value desc / doc asc, create.py:41).  pdoc / pval may be null (sizes only);
 * else cap >= *n_post.  Host threads: DI_HOST_THREADS or OMP_NUM_THREADS. */
int di_synth_postings(int64_t n_docs, int32_t v_terms, uint64_t seed, int32_t max_terms,
                      int32_t draws, double zipf_a, int64_t *term_off, uint32_t *pdoc,
                      uint8_t *pval, int64_t cap, int64_t *n_post, double *max_impact);

/* Skew of a synthetic collection's impacts -- a documented deviation from SURVEY §8d's
 * i.i.d. impacts, for block-max skipping (BASELINE configs[4]): impact =
 * softplus(N(-0.5, 1.5)) x min(1, ((t + 1) / term_rank0)^term_exp) (t = the term's
 * 0-based zipf rank: frequent terms carry small impacts; term_rank0 0 = off) x the doc's
 * mass min(mass_max, exp(cluster_sigma z_c + doc_sigma z_d)) (z_c shared by the
 * cluster_docs consecutive doc ids of a cluster, z_d per doc; mass_max 0 = no clip). */
typedef struct di_synth_skew {
    double term_rank0;
    double term_exp;
    int32_t cluster_docs;
    double cluster_sigma;
    double doc_sigma;
    double mass_max;
} di_synth_skew;

/* di_synth_postings with skewed impacts (skew null: exactly di_synth_postings). */
int di_synth_postings_skewed(int64_t n_docs, int32_t v_terms, uint64_t seed, int32_t max_terms,
                             int32_t draws, double zipf_a, const di_synth_skew *skew,
                             int64_t *term_off, uint32_t *pdoc, uint8_t *pval, int64_t cap,
                             int64_t *n_post, double *max_impact);

/* Docs [doc0, doc0 + n_docs) of the seeded collection di_synth_postings_skewed generates
 * for seed (each doc depends only on (seed, doc id)): one doc-id shard of it, doc ids
 * local (0-based).  quant_max > 0 quantizes with that max (the collection's: the
 * all_reduce(MAX) of the shards' maxima, as the sharded quantize CLI does) instead of the
 * shard's own; term_off null: only *max_impact (the shard's max) is computed.  Bench and
 * test input of the multi-rank retrieve legs. */
int di_synth_postings_shard(int64_t doc0, int64_t n_docs, int32_t v_terms, uint64_t seed,
                            int32_t max_terms, int32_t draws, double zipf_a,
                            const di_synth_skew *skew, double quant_max, int64_t *term_off,
                            uint32_t *pdoc, uint8_t *pval, int64_t cap, int64_t *n_post,
                            double *max_impact);

/* The same seeded collection as the impact TSV of the index CLI (indexer.py:62-68),
 * term id t spelled "\u2581t<t>": bench input of the quantize / index-create legs.
 * *n_terms receives the (doc, term) pairs written. */
int di_synth_impact_tsv(const char *path, int64_t n_docs, int32_t v_terms, uint64_t seed,
                        int32_t max_terms, int32_t draws, double zipf_a, int64_t *n_terms);

/* Decoding of a quantized-index merge key.  A query of at most DI_SHORT_QUERY_TERMS
 * known terms: score(16) | (255 - first term)(8) | its value(8) | ~doc(32).  A longer
 * one (wide key): score(20) | (4095 - first term)(12) | its value(8) | (0xFFFFFF - doc)(24).
 * Within one query every key has the same form and keys order exactly like the
 * reference ranking (score desc, then first touch). */
static inline uint32_t di_key_doc(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
static inline uint32_t di_key_score(uint64_t key) { return (uint32_t)(key >> 48); }
static inline uint32_t di_key_doc_wide(uint64_t key) { return 0xFFFFFFu - (uint32_t)(key & 0xFFFFFFu); }
static inline uint32_t di_key_score_wide(uint64_t key) { return (uint32_t)(key >> 44); }

#ifdef __cplusplus
}
#endif
#endif /* DEEPIMPACT_H */
