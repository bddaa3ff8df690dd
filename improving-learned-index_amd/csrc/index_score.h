// index_score.h -- what the scorer's device code (index_score.hip) shares with the host
// side of the quantized index (index.hip) and with the layout builders: the layout
// constants, the (term, block) tables, the item records, the launch arguments and the
// DI_PROFILE_ABLATE bits.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace di {

constexpr int MAX_BLOCK_DOCS = 32768;  // docs per block (one workgroup's accumulators)
constexpr int SC_THREADS = 1024;
constexpr int SC_WAVES = SC_THREADS / 64;
// Long sublists (>= WLONG_MIN postings in a block) carry a per-wave layout (build pass
// 3): wave w scatters only the docs of its segment.  Queries of at most WTERMS terms
// run every term that way (short terms: every wave reads the sublist, applies its own
// docs); longer ones run the all-wave form, a barrier per term.
constexpr int WSEG = SC_WAVES;
constexpr int WLONG_MIN = 128;  // (1024 / 512 / 256 / 64: within 1%, round 3; 128 vs
                                // 512 in round 4: exhaustive equal, block-max segment bounds
                                // for more terms -- f = 1 skips 0.44 vs 0.30 of the segments
                                // at 8.8 M skewed docs)
constexpr int WTERMS = 64;
constexpr int QH_BINS = 4096;  // per-query candidate-score histogram (shared threshold)
constexpr int BO_MAX_BLOCKS = 1024;  // block_order_kernel ranks by counting in LDS

// Device posting words are ((doc_in_block << 10) | value) XOR POST_X: bits 8-9 stay 0,
// so (word ^ POST_X) >> 8 is the doc's LDS byte address.  A buffer load
// past the descriptor's range returns 0, which decodes to doc MAX_BLOCK_DOCS -- the
// dummy accumulator word after the block -- with value 0: the padding lanes of a
// round need no clamp, no select and no branch (their update lands in the dummy).
// (Per-lane dummy words for the padding, with a quad-wise threshold sweep, measured
// 4.5% slower, profiles/r03pad_scorer_ab.txt; the quad sweep alone neutral,
// profiles/r03quad_scorer_ab.txt.)
constexpr uint32_t POST_X = (uint32_t)MAX_BLOCK_DOCS << 10;

// Packed (block-compressed) postings: frames of up to PK_FRAME postings, PK_PER_LANE
// per lane (the format: index_score.hip, packed_fields).  Short sublists of fewer than
// PK_MIN postings stay in the plain layout (a frame's header and lane rounding would
// cost more than their 4-byte words).
constexpr int PK_FRAME = 512, PK_PER_LANE = 8;
constexpr uint32_t PK_MIN = 32;

// The (term, block) sublists: sparse per term -- the entries of term t are
// [tb_start[t], tb_start[t+1]), one per block holding postings of t, in block order
// (eblk), at postings [epos[e], epos[e+1]); seg[8e + c] = end of impact class c inside
// the sublist; lid[e] = its long id (per-wave layout) or ~0.  A term present in every
// block is indexed directly; otherwise a binary search over its entries' blocks.
struct SubIndex {
    const uint32_t *tb_start;
    const uint16_t *eblk;
    const uint32_t *epos;
    const uint16_t *seg;
    const uint32_t *lid;
    const uint16_t *wmeta;
    const uint8_t *emax;  // block-max metadata: the sublist's largest value
    const uint8_t *wmax;  // long sublists: the largest value of each wave segment's run
    // packed (block-compressed) postings, di_index_set_packed (null: off): frames of
    // entry e = [pk_fs[e], pk_fs[e + 1]); a long entry's run w = frames pk_fs[e] +
    // [pk_fwt[17 lid + w], pk_fwt[17 lid + w + 1])
    const uint32_t *pk_fs;
    const uint16_t *pk_fwt;
    const uint4 *pk_fh;      // frame headers (PackedFrame)
    const uint32_t *pk_data;
};

// Per (item, query term) setup record, resolved for every item in bulk by
// item_setup_kernel before the scorer: the scorer's setup then reads one record per
// (term, wave segment) instead of walking the dependent chain query term -> entry ->
// per-wave runs (several global round trips per item).
struct ItemRec {
    int64_t lo, hi;        // the term's sublist [lo, hi) in this block (min_cls prefix)
    uint32_t wtab[WSEG];   // per-wave layout: run of wave w = start << 16 | end
    uint32_t flags;        // IR_LONG: per-wave layout; IR_BAD: invalid term id
    uint8_t wmx[WSEG];     // block-max bound of each wave segment (emax / wmax)
    uint32_t pad[3];
};
static_assert(sizeof(ItemRec) % 16 == 0, "records stay 16-byte aligned");
constexpr uint32_t IR_LONG = 1, IR_BAD = 2, IR_PLAIN = 4;

// DI_PROFILE_ABLATE (di_index::ablate, ScoreArgs::ablate): profiling and A/B bits.  The
// numeric values are the interface -- tests, tools and the benchmark pass numbers.
// "profiling": the search returns wrong (empty or partial) results, only its timing
// means anything.  "A/B": another route to the same results, bit for bit.
enum : int {
    AB_NO_SCATTER = 1,         // profiling: the scatter loops are skipped
    AB_NO_SELECT = 2,          // profiling: the item ends after the scatter, no candidates
    AB_STOP_AT_KTH = 4,        // profiling: the fast path stops after the k-th score
    AB_STOP_AT_COMPACT = 8,    // profiling: the fast path stops after the compaction
    AB_STAMPS = 64,            // per-phase shader cycles of workgroup 0's items (g_sb_phase);
                               // results unchanged.  launch_score waits for the stream and
                               // prints the cumulative counters after every chunk's
                               // launches, before its merge (not once per search): the
                               // wait falls inside the chunk's "score_blocks" timing
    AB_NO_RECORDS = 1024,      // A/B and the fallback test: no item records -- the scorer
                               // walks the chain query term -> entry -> runs itself (and
                               // the packed layout, which needs records, is off)
    AB_LOAD_B32 = 4096,        // A/B: 4-byte posting loads instead of the 16-byte rounds
    AB_HIST_THRESHOLD = 32768, // A/B: block-max reads the histogram-copy threshold
                               // instead of the running word qtq
    AB_FORCE_EXT_BM = 65536,   // A/B: the block-max instantiation with block-max off (its
                               // code alone)
    AB_NO_SKIP = 131072,       // A/B: block-max evaluates its bounds but skips nothing
    AB_ALL_WAVE = 524288,      // A/B: the all-wave scatter form for every query
    AB_NO_HIST_STAGE = 1048576,// A/B: no staging of candidates in the histogram area
    AB_NO_EMIT_ABOVE = 2097152,// A/B: no emit-above selection for few-block shards
};

// What the scorer's kernels read: by value to score_long_kernel, by reference to the item
// functions.  score_blocks_kernel<EXT> takes the members as separate __restrict__
// parameters in this order (it spills without the qualifier, which a struct cannot
// carry) and rebuilds the struct; launch_score alone unpacks it.  (tq_sched, qtq, kl,
// bm_factor: see score_item.)
struct ScoreArgs {
    const uint32_t *post;  // the posting array this search reads (di_index::post_for)
    SubIndex si;
    int min_cls, nb, block_docs;
    int64_t n_terms;
    uint32_t n_docs, doc_lo;
    const uint32_t *q_terms;  // the chunk's queries: terms of query q =
    const int32_t *cu_q;      // q_terms[cu_q[q] .. cu_q[q + 1])
    int k;
    uint64_t *cand_key;       // [n_q][nb][kl]
    int32_t *cand_n;          // [n_q][nb]: the list's length, < 0: a kernel limit exceeded
    int n_items, n_q;         // n_items = n_q * nb, item = b * n_q + q
    uint32_t *qhist;          // [n_q][QH_BINS] shared-threshold histograms, or null
    int ablate;               // AB_* bits
    ItemRec *rec;             // the items' records, rec_slots per item (item_setup_kernel
                              // writes them, launch_score runs it), or null: no records
    uint32_t *long_flag;      // raised by score_blocks_kernel for score_long_kernel
    float bm_factor;
    unsigned long long *bm_stat;  // {segments evaluated, segments skipped}
    uint16_t *border;         // [n_q][nb] per-query block order (block_order_kernel writes
                              // it, launch_score runs it), or null: blocks in index order
    uint32_t *qtq;            // [n_q] running thresholds, or null
    int rec_slots;
    int kl;                   // capacity of an item's candidate list (>= k)
    int tq_sched;             // first << 16 | every
};

// One chunk's scoring: the block-order kernel (a.border non-null), the record kernel
// (a.rec non-null), score_blocks_kernel<EXT> and score_long_kernel on `stream`.
struct ScoreLaunch {
    ScoreArgs a;
    bool pk, ext, few;     // the instantiation: pk ? EXT_PK : ext ? EXT_BM : few ? EXT_FEW : 0
    hipStream_t stream;
};
void launch_score(const ScoreLaunch &L);

}  // namespace di
