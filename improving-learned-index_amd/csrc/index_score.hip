// index_score.hip -- the quantized inverted-index scorer's device code for MI355X
// (gfx950) and its launcher, launch_score (index_score.h).  The host side of the index
// (the handle, the layout builders, the C ABI) is index.hip; the top-k merge that
// follows every scoring launch is topk_merge.hip.
//
// Replaces InvertedIndex.score (reference src/deep_impact/inverted_index/
// inverted_index.py:31-62) for batches of queries, bit-exact including the
// reference's tie order.
//
// Device layout ("doc-blocked, impact-ordered postings"):
//   docs of a shard are cut into nb = ceil(n_docs / 32768) equal blocks (a multiple
//   of 64 docs each, at most 32768); every term's postings are grouped by block
//   (block-major; inside a block by impact class, bank-dealt).  One posting = one
//   u32: (doc_in_block << 8) | value.  A sparse term -> block table locates the
//   (term, block) sublists (SubIndex).
//
// score_blocks: one 1024-thread workgroup per (query, block) item, persistent.  The
//   block's 32768 accumulators live in LDS (128 KiB), one word per doc
//   score(16) | (255 - j)(8) | v_j(8)  (j = the first query term touching it, v_j its
//   value there): comparing words orders docs exactly like the reference -- score
//   descending, then first-touch order (term order, then impact desc inside that
//   term's list, then doc asc).  Terms are applied in query order; a doc occurs once
//   per term and is updated by one wave (per-wave layout) or between term barriers, so
//   a plain LDS read-modify-write is race free.  Selection: a per-query threshold
//   shared across blocks, a 4096-bin score histogram (<= 16 query terms) or a
//   block-wide radix select.
// score_long: queries of more than 256 terms (64-bit words, wide keys).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdio>
#include <type_traits>

#include "di_common.h"
#include "index_score.h"
#include "topk_common.h"

namespace di {

constexpr int SC_PER_THREAD = MAX_BLOCK_DOCS / SC_THREADS;  // 32 docs per thread in a sweep
constexpr int MAX_TERMS = DI_SHORT_QUERY_TERMS;  // query terms of the compact word
// Fast selection: with at most 16 query terms every score is below 255 * 16 < 4096,
// so one pass of a 4096-bin score histogram finds the k-th score; the docs tied at
// that score (a few, typically) are ordered from a compact list in LDS.
constexpr int FAST_TERMS = 16;
constexpr int HIST_BINS = 4096;
constexpr int TIE_CAP = HIST_BINS;
// Long queries (score_long_item): 64-bit words over half blocks.
constexpr int LONG_TERMS = DI_MAX_QUERY_TERMS;
constexpr int LH_DOCS = 16384;
constexpr int LH_PER_THREAD = LH_DOCS / SC_THREADS;  // 16
constexpr int LH_HELD = DI_MAX_TOPK / SC_THREADS;    // 4
static_assert(MAX_BLOCK_DOCS <= 2 * LH_DOCS, "two halves cover a block");
static_assert(LONG_TERMS <= 4096, "12-bit first-touch index");

struct ScoreShared {
    // the block's words score(16) | (255 - j)(8) | v_j(8) (j = the first query term
    // touching the doc, v_j its value there), + 64 per-lane dummy words; a long-query
    // item uses the array as LH_DOCS 64-bit words (score_long_item)
    uint32_t acc[MAX_BLOCK_DOCS + 64];
    union {
        RadixScratch<SC_WAVES> rs;      // general radix path
        uint32_t hist[HIST_BINS + 64];  // fast path: score histogram (+ spare bins), then the tie list
    } u;
    union {
        int64_t bounds[2][MAX_TERMS];  // scatter: sublist [lo, hi) of every query term
        uint32_t h256[256];            // fast path: digit histogram over the tie list
    } v;
    uint32_t wsum[SC_WAVES];
    uint32_t emit;   // output cursor
    uint32_t n_tie;  // tie-list cursor
    uint32_t bad;
    uint32_t thr, above, ties, bin, bin_above;
    uint32_t tq;                   // the query's shared threshold as this item read it
    uint32_t lmask[WTERMS / 32];   // terms (j < WTERMS) with a per-wave layout in this block
    uint32_t pmask[WTERMS / 32];   // packed mode: short terms read from the plain postings
    unsigned long long bm_cnt[2];  // block-max statistics of the workgroup (thread 0)
    uint32_t tqe;                  // block-max: the query's running threshold (qtq) as
                                   // thread 0 read it -- one value for every wave
    uint32_t wub[WSEG];            // block-max: each wave segment's score upper bound
    uint32_t wtab[WTERMS][WSEG];   // their per-wave runs: start << 16 | end (in the sublist)
    uint32_t wstamp[SC_WAVES];     // profiling (AB_STAMPS): each wave's scatter loop
    uint32_t tqn;                  // EXT: a lower bound of the query's k-th score this item
                                   // found (thread 0), raised into qtq after the item
                                   // (last: the fields above keep their alignment)
};
static_assert(offsetof(ScoreShared, acc) == 0, "accumulators at LDS address 0");
static_assert(sizeof(ScoreShared().acc) >= LH_DOCS * sizeof(uint64_t), "half-block words fit");
static_assert(sizeof(RadixScratch<SC_WAVES>) >= (HIST_BINS + 64) * 4,
              "histogram (+ 64 spare bins) overlays the radix scratch");
static_assert(sizeof(ScoreShared().wtab) >= SC_THREADS * 4, "score_long_kernel's query list");

template <class KeyF, class Pred>
__device__ __forceinline__ void score_radix_pass(ScoreShared &sh, int n_local, int shift,
                                                 uint32_t need, KeyF key, Pred pred) {
    radix_clear<SC_THREADS, SC_WAVES>(sh.u.rs);
    __syncthreads();
    RunLen rl;
#pragma unroll 4
    for (int i = 0; i < SC_PER_THREAD; ++i) {
        int idx = i * SC_THREADS + threadIdx.x;
        if (idx < n_local) {
            uint32_t w = sh.acc[idx];
            uint32_t kk = key(w, idx);
            if (pred(w, idx, kk)) rl.add(sh.u.rs, (kk >> shift) & 255u);
        }
    }
    rl.flush(sh.u.rs);
    __syncthreads();
    radix_pick<SC_THREADS, SC_WAVES>(sh.u.rs, need);
}

// Sweep of the block's accumulator words: f(w, idx) for idx < round4(n_local), 4
// consecutive words per lane per ds_read_b128, 4 reads in flight before any is
// used (a read-then-use loop is LDS-latency bound).  Words past the zeroed range
// come as 0; f runs in wave-uniform control flow (it may ballot).
template <class F>
__device__ __forceinline__ void sweep_words(const uint32_t *acc, int n_local, int tid, F f) {
    const uint4 *a4 = reinterpret_cast<const uint4 *>(acc);
    const int n4 = (n_local + 3) >> 2;
    constexpr int G = 4;  // uint4 reads in flight per lane
    for (int i0 = 0; i0 < SC_PER_THREAD / 4; i0 += G) {
        if (i0 * SC_THREADS >= n4) break;  // (uniform)
        uint4 x[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            // q4 < 8192 always lies inside the array: load unconditionally (no branch),
            // then drop what lies past the zeroed range
            const int q4 = (i0 + i) * SC_THREADS + tid;
            const uint4 y = a4[q4];
            x[i].x = q4 < n4 ? y.x : 0u;
            x[i].y = q4 < n4 ? y.y : 0u;
            x[i].z = q4 < n4 ? y.z : 0u;
            x[i].w = q4 < n4 ? y.w : 0u;
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int base = 4 * ((i0 + i) * SC_THREADS + tid);
            f(x[i].x, base);
            f(x[i].y, base + 1);
            f(x[i].z, base + 2);
            f(x[i].w, base + 3);
        }
    }
}

// Block-wide stable compaction over the accumulator words into two lists:
// cls(w, idx) -> bit 0: list A, bit 1: list B.  One counting sweep, one exclusive
// block scan of the packed per-thread counts, one writing sweep calling
// out(list, pos, w, idx) -- no atomics.  Returns the packed totals (A | B << 16;
// each list holds at most 32768).  Ends with a barrier.
template <class Cls, class Out, class St = void (*)(int)>
__device__ __forceinline__ uint32_t compact_words(ScoreShared &sh, int n_local, int tid, Cls cls,
                                                  Out out, St st = nullptr) {
    uint32_t cnt = 0;
    sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int idx) {
        const uint32_t c = cls(w, idx);
        cnt += (c & 1u) + ((c & 2u) << 15);
    });
    if constexpr (!std::is_same<St, void (*)(int)>::value) st(6);
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t incl = wave_prefix_sum(cnt);
    if (lane == 63) sh.wsum[wave] = incl;
    __syncthreads();
    uint32_t base = incl - cnt, total = 0;
    for (int w2 = 0; w2 < SC_WAVES; ++w2) {
        const uint32_t x = sh.wsum[w2];
        if (w2 < wave) base += x;
        total += x;
    }
    uint32_t pa = base & 0xFFFFu, pb = base >> 16;
    if constexpr (!std::is_same<St, void (*)(int)>::value) st(7);
    sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int idx) {
        const uint32_t c = cls(w, idx);
        if (c & 1u) out(0, pa++, w, idx);
        if (c & 2u) out(1, pb++, w, idx);
    });
    __syncthreads();
    return total;
}

// One scatter round over postings p[0 .. min(avail, UU * SC_THREADS)) (lane-
// consecutive, UU per lane; p and avail wave-uniform): all loads first -- buffer loads
// bounds-checked by the hardware, a 32-bit lane offset and no per-posting address
// arithmetic -- then the LDS reads, then the writes.  A doc occurs once per term, so
// the read-modify-write needs no atomics.
//
// wide (UU a multiple of 4): 16-byte loads, lane tid taking the postings 4 tid ..
// 4 tid + 3 of each group of 4 NT -- a quarter of the load instructions (the scatter
// is bound by them).  Any posting -> lane mapping is exact (a doc occurs
// once per term), and a multi-dword buffer load is range-checked per dword, so the
// padding past avail still reads 0.
template <int UU, int NT = SC_THREADS>
__device__ __forceinline__ void scatter_load(const uint32_t *p, int64_t avail, int tid,
                                             uint32_t (&cur)[UU], bool wide = false) {
    const uint64_t pa = reinterpret_cast<uint64_t>(p);
    const uint32_t lo32 = __builtin_amdgcn_readfirstlane((uint32_t)pa);
    const uint32_t hi32 = __builtin_amdgcn_readfirstlane((uint32_t)(pa >> 32));
    const int bytes = __builtin_amdgcn_readfirstlane(
        (int)(min(avail, (int64_t)UU * NT) * 4));
    void *base = reinterpret_cast<void *>(((uint64_t)hi32 << 32) | lo32);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
    if constexpr (UU % 4 == 0) {
        if (wide) {
#pragma unroll
            for (int g = 0; g < UU / 4; ++g) {
                const auto v =
                    __builtin_amdgcn_raw_buffer_load_b128(rsrc, (4 * tid + g * 4 * NT) * 4, 0, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) cur[4 * g + k] = v[k];
            }
            return;
        }
    }
#pragma unroll
    for (int u = 0; u < UU; ++u)
        cur[u] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, (tid + u * NT) * 4, 0, 0);
}
// The word update: touched w + (v << 16), first touch (v << 16) | first_bits | v --
// both one 24-bit multiply-add (v < 256, first_bits = (255 - j) << 8: no carries).
__device__ __forceinline__ uint32_t word_update(uint32_t w, uint32_t v, uint32_t first_bits) {
    const uint32_t t = __umul24(v, 0x10000u) + w;
    const uint32_t f = __umul24(v, 0x10001u) + first_bits;
    return w ? t : f;
}

// FILT (the all-wave form under impact pruning): postings below vmin update the lane's
// dummy word instead.
template <int UU, bool FILT = false>
__device__ __forceinline__ void scatter_apply(uint32_t *acc, const uint32_t (&cur)[UU],
                                              uint32_t first_bits, uint32_t vmin = 0) {
    // LDS byte addresses formed here and the accesses in inline asm (the compiler's own
    // form adds the array's zero base once more per posting); the reads are retired by
    // the explicit wait, the writes by the caller's term barrier / final wait.
    // (acc is the first member of the kernel's only LDS object, the dynamic segment at
    // LDS address 0: score_blocks_kernel checks that once)
    (void)acc;
    uint32_t w[UU], a[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        a[u] = (cur[u] ^ POST_X) >> 8;
        if constexpr (FILT)
            a[u] = (cur[u] & 255u) >= vmin ? a[u] : (uint32_t)(MAX_BLOCK_DOCS + lane_id()) << 2;
        asm volatile("ds_read_b32 %0, %1" : "=v"(w[u]) : "v"(a[u]) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // the compiler sees the asm reads' results as ready at once: redefine them after
    // the wait, and fence the scheduler, so that no use is hoisted above it
#pragma unroll
    for (int u = 0; u < UU; ++u) asm volatile("" : "+v"(w[u]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t v = cur[u] & 255u;
        asm volatile("ds_write_b32 %0, %1" ::"v"(a[u]), "v"(word_update(w[u], v, first_bits))
                     : "memory");
    }
}

// scatter_apply restricted to the docs [dlo, dlo + dn) of one wave (a short term, whose
// sublist every wave reads in full): the other postings (and the padding) update a
// per-lane dummy word past the block instead.  (Exec-masking them off instead measured
// no faster, profiles/r03sc_scorer_ab.txt.)
template <int UU>
__device__ __forceinline__ void scatter_apply_own(const uint32_t (&cur)[UU], uint32_t first_bits,
                                                  uint32_t dlo, uint32_t dn, uint32_t dummy) {
    uint32_t w[UU], a[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t d = (cur[u] ^ POST_X) >> 10;
        a[u] = (d - dlo < dn) ? d << 2 : dummy;
        asm volatile("ds_read_b32 %0, %1" : "=v"(w[u]) : "v"(a[u]) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < UU; ++u) asm volatile("" : "+v"(w[u]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const uint32_t v = cur[u] & 255u;
        asm volatile("ds_write_b32 %0, %1" ::"v"(a[u]), "v"(word_update(w[u], v, first_bits))
                     : "memory");
    }
}

// The histogram crossing.  A thread owns 4 consecutive bins (counts hv, their sum
// `count`) and knows `suffix`, the count of its bins and every bin above them.  Exactly
// one thread holds the crossing suffix >= need > suffix - count: it walks its 4 bins down
// from the suffix sum to the bin e (0..3) where the count from above reaches need, and
// `above` = the count strictly above that bin.  False for every other thread.
__device__ __forceinline__ bool crossing4(uint32_t suffix, uint32_t count, const uint32_t (&hv)[4],
                                          uint32_t need, int &e, uint32_t &above) {
    if (!(suffix >= need && suffix - count < need)) return false;
    above = suffix - count;
    for (e = 3; e > 0; --e) {
        if (above + hv[e] >= need) break;
        above += hv[e];
    }
    return true;
}

// ---------------------------------------------------------------------------
// Packed (block-compressed) postings -- BASELINE configs[4], di_index_set_packed.
// Every run (a short sublist, or one wave segment's run of a long sublist) is sorted
// by doc and cut into frames of up to 512 postings.  Lane L of a frame holds postings
// 8 L .. 8 L + 7 as eight W-bit fields, W = bd + bv rounded up to a multiple of 4
// (<= 24): field = delta | (value - vmin) << bd, delta = doc - the previous posting's
// doc in the frame (0 for the first), W / 4 dwords per lane, lanes back to back (a
// frame of n postings stores ceil(n / 8) lanes).
// Header (uint4): x = data offset (dwords), y = doc_base (the first doc, 16 bits) |
// count << 16 (10 bits) | bd << 26 (5 bits), z = vmin | bv << 8 (4 bits) | W << 12.
// Decoding happens in registers: the eight fields by static shifts, the lane's
// running delta sums, a DPP wave scan for the lanes before it (no LDS crossbar).

template <int W>
__device__ __forceinline__ void packed_fields(const uint32_t *data, uint32_t cnt, int lane,
                                              uint32_t (&f)[8]) {
    constexpr int ND = W / 4;  // dwords per lane
    static_assert(W % 4 == 0 && W >= 4 && W <= 24, "field width");
    const uint64_t pa = reinterpret_cast<uint64_t>(data);
    const uint32_t lo32 = __builtin_amdgcn_readfirstlane((uint32_t)pa);
    const uint32_t hi32 = __builtin_amdgcn_readfirstlane((uint32_t)(pa >> 32));
    void *base = reinterpret_cast<void *>(((uint64_t)hi32 << 32) | lo32);
    // the frame's ceil(cnt / 8) lanes of data (lanes past them read 0)
    const int bytes = __builtin_amdgcn_readfirstlane((int)((cnt + PK_PER_LANE - 1) / PK_PER_LANE) * ND * 4);
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, bytes, 0x00020000);
    const int off = lane * ND * 4;
    uint32_t d[ND + 1];
    if constexpr (ND == 1) {
        d[0] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
    } else if constexpr (ND == 2) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
        d[0] = v[0], d[1] = v[1];
    } else if constexpr (ND == 3) {
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rsrc, off, 0, 0);
        d[0] = v[0], d[1] = v[1], d[2] = v[2];
    } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0);
        d[0] = v[0], d[1] = v[1], d[2] = v[2], d[3] = v[3];
        if constexpr (ND == 5) {
            d[4] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 16, 0, 0);
        } else if constexpr (ND == 6) {
            const auto u = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off + 16, 0, 0);
            d[4] = u[0], d[5] = u[1];
        }
    }
    d[ND] = 0;
    constexpr uint32_t mask = (1u << W) - 1u;
#pragma unroll
    for (int i = 0; i < PK_PER_LANE; ++i) {
        const int bit = i * W, k = bit >> 5, sft = bit & 31;
        if (sft + W <= 32)
            f[i] = (d[k] >> sft) & mask;
        else
            f[i] = __builtin_amdgcn_alignbit(d[k + 1], d[k], (uint32_t)sft) & mask;
    }
}

// One frame applied to the block's words (the read-modify-write of scatter_apply);
// OWN: only the docs [dlo, dlo + dn) (the wave's own segment), the rest to the lane's
// dummy word.
template <int W, bool OWN>
__device__ __forceinline__ void packed_apply_w(const uint4 h, const uint32_t *__restrict__ pdata,
                                               int lane, uint32_t first_bits, uint32_t dlo,
                                               uint32_t dn, uint32_t dummy) {
    uint32_t f[PK_PER_LANE];
    const uint32_t base = h.y & 0xFFFFu, cnt = (h.y >> 16) & 1023u, bd = (h.y >> 26) & 31u;
    packed_fields<W>(pdata + h.x, cnt, lane, f);
    const uint32_t vmin = h.z & 255u, bv = (h.z >> 8) & 15u;
    uint32_t run = 0, ds[PK_PER_LANE];
#pragma unroll
    for (int i = 0; i < PK_PER_LANE; ++i) {
        run += __builtin_amdgcn_ubfe(f[i], 0, bd);
        ds[i] = run;
    }
    const uint32_t first = base + wave_incl_scan_dpp(run) - run;  // doc before this lane's
    uint32_t w[PK_PER_LANE], a[PK_PER_LANE];
#pragma unroll
    for (int i = 0; i < PK_PER_LANE; ++i) {
        const uint32_t d = first + ds[i];
        bool ok = (uint32_t)(PK_PER_LANE * lane + i) < cnt;
        if constexpr (OWN) ok = ok && d - dlo < dn;  // (the wave's own docs only)
        a[i] = ok ? d << 2 : dummy;
        asm volatile("ds_read_b32 %0, %1" : "=v"(w[i]) : "v"(a[i]) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < PK_PER_LANE; ++i) asm volatile("" : "+v"(w[i]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < PK_PER_LANE; ++i) {
        const uint32_t v = vmin + __builtin_amdgcn_ubfe(f[i], bd, bv);
        asm volatile("ds_write_b32 %0, %1" ::"v"(a[i]), "v"(word_update(w[i], v, first_bits))
                     : "memory");
    }
}

template <bool OWN>
__device__ __forceinline__ void packed_apply(const uint4 h, const uint32_t *__restrict__ pdata,
                                             int lane, uint32_t first_bits, uint32_t dlo,
                                             uint32_t dn, uint32_t dummy) {
    switch ((h.z >> 12) & 63u) {  // (wave-uniform)
    case 4: packed_apply_w<4, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    case 8: packed_apply_w<8, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    case 12: packed_apply_w<12, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    case 16: packed_apply_w<16, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    case 20: packed_apply_w<20, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    default: packed_apply_w<24, OWN>(h, pdata, lane, first_bits, dlo, dn, dummy); break;
    }
}

// Profiling (AB_STAMPS): per-phase shader cycles of workgroup 0's items
// accumulated here and printed by launch_score.
__device__ unsigned long long g_sb_phase[12];  // [9] slowest wave's scatter loop, [10] mean

// entry of (term t, block b), or -1 when t has no posting in b
__device__ __forceinline__ int64_t find_entry(const SubIndex &si, int nb, uint32_t t, int b) {
    const uint32_t e0 = si.tb_start[t], e1 = si.tb_start[t + 1];
    if (e1 - e0 == (uint32_t)nb) return (int64_t)e0 + b;
    uint32_t lo = e0, hi = e1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (si.eblk[mid] < (uint32_t)b) lo = mid + 1;
        else hi = mid;
    }
    return lo < e1 && si.eblk[lo] == (uint32_t)b ? (int64_t)lo : -1;
}

// [lo, hi) of entry e scored at impact-class prefix min_cls (7: the whole sublist)
__device__ __forceinline__ void entry_bounds(const SubIndex &si, int64_t e, int min_cls,
                                             int64_t &lo, int64_t &hi) {
    if (e < 0) {
        lo = hi = 0;
        return;
    }
    lo = si.epos[e];
    hi = min_cls >= 7 ? (int64_t)si.epos[e + 1] : lo + si.seg[e * 8 + min_cls];
}

// Items (query q, block b) as the scorer numbers them (item = b * n_q + q); records
// only for queries of 1..WTERMS terms (the scorer's per-wave form), rec_slots per item
// (the batch's longest such query).
__global__ void __launch_bounds__(128)
item_setup_kernel(SubIndex si, int min_cls, int nb, int64_t n_terms,
                  const uint32_t *__restrict__ q_terms, const int32_t *__restrict__ cu_q, int n_q,
                  ItemRec *__restrict__ rec, const uint16_t *__restrict__ border, int rec_slots) {
    const int item = blockIdx.x, q = item % n_q, r_ = item / n_q;
    const int b = border ? (int)border[(int64_t)q * nb + r_] : r_;
    const int q0 = cu_q[q], nt = cu_q[q + 1] - q0;
    if (nt > rec_slots || nt <= 0) return;  // (rec_slots >= every per-wave query's terms)
    ItemRec *r = rec + (int64_t)item * rec_slots;
    for (int e = threadIdx.x; e < nt * WSEG; e += blockDim.x) {
        const int j = e / WSEG, w = e % WSEG;
        const uint32_t t = q_terms[q0 + j];
        if (t >= n_terms) {  // invalid id (device-pointer callers are not pre-checked)
            if (w == 0) {
                r[j].lo = r[j].hi = 0;
                r[j].flags = IR_BAD;
            }
            continue;
        }
        const int64_t en = find_entry(si, nb, t, b);
        const uint32_t id = en >= 0 ? si.lid[en] : 0xFFFFFFFFu;
        if (w == 0) {
            int64_t lo, hi;
            uint32_t fl = id != 0xFFFFFFFFu ? IR_LONG : 0u;
            if (si.pk_fs && en >= 0 && (id != 0xFFFFFFFFu || si.epos[en + 1] - si.epos[en] >= PK_MIN)) {
                // packed: frame ranges (exact scoring only, min_cls 7)
                lo = si.pk_fs[en];
                hi = si.pk_fs[en + 1];
            } else {
                entry_bounds(si, en, min_cls, lo, hi);
                if (si.pk_fs) fl |= IR_PLAIN;
            }
            r[j].lo = lo;
            r[j].hi = hi;
            r[j].flags = fl;
        }
        r[j].wmx[w] = en < 0 ? 0 : id != 0xFFFFFFFFu ? si.wmax[(int64_t)id * WSEG + w] : si.emax[en];
        if (id != 0xFFFFFFFFu) {
            if (si.pk_fs) {
                const uint16_t *m = si.pk_fwt + (int64_t)id * (WSEG + 1);
                r[j].wtab[w] = ((uint32_t)m[w] << 16) | m[w + 1];
            } else {
                const uint16_t *m = si.wmeta + (int64_t)id * (WSEG * 8);
                const uint32_t s0 = w ? m[(w - 1) * 8 + 7] : 0u;
                r[j].wtab[w] = (s0 << 16) | m[w * 8 + min(min_cls, 7)];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Long queries: DI_SHORT_QUERY_TERMS < known terms <= DI_MAX_QUERY_TERMS.  The packed
// score does not hold their sums (255 x 4096 > 2^16) nor the key their first-touch index
// (> 255), so an item (query, block) of such a query accumulates 64-bit words
//     score(20) | (4095 - j)(12) | v_j(8)                       (bits 39..0)
// -- ordered exactly like the short word: score, then first touch -- over half blocks
// of LH_DOCS docs (128 KiB of LDS, the accumulators of ScoreShared), and its candidates
// carry the wide merge key  word << 24 | (0xFFFFFF - doc)  (docs < 2^24).  The first
// half's candidates wait in the item's output list; the second half's selection runs
// over the union (the waiting keys held in registers, LH_HELD per thread) and rewrites
// the list, so a long item emits one list of <= k keys like a short one and the merge
// is unchanged (it decodes wide keys per query, see merge_topk_kernel).  Terms go in
// chunks of MAX_TERMS bounds, a barrier per term.  Rare (no MS MARCO query comes close),
// so simple: one posting per lane per load, a read-modify-write per posting.
__device__ __forceinline__ void score_long_item(ScoreShared &sh, int q, int b, const ScoreArgs &a) {
    const uint32_t *__restrict__ post = a.post;
    const SubIndex &si = a.si;
    const int min_cls = a.min_cls, nb = a.nb, block_docs = a.block_docs, k = a.k;
    const int64_t n_terms = a.n_terms;
    const uint32_t n_docs = a.n_docs, doc_lo = a.doc_lo;
    const uint32_t *__restrict__ q_terms = a.q_terms;
    const int32_t *__restrict__ cu_q = a.cu_q;
    uint64_t *__restrict__ ck = a.cand_key + ((int64_t)q * nb + b) * a.kl;
    int32_t *__restrict__ cn = a.cand_n + (int64_t)q * nb + b;
    uint64_t *acc = reinterpret_cast<uint64_t *>(sh.acc);
    int64_t *lo = sh.v.bounds[0], *hi = sh.v.bounds[1];
    const int tid = threadIdx.x;
    const int64_t block_first = (int64_t)b * block_docs;
    const int n_local = (int)min((int64_t)block_docs, (int64_t)n_docs - block_first);
    const int q0 = cu_q[q], nt = cu_q[q + 1] - q0;
    if (n_local <= 0) {
        if (tid == 0) *cn = 0;
        return;
    }
    if ((uint64_t)doc_lo + n_docs > (1ull << 24)) {  // the wide key holds 24-bit docs
        if (tid == 0) *cn = -1;
        return;
    }
    const uint32_t vmin = 1u << (7 - min(min_cls, 7));  // impact pruning: values >= vmin
    uint64_t held[LH_HELD] = {0, 0, 0, 0};
    uint32_t n_held = 0;
    for (int hb = 0; hb < n_local; hb += LH_DOCS) {
        const int hn = min(LH_DOCS, n_local - hb);
        const uint32_t gbase = doc_lo + (uint32_t)(block_first + hb);
        {
            uint4 *a4 = reinterpret_cast<uint4 *>(acc);
            for (int i = tid; i < (hn + 1) / 2; i += SC_THREADS) a4[i] = make_uint4(0, 0, 0, 0);
        }
        if (tid == 0) sh.bad = 0;
        for (int c0 = 0; c0 < nt; c0 += MAX_TERMS) {
            const int cnt = min(MAX_TERMS, nt - c0);
            __syncthreads();  // zeroing done / the previous chunk's bounds no longer read
            for (int j = tid; j < cnt; j += SC_THREADS) {
                const uint32_t t = q_terms[q0 + c0 + j];
                if (t >= n_terms) {
                    sh.bad = 1;
                    lo[j] = hi[j] = 0;
                    continue;
                }
                // the whole sublist: a long sublist is laid out per wave segment (classes
                // in order inside each), so the class prefix is not one range -- pruning
                // (min_cls < 7) filters by value in the scatter instead
                entry_bounds(si, find_entry(si, nb, t, b), 7, lo[j], hi[j]);
            }
            __syncthreads();
            if (sh.bad) {
                if (tid == 0) *cn = -1;
                return;
            }
            for (int jj = 0; jj < cnt; ++jj) {
                const uint64_t fb = (uint64_t)(4095 - (c0 + jj)) << 8;
                const int64_t L = lo[jj], H = hi[jj];
                for (int64_t p0 = L; p0 < H; p0 += 4 * SC_THREADS) {
                    uint32_t r[4];
                    scatter_load<4>(post + p0, H - p0, tid, r);  // past the end: doc 32768, v 0
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t d = ((r[u] ^ POST_X) >> 10) - (uint32_t)hb;
                        const uint64_t v = r[u] & 255u;
                        if (d < (uint32_t)hn && v >= vmin) {  // a doc occurs once per term
                            const uint64_t w = acc[d];
                            acc[d] = w ? w + (v << 20) : (v << 20) | fb | v;
                        }
                    }
                }
                __syncthreads();  // term boundary
            }
        }
        // ---- selection over this half's touched words + the held keys -------------
        auto key_of = [&](uint64_t w, int idx) {
            return (w << 24) | (uint64_t)(0xFFFFFFu - (gbase + (uint32_t)idx));
        };
        uint64_t prefix = 0, mask = 0;
        uint32_t need = (uint32_t)k;
        for (int shift = 56; shift >= 0; shift -= 8) {
            radix_clear<SC_THREADS, SC_WAVES>(sh.u.rs);
            __syncthreads();
            RunLen rl;
            for (int i = 0; i < LH_PER_THREAD; ++i) {
                const int idx = i * SC_THREADS + tid;
                const uint64_t w = idx < hn ? acc[idx] : 0ull;
                if (w) {
                    const uint64_t x = key_of(w, idx);
                    if ((x & mask) == prefix) rl.add(sh.u.rs, (uint32_t)(x >> shift) & 255u);
                }
            }
#pragma unroll
            for (int i = 0; i < LH_HELD; ++i)
                if ((uint32_t)(i * SC_THREADS + tid) < n_held && (held[i] & mask) == prefix)
                    rl.add(sh.u.rs, (uint32_t)(held[i] >> shift) & 255u);
            rl.flush(sh.u.rs);
            __syncthreads();
            radix_pick<SC_THREADS, SC_WAVES>(sh.u.rs, need);
            if (shift == 56 && sh.u.rs.total <= (uint32_t)k) {  // every key is a candidate
                prefix = 0;
                break;
            }
            prefix |= (uint64_t)sh.u.rs.bin << shift;
            mask |= (uint64_t)255 << shift;
            need -= sh.u.rs.above;
        }
        // keys are unique: the keys >= prefix are exactly min(k, total) (prefix = the
        // k-th largest key, or 0 when there are at most k)
        if (tid == 0) sh.emit = 0;
        __syncthreads();
        for (int i = 0; i < LH_PER_THREAD; ++i) {
            const int idx = i * SC_THREADS + tid;
            const uint64_t w = idx < hn ? acc[idx] : 0ull;
            const uint64_t x = w ? key_of(w, idx) : 0ull;
            uint32_t pos;
            if (wave_append(w != 0 && x >= prefix, &sh.emit, pos) && pos < (uint32_t)k) ck[pos] = x;
        }
#pragma unroll
        for (int i = 0; i < LH_HELD; ++i) {
            const bool ok = (uint32_t)(i * SC_THREADS + tid) < n_held && held[i] >= prefix;
            uint32_t pos;
            if (wave_append(ok, &sh.emit, pos) && pos < (uint32_t)k) ck[pos] = held[i];
        }
        __syncthreads();
        n_held = min(sh.emit, (uint32_t)k);
        if (hb + LH_DOCS < n_local) {  // the next half: hold this list (written above)
#pragma unroll
            for (int i = 0; i < LH_HELD; ++i) {
                const uint32_t p = (uint32_t)(i * SC_THREADS + tid);
                held[i] = p < n_held ? ck[p] : 0ull;
            }
        }
        __syncthreads();  // the list is held before the next selection rewrites it
    }
    if (tid == 0) *cn = (int32_t)n_held;
}

// One work item = (query q, doc block b): accumulate, select the block's top-k.
// EXT: the configs[4] extensions -- 0 none (the plain scorer: its code and registers
// stay exactly as without them), EXT_BM block-max skipping over the plain postings
// (bm_factor, per-query block order, the cooperative form), EXT_PK the packed postings
// (si.pk_fs; with or without block-max) -- one kernel each.
constexpr int EXT_BM = 1, EXT_PK = 2, EXT_FEW = 4;  // (EXT_FEW: the emit-above selection of
                                                   // few-block shards, its own kernel so
                                                   // the plain one keeps its code)
template <int EXT>
__device__ __forceinline__ void score_item(ScoreShared &sh, int q, int b, const ScoreArgs &a,
                                           const ItemRec *__restrict__ ir) {
    const uint32_t *__restrict__ post = a.post;
    const SubIndex &si = a.si;
    const int min_cls = a.min_cls, nb = a.nb, block_docs = a.block_docs, k = a.k, kl = a.kl;
    const int64_t n_terms = a.n_terms;
    const uint32_t n_docs = a.n_docs, doc_lo = a.doc_lo;
    const uint32_t *__restrict__ q_terms = a.q_terms;
    const int32_t *__restrict__ cu_q = a.cu_q;
    uint32_t *__restrict__ qhist = a.qhist, *__restrict__ qtq = a.qtq;
    const int ablate = a.ablate, tq_sched = a.tq_sched;
    const float bm_factor = a.bm_factor;
    int64_t *lo = sh.v.bounds[0], *hi = sh.v.bounds[1];

    // opaque per item: keeps the per-thread index arithmetic of the sweeps from being
    // hoisted out of the persistent item loop (it spilled there)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t block_first = (int64_t)b * block_docs;
    const int n_local = (int)min((int64_t)block_docs, (int64_t)n_docs - block_first);
    const int q0 = cu_q[q], nt = cu_q[q + 1] - q0;
    uint64_t *ck = a.cand_key + ((int64_t)q * nb + b) * kl;
    int32_t *cn = a.cand_n + (int64_t)q * nb + b;

    if (nt > MAX_TERMS && nt <= LONG_TERMS) {  // score_long_kernel's item (it runs next)
        if (tid == 0) {
            *cn = 0;
            *a.long_flag = 1;
        }
        return;
    }
    if (nt > MAX_TERMS || nt < 0 || n_local <= 0) {
        if (tid == 0) *cn = (nt > MAX_TERMS || nt < 0) ? -1 : 0;
        return;
    }
    const bool fast = nt <= FAST_TERMS;
    const bool stamps = (ablate & AB_STAMPS) && blockIdx.x == 0 && tid == 0;
    uint64_t t_prev = stamps ? __builtin_amdgcn_s_memtime() : 0;
    auto stamp = [&](int ph) {
        if (stamps) {
            const uint64_t t = __builtin_amdgcn_s_memtime();
            atomicAdd(&g_sb_phase[ph], (unsigned long long)(t - t_prev));
            t_prev = t;
        }
    };
    if (tid == 0) {
        sh.bad = 0;
        sh.emit = 0;
        sh.n_tie = 0;
        for (int i = 0; i < WTERMS / 32; ++i) sh.lmask[i] = sh.pmask[i] = 0;
        for (int i = 0; i < WSEG; ++i) sh.wub[i] = 0;
        sh.tq = 0;
    }
    __syncthreads();

    // per-wave form (at most WTERMS terms): every term applied by each wave to its own
    // docs -- long terms over their per-wave runs, short ones read in full by every wave
    // -- so no term needs a barrier; longer queries: the all-wave form, a barrier per term
    const bool wl = nt <= WTERMS && !(ablate & AB_ALL_WAVE);
    // block-max skipping (opt-in, configs[4]): per-wave segment upper bounds (wub)
    // (XBM: the block-max / packed instantiations; EXT_FEW is the plain scorer + the
    // emit-above selection, with only the running-threshold bookkeeping of the others)
    constexpr bool XBM = EXT == EXT_BM || EXT == EXT_PK;
    const bool bm = XBM && bm_factor > 0.0f && wl && qhist != nullptr;
    // block-max: the query's running threshold as one word (qtq, raised by every item's
    // selection with a lower bound of the final k-th score), loaded with the setup's
    // loads -- the skip decision needs no histogram copy, no extra barrier
    // (thread 0 alone loads it and publishes it through LDS at the setup barrier: waves
    // that read the word themselves could see different values -- other CUs raise it --
    // and disagree on skipping, i.e. on which barriers they reach)
    // (few blocks, no qhist: the same word bounds the emit-above selection, see below)
    uint32_t tq_early = 0;
    if (qtq && threadIdx.x == 0)
        tq_early = __hip_atomic_load(&qtq[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The query's shared threshold histogram (qhist, below) is copied by LDS-DMA into
    // the selection histogram (idle until the selection) here, so its round trip
    // overlaps the scatter and the selection reads it from LDS; the fast selection
    // path zeroes the histogram itself when it runs.
    uint32_t *qh = qhist ? qhist + (int64_t)q * QH_BINS : nullptr;
    // Threshold refresh schedule (tq_sched = first << 16 | every; plain exact scoring with
    // the running word qtq): only the items of blocks b < first and b % every == 0 copy
    // and read the histogram (and raise qtq with the Tq it gives); the others take qtq,
    // one word read with the setup loads -- no 16 KiB copy to wait for, no threshold read.
    // qtq only ever holds lower bounds of the final k-th score, so any schedule is exact.
    const int tq_every = tq_sched & 0xFFFF, tq_first = tq_sched >> 16;
    const bool qpre = qh != nullptr &&
                      (!qtq || tq_every <= 1 || b < tq_first || b % tq_every == 0);
    static_assert(QH_BINS == 4 * SC_THREADS && QH_BINS <= HIST_BINS, "qhist prefetch");
    if (qpre) {
        typedef __attribute__((address_space(3))) void lds_void;
        __builtin_amdgcn_global_load_lds((const void *)(qh + 4 * tid),
                                         (lds_void *)(sh.u.hist + wave * 256), 16, 0, 0);
    }
    // zeroing of the accumulators (and the fast path's histogram): LDS stores only,
    // placed where the setup's global loads are in flight
    auto zero = [&]() {
        uint4 *a4 = reinterpret_cast<uint4 *>(sh.acc);
        const int n4 = (n_local + 3) >> 2;
        for (int i = tid; i < n4; i += SC_THREADS) a4[i] = make_uint4(0, 0, 0, 0);
        if (fast && !qpre) reinterpret_cast<uint4 *>(sh.u.hist)[tid] = make_uint4(0, 0, 0, 0);
        // (the 64 spare bins past them are written, never read: no zeroing needed)
    };
    if (wl && ir != nullptr) {
        // the item's records (item_setup_kernel): one (term j, wave segment w) per thread
        const int e = tid;
        const bool act = e < nt * WSEG;
        const int j = act ? e / WSEG : 0, w = e % WSEG;
        uint32_t f = 0, wt = 0, ub = 0;
        int64_t rlo = 0, rhi = 0;
        if (act) {
            const ItemRec &R = ir[j];
            f = R.flags;
            wt = R.wtab[w];
            if (bm) ub = R.wmx[w];
            if (w == 0) {
                rlo = R.lo;
                rhi = R.hi;
            }
        }
        zero();
        if (act) {
            if (bm && ub) atomicAdd(&sh.wub[w], ub);
            if (w == 0) {
                lo[j] = rlo;
                hi[j] = rhi;
                if (f & IR_BAD) sh.bad = 1;
                if (f & IR_LONG) atomicOr(&sh.lmask[j >> 5], 1u << (j & 31));
                if (EXT == EXT_PK && (f & IR_PLAIN)) atomicOr(&sh.pmask[j >> 5], 1u << (j & 31));
            }
            if (f & IR_LONG) sh.wtab[j][w] = wt;
        }
    } else if (wl) {
        // nt * WSEG <= SC_THREADS: one (term j, wave segment w) per thread.  The entry
        // lookup and the loads that depend on it (bounds, long id) are issued, the
        // accumulators zeroed while they are in flight, then the per-wave runs read.
        static_assert(WTERMS * WSEG <= SC_THREADS, "one setup entry per thread");
        const int e = tid;
        const bool act = e < nt * WSEG;
        const int j = act ? e / WSEG : 0, w = e % WSEG;
        const uint32_t t = act ? q_terms[q0 + j] : 0u;
        const bool tok = act && t < n_terms;  // (device-pointer callers are not pre-checked)
        int64_t en = -1, blo = 0, bhi = 0;
        uint32_t id = 0xFFFFFFFFu, ub = 0;
        if (tok) {
            en = find_entry(si, nb, t, b);
            if (en >= 0) id = si.lid[en];
            if (w == 0) entry_bounds(si, en, min_cls, blo, bhi);
            if (bm && en >= 0)
                ub = id != 0xFFFFFFFFu ? si.wmax[(int64_t)id * WSEG + w] : si.emax[en];
        }
        zero();
        if (bm && ub) atomicAdd(&sh.wub[w], ub);
        if (act && !tok) {  // invalid term id
            if (w == 0) {
                sh.bad = 1;
                lo[j] = hi[j] = 0;
            }
        } else if (act) {
            if (w == 0) {
                lo[j] = blo;
                hi[j] = bhi;
            }
            if (id != 0xFFFFFFFFu) {
                const uint16_t *m = si.wmeta + (int64_t)id * (WSEG * 8);
                const uint32_t s0 = w ? m[(w - 1) * 8 + 7] : 0u;
                sh.wtab[j][w] = (s0 << 16) | m[w * 8 + min(min_cls, 7)];
                if (w == 0) atomicOr(&sh.lmask[j >> 5], 1u << (j & 31));
            }
        }
    } else {
        // all-wave form: whole sublists (a long one is laid out per wave segment, so its
        // class prefix is not one range); impact pruning filters by value (vmin below)
        for (int j = tid; j < nt; j += SC_THREADS) {
            const uint32_t t = q_terms[q0 + j];
            if (t >= n_terms) {
                sh.bad = 1;
                lo[j] = hi[j] = 0;
                continue;
            }
            entry_bounds(si, find_entry(si, nb, t, b), 7, lo[j], hi[j]);
        }
        zero();
    }
    if (qtq && tid == 0) sh.tqe = tq_early;
    __syncthreads();
    if (sh.bad) {
        // (the histogram copy lands before the next item touches the histogram)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) *cn = -1;
        return;
    }

    stamp(0);  // setup + zeroing
    const bool wstamps = (ablate & AB_STAMPS) && blockIdx.x == 0;
    const uint64_t t_w0 = wstamps ? __builtin_amdgcn_s_memtime() : 0;
    // The query's shared threshold (qhist, when given) counts the scores of every
    // candidate its finished blocks emitted (distinct docs, full scores; bin 4095 =
    // 4095 and above).  read_tq -> the largest s with >= k counted candidates scoring
    // >= s: at least k docs score >= s, so the final k-th score is >= s.  A stale
    // (smaller) count still gives a valid lower bound.  Block-wide (barriers).
    auto read_tq = [&]() -> uint32_t {
        // thread t: bins 4t..4t+3 (relaxed atomic loads: other CUs add to them; or the
        // LDS copy made at the item's start)
        uint32_t hv[4], c = 0;
        if (qpre) {
            const uint4 h = reinterpret_cast<const uint4 *>(sh.u.hist)[tid];
            hv[0] = h.x, hv[1] = h.y, hv[2] = h.z, hv[3] = h.w;
            c = h.x + h.y + h.z + h.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                c += (hv[e] = __hip_atomic_load(&qh[4 * tid + e], __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT));
        }
        uint32_t sfx = wave_suffix_sum(c);
        if (lane == 0) sh.wsum[wave] = sfx;
        if (tid == 0) sh.tq = 0;
        __syncthreads();
        for (int w2 = wave + 1; w2 < SC_WAVES; ++w2) sfx += sh.wsum[w2];
        // one thread holds the crossing: count(>= 4t + e) >= k > count(>= 4t + e + 1)
        int e;
        uint32_t above;
        if (crossing4(sfx, c, hv, (uint32_t)k, e, above)) sh.tq = (uint32_t)(4 * tid + e);
        __syncthreads();
        const uint32_t r = sh.tq;
        __syncthreads();  // (wsum / tq are reused)
        return r;
    };
    // Block-max skipping (bm, opt-in; configs[4]): a wave segment whose upper bound
    // wub = sum over the query terms of the segment's largest value in their sublists
    // stays below the query's shared threshold Tq cannot hold a top-k doc (every doc of
    // it scores <= wub < Tq <= the final k-th score): its wave skips its scatter and its
    // docs stay 0.  bm_factor 1 is exact; > 1 skips segments below factor x Tq -- an
    // approximation (the QPS-vs-recall sweep).  Every segment below: the item ends.
    bool skip_wave = false;
    uint32_t live16 = 0xFFFFu;  // bm: the wave segments that are scored (bit w)
    if (bm) {
        uint32_t tq0;
        if (qtq) {
            tq0 = sh.tqe;  // (written before the setup barrier)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the threshold copy (read_tq)
            tq0 = read_tq();
        }
        const float thr = bm_factor * (float)tq0;
        skip_wave = tq0 > 0 && (float)sh.wub[wave] < thr && !(ablate & AB_NO_SKIP);
        // every segment below: lanes 0..15 of each wave check one each (no block
        // reduction: __syncthreads_and would take static LDS, and the scatter needs the
        // dynamic segment at address 0)
        static_assert(WSEG <= 64, "one lane per segment");
        const bool below = lane >= WSEG || (tq0 > 0 && (float)sh.wub[lane] < thr);
        const uint64_t below_m = __ballot(below);
        const bool all_below = below_m == ~0ull && !(ablate & AB_NO_SKIP);
        live16 = (uint32_t)~below_m & 0xFFFFu;
        // skip statistics (di_index_timing "bm_segments" / "bm_segments_skipped"): every
        // evaluated item counts its WSEG segments, every skipped segment one -- in the
        // workgroup's LDS, added to the device counters once per workgroup at the kernel's
        // end (an atomic per item and skipping wave on one address cost tens of ms per
        // 8.8 M-doc batch)
        if (tid == 0) {
            sh.bm_cnt[0] += WSEG;
            sh.bm_cnt[1] += (unsigned long long)__builtin_popcount(~live16 & 0xFFFFu);
        }
        if (all_below) {
            // the item's threshold-histogram copy (LDS-DMA into sh.u.hist) lands before
            // the next item uses that LDS (it would overwrite the next query's copy)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 0) *cn = 0;
            return;
        }
    }
    // ---- scatter: terms in query order, barrier between terms -------------
    // A term's sublist goes in rounds of 16 postings per lane while 16 k remain, then
    // 4 per lane while more than 1 k remain, then 1: a short tail does not pay for a
    // full round of issue (loads, LDS reads and writes of masked lanes).  Each round
    // has all its loads in flight before any is applied; the 16 waves of the CU
    // overlap one another's load latency with their LDS work.
    // The last round of a term also loads the next term's first 4 k postings, before
    // the term barrier (a raw one: LDS writes retired, loads left in flight), so the
    // barrier does not expose a load round trip per term.
    // A long term (per-wave layout) is scattered by each wave over its own doc segment,
    // rounds of up to 16 postings per lane: no other wave touches those docs, so a run
    // of long terms needs no barrier between its terms, only at its ends.
    uint32_t pre[4];
    bool have_pre = false;
    auto is_long = [&](int j) { return wl && ((sh.lmask[j >> 5] >> (j & 31)) & 1u); };
    const uint32_t wseg = ((uint32_t)block_docs + WSEG - 1) / WSEG;
    // (A cooperative form -- every wave on every scored segment, barriers between terms,
    // so that a skipped segment's wave does not idle -- measured no faster at 8.8 M skewed
    // docs, 45.8 k vs 46.3 k q/s, and was removed; round-4 DESIGN §3.)
    if (EXT == 0) {
        // (the plain kernel: the per-wave / all-wave loops below)
    } else if (EXT == EXT_PK && si.pk_fs && wl) {
        // packed postings (configs[4]), the per-wave form of the plain scorer: a long
        // term's frames of the wave's own segment run; a short term read whole by every
        // wave (its frame, or its plain words when short of PK_MIN), applied to the
        // wave's own docs only -- no barrier between terms; a skipped segment's wave
        // scores nothing (skip_wave)
        const uint32_t wd = (uint32_t)(MAX_BLOCK_DOCS + lane) << 2;
        const uint32_t dlo = (uint32_t)wave * wseg;
        const uint32_t dn = wave == WSEG - 1 ? 0x7FFFFFFFu - dlo : wseg;
        for (int j = skip_wave ? nt : 0; j < nt; ++j) {
            const uint32_t first_bits = (uint32_t)(255 - j) << 8;
            if (is_long(j)) {
                const uint32_t se = sh.wtab[j][wave];
                const int64_t f1 = lo[j] + (se & 0xFFFFu);
                for (int64_t f = lo[j] + (se >> 16); f < f1; ++f)
                    packed_apply<false>(si.pk_fh[f], si.pk_data, lane, first_bits, 0u, 0x7FFFFFFFu, wd);
            } else if ((sh.pmask[j >> 5] >> (j & 31)) & 1u) {
                for (int64_t pos = lo[j], end = hi[j]; pos < end;) {
                    const int64_t rem = end - pos;
                    if (rem > 4 * 64) {
                        uint32_t r[8];
                        scatter_load<8, 64>(post + pos, rem, lane, r, true);
                        scatter_apply_own<8>(r, first_bits, dlo, dn, wd);
                        pos += 8 * 64;
                    } else if (rem > 64) {
                        uint32_t r[4];
                        scatter_load<4, 64>(post + pos, rem, lane, r, true);
                        scatter_apply_own<4>(r, first_bits, dlo, dn, wd);
                        pos = end;
                    } else {
                        uint32_t r[1];
                        scatter_load<1, 64>(post + pos, rem, lane, r);
                        scatter_apply_own<1>(r, first_bits, dlo, dn, wd);
                        pos = end;
                    }
                }
            } else {
                for (int64_t f = lo[j]; f < hi[j]; ++f)
                    packed_apply<true>(si.pk_fh[f], si.pk_data, lane, first_bits, dlo, dn, wd);
            }
        }
        skip_wave = true;  // (nothing left for the per-wave loop below)
    }
    const uint32_t wdlo = (uint32_t)wave * wseg;
    const uint32_t wdn = wave == WSEG - 1 ? 0x7FFFFFFFu - wdlo : wseg;  // last: the rest
    const uint32_t wdummy = (uint32_t)(MAX_BLOCK_DOCS + lane) << 2;
    const uint32_t vmin = 1u << (7 - min(min_cls, 7));  // all-wave form: pruning by value
    const bool x4 = !(ablate & AB_LOAD_B32);  // rounds of 4k postings per lane by 16-byte loads
    for (int j = (ablate & AB_NO_SCATTER) || skip_wave ? nt : 0; j < nt; ++j) {
        const uint32_t first_bits = (uint32_t)(255 - j) << 8;
        const bool lj = is_long(j);
        if (lj) {
            const uint32_t se = sh.wtab[j][wave];
            int64_t pos = lo[j] + (se >> 16);
            const int64_t end = lo[j] + (se & 0xFFFFu);
            while (pos < end) {
                const int64_t rem = end - pos;
                if (rem > 8 * 64) {
                    uint32_t r[16];
                    scatter_load<16, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply<16>(sh.acc, r, first_bits);
                    pos += 16 * 64;
                } else if (rem > 4 * 64) {
                    uint32_t r[8];
                    scatter_load<8, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply<8>(sh.acc, r, first_bits);
                    pos = end;
                } else if (rem > 64) {
                    uint32_t r[4];
                    scatter_load<4, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply<4>(sh.acc, r, first_bits);
                    pos = end;
                } else {
                    uint32_t r[1];
                    scatter_load<1, 64>(post + pos, rem, lane, r);
                    scatter_apply<1>(sh.acc, r, first_bits);
                    pos = end;
                }
            }
            continue;
        }
        if (wl) {
            // a short term (< WLONG_MIN postings in the block): every wave reads the whole
            // sublist and applies the postings of its own doc segment -- no barrier
            for (int64_t pos = lo[j], end = hi[j]; pos < end;) {
                const int64_t rem = end - pos;
                if (rem > 8 * 64) {
                    uint32_t r[16];
                    scatter_load<16, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply_own<16>(r, first_bits, wdlo, wdn, wdummy);
                    pos += 16 * 64;
                } else if (rem > 4 * 64) {
                    uint32_t r[8];
                    scatter_load<8, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply_own<8>(r, first_bits, wdlo, wdn, wdummy);
                    pos = end;
                } else if (rem > 64) {
                    uint32_t r[4];
                    scatter_load<4, 64>(post + pos, rem, lane, r, x4);
                    scatter_apply_own<4>(r, first_bits, wdlo, wdn, wdummy);
                    pos = end;
                } else {
                    uint32_t r[1];
                    scatter_load<1, 64>(post + pos, rem, lane, r);
                    scatter_apply_own<1>(r, first_bits, wdlo, wdn, wdummy);
                    pos = end;
                }
            }
            continue;
        }
        int64_t pos = lo[j];
        const int64_t end = hi[j];
        if (have_pre) {
            scatter_apply<4, true>(sh.acc, pre, first_bits, vmin);
            pos = min(end, pos + (int64_t)4 * SC_THREADS);
            have_pre = false;
        }
        const bool next = j + 1 < nt && hi[j + 1] > lo[j + 1] && !is_long(j + 1);
        auto prefetch_next = [&]() {
            scatter_load<4>(post + lo[j + 1], hi[j + 1] - lo[j + 1], tid, pre, x4);
            have_pre = true;
        };
        while (pos < end) {
            const int64_t rem = end - pos;
            if (rem >= 16 * SC_THREADS) {
                uint32_t r[16];
                scatter_load<16>(post + pos, rem, tid, r, x4);
                if (rem == 16 * SC_THREADS && next) prefetch_next();
                scatter_apply<16, true>(sh.acc, r, first_bits, vmin);
                pos += 16 * SC_THREADS;
            } else if (rem > SC_THREADS) {
                uint32_t r[4];
                scatter_load<4>(post + pos, rem, tid, r, x4);
                if (rem <= 4 * SC_THREADS && next) prefetch_next();
                scatter_apply<4, true>(sh.acc, r, first_bits, vmin);
                pos += 4 * SC_THREADS;
            } else {
                uint32_t r[1];
                scatter_load<1>(post + pos, rem, tid, r);
                if (next) prefetch_next();
                scatter_apply<1, true>(sh.acc, r, first_bits, vmin);
                pos = end;
            }
        }
        // term boundary: this term's LDS writes land before any wave reads the next
        if (j + 1 < nt) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // the asm LDS writes; the threshold histogram's LDS-DMA copy.  The first half of the
    // threshold read (read_tq) goes before the barrier: thread t's own 4 bins are the
    // 16 B its own LDS-DMA wrote (no barrier needed to read them), their wave suffix
    // sums go to wsum -- the barrier the scatter needs anyway publishes them.
    if (wstamps && lane == 0) sh.wstamp[wave] = (uint32_t)(__builtin_amdgcn_s_memtime() - t_w0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    uint32_t tq_hv[4] = {0, 0, 0, 0}, tq_c = 0, tq_sfx = 0;
    if (qpre) {
        const uint4 h = reinterpret_cast<const uint4 *>(sh.u.hist)[tid];
        tq_hv[0] = h.x, tq_hv[1] = h.y, tq_hv[2] = h.z, tq_hv[3] = h.w;
        tq_c = h.x + h.y + h.z + h.w;
        tq_sfx = wave_suffix_sum(tq_c);
        if (lane == 0) sh.wsum[wave] = tq_sfx;
    }
    __syncthreads();

    stamp(1);  // scatter
    if (stamps) {
        uint32_t mx = 0, sm = 0;
        for (int w2 = 0; w2 < SC_WAVES; ++w2) {
            mx = max(mx, sh.wstamp[w2]);
            sm += sh.wstamp[w2];
        }
        atomicAdd(&g_sb_phase[9], (unsigned long long)mx);
        atomicAdd(&g_sb_phase[10], (unsigned long long)(sm / SC_WAVES));
    }
    if (ablate & AB_NO_SELECT) {
        if (tid == 0) *cn = 0;
        return;
    }
    const uint64_t doc_base = (uint64_t)doc_lo + (uint64_t)block_first;
    // Candidates are staged in the unused tail of the accumulator array when they fit
    // there and copied out coalesced (a lane-scattered 8-byte store per candidate slot
    // costs a store instruction per slot and wave); else they go straight out.
    const int n4z = (n_local + 3) >> 2;
    const bool tail_fits = 2 * k <= MAX_BLOCK_DOCS - 4 * n4z;
    uint64_t *const acc_tail = reinterpret_cast<uint64_t *>(sh.acc + 4 * n4z);
    // (full blocks leave no tail: the one-sweep selections below stage in the histogram
    // area instead, free by then -- otherwise the flush re-read the keys from global
    // memory, a round trip per item at 1.1 M / 8.8 M docs)
    uint64_t *const hist_stage = reinterpret_cast<uint64_t *>(sh.u.hist);
    static_assert(sizeof(ScoreShared().u) >= (size_t)HIST_BINS * 4, "histogram stage");
    const bool hist_fits = (uint32_t)k * 8u <= (uint32_t)HIST_BINS * 4u;
    uint64_t *stage = tail_fits ? acc_tail : nullptr;  // null: straight to ck
    uint32_t cap = (uint32_t)k;  // list capacity of the current selection (emit-above: kl)
    auto cand = [&](uint32_t pos, uint32_t w, int idx) {
        const uint32_t doc = (uint32_t)(doc_base + (uint64_t)idx);
        const uint64_t key = ((uint64_t)w << 32) | (uint64_t)(0xFFFFFFFFu - doc);
        if (pos < cap) {
            if (stage)
                stage[pos] = key;
            else
                ck[pos] = key;
        }
    };
    // final candidates: copied out (staged) and counted into the query's score
    // histogram (qhist, see read_tq); called once per item, after a barrier
    auto flush = [&](uint32_t n_c) {
        // (thread order reversed: the last waves issue these stores and atomics, so the
        // next item's record loads -- issued by the first waves -- do not wait for their
        // acknowledgements behind them in the in-order vmcnt)
        for (uint32_t i = (uint32_t)(SC_THREADS - 1 - tid); i < n_c; i += SC_THREADS) {
            const uint64_t key = stage ? stage[i] : ck[i];
            if (stage) ck[i] = key;
            if (qh) atomicAdd(&qh[min((uint32_t)(key >> 48), (uint32_t)QH_BINS - 1)], 1u);
        }
    };
    auto emit_all_touched = [&]() {
        const uint32_t n = compact_words(sh, n_local, tid, [](uint32_t w, int) { return w ? 1u : 0u; },
                                         [&](int, uint32_t pos, uint32_t w, int idx) {
                                             cand(pos, w, idx);
                                         });
        flush(min(n & 0xFFFFu, (uint32_t)k));
        if (tid == 0) *cn = (int32_t)min(n & 0xFFFFu, (uint32_t)k);
    };

    // Shared per-query threshold.  qhist[q] (when given) counts the scores of every
    // candidate the query's finished blocks emitted (distinct docs, full scores; bin
    // 4095 = 4095 and above).  Tq = the largest s with >= k counted candidates scoring
    // >= s: at least k docs score >= Tq, so the final k-th score is >= Tq and a doc
    // below Tq cannot be in the query's top-k.  When at most k of this block's docs
    // reach Tq they are its only candidates (no histogram, no tie order -- the merge
    // orders them by key); else the full selection below runs.  Items run block-major
    // (all queries' block 0 first), so Tq is close to the final k-th score after the
    // first blocks and the later blocks emit few candidates.  A stale (smaller) count
    // still gives a valid lower bound.
    // Emit-above (few blocks: no qhist, a list capacity kl > k): the query's running
    // threshold T1 (qtq = the largest k-th score of its finished blocks' full selections,
    // read at the item's start) is a lower bound of its final k-th score, so only this
    // block's docs scoring >= T1 can reach the top-k.  When at most kl of them do, one
    // append sweep emits them all -- no histogram, no tie order, no compaction (the merge
    // orders by key); else the full selection below runs (and raises qtq).  Items are
    // block-major, so every block after a query's first finds the first block's k-th
    // score: at 100 k docs (4 blocks) ~k docs of each pass it, <= kl = 2 k.
    if (EXT == EXT_FEW && !qh && qtq && kl > k) {
        const uint32_t T1 = sh.tqe;  // (written before the setup barrier)
        if (T1 > 0) {
            const bool tail_kl = 2 * kl <= MAX_BLOCK_DOCS - 4 * n4z;
            if (!tail_kl && (uint32_t)kl * 8u <= (uint32_t)HIST_BINS * 4u) stage = hist_stage;
            else if (!tail_kl) stage = nullptr;
            cap = (uint32_t)kl;
            const uint32_t thr_w = T1 << 16;
            sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int idx) {
                uint32_t pos;
                if (wave_append<true>(w >= thr_w, &sh.emit, pos)) cand(pos, w, idx);
            });
            __syncthreads();
            const uint32_t na = sh.emit;
            if (na <= (uint32_t)kl) {
                flush(na);
                if (tid == 0) *cn = (int32_t)na;
                return;
            }
            // (too many: the full selection, k keys; sh.emit is reset by the paths that use
            // it -- the radix ties set it, the fast path's compaction does not read it)
            // The sweep may have staged up to kl keys in the histogram area (a near-full
            // block leaves no accumulator tail); the fast path counts into those bins and
            // they were zeroed only at the setup, so zero them again here.
            if (fast && stage == hist_stage) reinterpret_cast<uint4 *>(sh.u.hist)[tid] = make_uint4(0, 0, 0, 0);
            cap = (uint32_t)k;
            stage = tail_fits ? acc_tail : nullptr;
            __syncthreads();  // every wave has read sh.emit (and the bins are zero again)
            if (tid == 0) sh.emit = 0;
        }
    }
    uint32_t Tq = 0;
    bool hist_dirty = false;  // keys staged in the histogram area by a sweep that overflowed
    if (qh) {
        if (qpre) {
            // second half of read_tq over the suffix sums published by the scatter
            // barrier: the crossing thread writes tq (0 from the item's start when the
            // histogram holds fewer than k candidates); one barrier
            for (int w2 = wave + 1; w2 < SC_WAVES; ++w2) tq_sfx += sh.wsum[w2];
            int e;
            uint32_t above;
            if (crossing4(tq_sfx, tq_c, tq_hv, (uint32_t)k, e, above))
                sh.tq = (uint32_t)(4 * tid + e);
            __syncthreads();
            Tq = sh.tq;
        } else {
            Tq = sh.tqe;  // (the running word, published by the setup barrier)
        }
        if (tid == 0) sh.tqn = max(sh.tqn, Tq);
        stamp(8);  // threshold read (the part of tq-select before the sweep)
        // (wsum is written again only after a barrier of the selection below; tq only
        // at the next item's start)
        if (Tq > 0) {
            // one sweep: the docs reaching Tq (usually a few dozen) are appended by
            // wave-aggregated LDS atomics in any order (the merge orders them by key)
            // (the histogram copy is consumed: its area stages the keys of a full block)
            if (!tail_fits && hist_fits && !(ablate & AB_NO_HIST_STAGE)) stage = hist_stage;
            const uint32_t thr_w = Tq << 16;
            sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int idx) {
                uint32_t pos;
                if (wave_append<XBM>(w >= thr_w, &sh.emit, pos)) cand(pos, w, idx);
            });
            __syncthreads();
            const uint32_t na = sh.emit;
            stamp(7);  // shared-threshold selection
            if (na <= (uint32_t)k) {
                flush(na);
                if (tid == 0) *cn = (int32_t)na;
                return;
            }
            hist_dirty = stage == hist_stage;
            stage = tail_fits ? acc_tail : nullptr;  // (the selections below use the histogram)
        }
    }

    if (EXT == EXT_BM && fast) {
        // A sparse item: at most k postings were scattered, so at most k docs are touched
        // and every touched doc is a candidate.  One append sweep (any order: the merge
        // orders by key) replaces the histogram sweep (an LDS atomic per word) and the two
        // compaction sweeps.  Every wave sums the scattered postings itself from the LDS
        // bounds (lane j: term j; a long term: its per-wave runs), so the branch is uniform
        // with no barrier.  In the EXT_BM instantiation only, which impact-pruned searches
        // use (di_index_search): in the plain kernel the same code cost the dense 100 k-doc
        // items 4% (2.148 vs 2.062 ms per launch, profiles/round4_p5_sparse_items_ab.txt);
        // here it takes 8.8 M skewed docs at min_impact 128 from 70.6 to 48.9 ms per batch.
        uint32_t np = 0;
        if (lane < nt) {
            if (is_long(lane)) {
#pragma unroll
                for (int w = 0; w < WSEG; ++w) {
                    const uint32_t se = sh.wtab[lane][w];
                    const uint32_t s0 = se >> 16, s1 = se & 0xFFFFu;
                    np += s1 > s0 ? s1 - s0 : 0u;
                }
            } else {
                np = (uint32_t)min(hi[lane] - lo[lane], (int64_t)0xFFFFFF);
            }
        }
        np = (uint32_t)__shfl(wave_prefix_sum(np), 63, 64);
        if (np <= (uint32_t)k) {
            if (!tail_fits && hist_fits && !(ablate & AB_NO_HIST_STAGE)) stage = hist_stage;
            sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int idx) {
                uint32_t pos;
                if (wave_append<true>(w != 0, &sh.emit, pos)) cand(pos, w, idx);
            });
            __syncthreads();
            const uint32_t na = sh.emit;
            flush(na);
            if (tid == 0) *cn = (int32_t)na;
            return;
        }
    }

    uint32_t prefix = 0, mask = 0, need = (uint32_t)k;
    int shift = 24;  // next digit of the general radix path
    if (fast) {
        // ---- fast path: score histogram -> k-th score T -------------------
        uint32_t *hist = sh.u.hist;
        // branch-free: an untouched doc (w = 0) counts into a per-lane spare bin past
        // the 4096 score bins (no same-address conflicts), never read
        const uint32_t spare = HIST_BINS + (uint32_t)lane;
        if (qpre || hist_dirty) {  // the threshold copy was read (read_tq's barriers), or
            // keys were staged there: zero the bins
            reinterpret_cast<uint4 *>(hist)[tid] = make_uint4(0, 0, 0, 0);
            __syncthreads();
        }
        sweep_words(sh.acc, n_local, tid, [&](uint32_t w, int) {
            atomicAdd(&hist[w ? (w >> 16) : spare], 1u);
        });
        __syncthreads();
        // thread t owns bins 4t..4t+3; s = touched docs with score >= 4t
        const uint4 h4 = reinterpret_cast<const uint4 *>(hist)[tid];
        const uint32_t c = h4.x + h4.y + h4.z + h4.w;
        uint32_t s = wave_suffix_sum(c);
        if (lane == 0) sh.wsum[wave] = s;
        __syncthreads();
        uint32_t total = 0;
        for (int w2 = 0; w2 < SC_WAVES; ++w2) {
            const uint32_t x = sh.wsum[w2];
            total += x;
            if (w2 > wave) s += x;
        }
        __syncthreads();  // wsum is reused by the compaction
        if (total <= (uint32_t)k) {  // every touched doc is a candidate
            emit_all_touched();
            return;
        }
        {
            const uint32_t hv[4] = {h4.x, h4.y, h4.z, h4.w};
            int e;
            uint32_t ab;
            if (crossing4(s, c, hv, need, e, ab)) {  // exactly one thread: T is in its bins
                sh.thr = (uint32_t)(4 * tid + e);
                sh.above = ab;
                sh.ties = hv[e];
            }
        }
        __syncthreads();
        stamp(2);  // histogram + threshold
        if (ablate & AB_STOP_AT_KTH) {
            if (tid == 0) *cn = 0;
            return;
        }
        // (this block alone has >= k docs scoring >= T: a lower bound of the query's final
        // k-th score for block-max, qtq)
        if (tid == 0) sh.tqn = max(sh.tqn, sh.thr);
        const uint32_t T = sh.thr, ties = sh.ties;  // T >= 1: every touched score is
        const uint32_t above = sh.above;             // nonzero

        need -= above;
        if (ties == need || ties <= (uint32_t)TIE_CAP) {
            // scores above T are in; the ties at T all go in, or into a list (the
            // histogram is consumed) as (low 16 bits of the word, 0xFFFF - idx):
            // unique, and larger = first-touch earlier, then doc smaller.
            // Compaction: one sweep marks each lane's candidates and ties in two
            // 32-bit masks over its 32 words (4 per ds_read_b128); a block scan of the
            // counts gives positions; the write loop visits only the marked words
            // (~1 per lane), not all 32.
            const bool all_ties = ties == need;
            const uint32_t thr_a = (all_ties ? T : T + 1) << 16;  // list A: w >= thr_a
            uint32_t *tl = sh.u.hist;
            uint32_t ma = 0, mb = 0;
            {
                const uint4 *a4 = reinterpret_cast<const uint4 *>(sh.acc);
                const int n4 = (n_local + 3) >> 2;
#pragma unroll
                for (int i = 0; i < SC_PER_THREAD / 4; ++i) {
                    const int q4 = i * SC_THREADS + tid;
                    const uint4 y = a4[q4];  // q4 < 8192: inside the array
                    const bool ok = q4 < n4;
                    const uint32_t wv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t w = ok ? wv[e] : 0u;
                        ma |= (uint32_t)(w >= thr_a) << (4 * i + e);
                        mb |= (uint32_t)((w >> 16) == T) << (4 * i + e);
                    }
                }
                if (all_ties) mb = 0;
            }
            const uint32_t cnt = (uint32_t)__builtin_popcount(ma) +
                                 ((uint32_t)__builtin_popcount(mb) << 16);
            const uint32_t incl = wave_prefix_sum(cnt);
            if (lane == 63) sh.wsum[wave] = incl;
            __syncthreads();
            uint32_t base = incl - cnt;
            for (int w2 = 0; w2 < wave; ++w2) base += sh.wsum[w2];
            stamp(6);
            {
                uint32_t pa = base & 0xFFFFu, pb = base >> 16;
                auto idx_of = [&](int bit) { return 4 * ((bit >> 2) * SC_THREADS + tid) + (bit & 3); };
                while (ma) {
                    const int bit = __builtin_ctz(ma);
                    ma &= ma - 1;
                    const int idx = idx_of(bit);
                    cand(pa++, sh.acc[idx], idx);
                }
                while (mb) {
                    const int bit = __builtin_ctz(mb);
                    mb &= mb - 1;
                    const int idx = idx_of(bit);
                    tl[pb++] = ((sh.acc[idx] & 0xFFFFu) << 16) | (0xFFFFu - (uint32_t)idx);
                }
            }
            __syncthreads();
            stamp(3);  // compaction
            if (ablate & AB_STOP_AT_COMPACT) {
                if (tid == 0) *cn = 0;
                return;
            }
            if (!all_ties && ties <= 64) {
                // few ties (the common case): one wave ranks them -- lane i holds tie
                // key i and counts the larger keys among all lanes (keys are unique);
                // the `need` largest go right after the `above` candidates, in rank
                // order, with no atomics and no further block barrier
                if (wave == 0) {
                    const uint32_t x = lane < (int)ties ? tl[lane] : 0u;
                    uint32_t rank = 0;
                    for (int j = 0; j < (int)ties; ++j) rank += __shfl(x, j, 64) > x;
                    if (lane < (int)ties && rank < need)
                        cand(above + rank, (T << 16) | (x >> 16), (int)(0xFFFFu - (x & 0xFFFFu)));
                }
                __syncthreads();
                stamp(4);  // tie order
                flush((uint32_t)k);
                stamp(5);  // copy-out
                if (tid == 0) *cn = k;
            } else if (!all_ties) {
                // radix select of the `need` largest tie keys (4 digits)
                uint32_t *h = sh.v.h256;
                uint32_t tp = 0, tm = 0, tneed = need;
                for (int sft = 24; sft >= 0; sft -= 8) {
                    if (tid < 256) h[tid] = 0;
                    __syncthreads();
                    for (uint32_t i = tid; i < ties; i += SC_THREADS) {
                        const uint32_t x = tl[i];
                        if ((x & tm) == tp) atomicAdd(&h[(x >> sft) & 255u], 1u);
                    }
                    __syncthreads();
                    if (wave == 0) {
                        const uint32_t hb[4] = {h[4 * lane], h[4 * lane + 1], h[4 * lane + 2],
                                                h[4 * lane + 3]};
                        const uint32_t c4 = hb[0] + hb[1] + hb[2] + hb[3];
                        int e;
                        uint32_t ab;
                        if (crossing4(wave_suffix_sum(c4), c4, hb, tneed, e, ab)) {
                            sh.bin = (uint32_t)(4 * lane + e);
                            sh.bin_above = ab;
                        }
                    }
                    __syncthreads();
                    tp |= sh.bin << sft;
                    tm |= 255u << sft;
                    tneed -= sh.bin_above;
                }
                // the keys are unique: exactly `need` ties are >= tp; they follow the
                // `above` candidates
                if (tid == 0) sh.emit = above;
                __syncthreads();
                for (uint32_t i0 = 0; i0 < ties; i0 += SC_THREADS) {
                    const uint32_t i = i0 + tid;
                    const uint32_t x = i < ties ? tl[i] : 0u;
                    uint32_t pos;
                    if (wave_append<XBM>(i < ties && x >= tp, &sh.emit, pos))
                        cand(pos, (T << 16) | (x >> 16), (int)(0xFFFFu - (x & 0xFFFFu)));
                }
                __syncthreads();
                flush((uint32_t)k);
                // sh.emit == k by construction; anything else is a selection bug
                if (tid == 0) *cn = sh.emit == (uint32_t)k ? k : -2;
            } else {
                flush((uint32_t)k);
                if (tid == 0) *cn = k;
            }
            return;
        }
        // more ties than the list holds: the general path finishes from score T
        // (digits 15..8 and 7..0 of the word, then doc order)
        prefix = T << 16;
        mask = 0xFFFF0000u;
        shift = 8;
    }

    // ---- general path: block-wide radix select on the 32-bit words ----------
    auto id_key = [](uint32_t w, int) { return w; };
    if (shift == 24) {  // pass 0 also counts touched docs
        score_radix_pass(sh, n_local, 24, need, id_key,
                         [](uint32_t w, int, uint32_t) { return w != 0; });
        if (sh.u.rs.total <= (uint32_t)k) {
            __syncthreads();
            emit_all_touched();
            return;
        }
    } else {
        score_radix_pass(sh, n_local, shift, need, id_key,
                         [prefix, mask](uint32_t w, int, uint32_t) {
                             return w != 0 && (w & mask) == prefix;
                         });
    }
    for (;; shift -= 8) {
        prefix |= sh.u.rs.bin << shift;
        mask |= 255u << shift;
        need -= sh.u.rs.above;
        if (shift == 0) break;
        __syncthreads();
        score_radix_pass(sh, n_local, shift - 8, need, id_key,
                         [prefix, mask](uint32_t w, int, uint32_t) {
                             return w != 0 && (w & mask) == prefix;
                         });
    }
    const uint32_t T = prefix;
    if (tid == 0) sh.tqn = max(sh.tqn, T >> 16);
    const uint32_t ties = sh.u.rs.tot[sh.u.rs.bin];

    // doc-order cut among the ties: the `need` smallest doc indices
    // (all ties when exactly `need` of them exist)
    uint32_t dcut = 0;
    if (ties != need) {
        uint32_t dneed = need, dprefix = 0, dmask = 0;
        auto dkey = [](uint32_t, int idx) { return 0xFFFFu - (uint32_t)idx; };
        for (int sft = 8;; sft -= 8) {
            __syncthreads();
            score_radix_pass(sh, n_local, sft, dneed, dkey,
                             [T, dprefix, dmask](uint32_t w, int, uint32_t kk) {
                                 return w == T && (kk & dmask) == dprefix;
                             });
            dprefix |= sh.u.rs.bin << sft;
            dmask |= 255u << sft;
            dneed -= sh.u.rs.above;
            if (sft == 0) break;
        }
        dcut = dprefix;  // keep ties whose (0xFFFF - idx) >= dcut
    }
    __syncthreads();
    const uint32_t n = compact_words(
        sh, n_local, tid,
        [T, dcut](uint32_t w, int idx) -> uint32_t {
            return (w != 0 && (w > T || (w == T && (0xFFFFu - (uint32_t)idx) >= dcut))) ? 1u : 0u;
        },
        [&](int, uint32_t pos, uint32_t w, int idx) { cand(pos, w, idx); });
    flush((uint32_t)k);
    // exactly k by construction; anything else is a selection bug -> flag it
    if (tid == 0) *cn = (n & 0xFFFFu) == (uint32_t)k ? k : -2;
}

// Block order of each query for block-max scoring (BASELINE configs[4]): blocks by
// descending upper bound sum_j emax(t_j, b) (ties: block order), so the query's shared
// threshold -- the k-th score among the candidates of its finished blocks -- rises to
// near its final value within the first blocks and the later, weaker blocks skip more
// of their wave segments.  Any order is exact (the threshold is a lower bound of the
// final k-th score whatever blocks it has seen; the merge orders by key).  One
// workgroup per query; rank by counting (nb <= BO_MAX_BLOCKS).
__global__ void __launch_bounds__(256)
block_order_kernel(SubIndex si, int nb, int64_t n_terms, const uint32_t *__restrict__ q_terms,
                   const int32_t *__restrict__ cu_q, uint16_t *__restrict__ border) {
    __shared__ uint32_t bound[BO_MAX_BLOCKS];
    const int q = blockIdx.x;
    const int q0 = cu_q[q], nt = cu_q[q + 1] - q0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        uint32_t u = 0;
        for (int j = 0; j < nt && j < WTERMS; ++j) {
            const uint32_t t = q_terms[q0 + j];
            if (t >= n_terms) continue;
            const int64_t e = find_entry(si, nb, t, b);
            if (e >= 0) u += si.emax[e];
        }
        bound[b] = u;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        const uint32_t u = bound[b];
        int r = 0;
        for (int x = 0; x < nb; ++x) {
            const uint32_t v = bound[x];
            r += v > u || (v == u && x < b);
        }
        border[(int64_t)q * nb + r] = (uint16_t)b;
    }
}

// Persistent: one workgroup per CU walks the (query, block) items, so the per-
// workgroup launch cost (16 waves, 154 KiB of LDS) is paid once per CU, not per item.
template <int EXT>
__global__ void __launch_bounds__(SC_THREADS)
score_blocks_kernel(const uint32_t *__restrict__ post, SubIndex si, int min_cls, int nb,
                    int block_docs, int64_t n_terms, uint32_t n_docs, uint32_t doc_lo,
                    const uint32_t *__restrict__ q_terms, const int32_t *__restrict__ cu_q, int k,
                    uint64_t *__restrict__ cand_key, int32_t *__restrict__ cand_n, int n_items,
                    int n_q, uint32_t *__restrict__ qhist, int ablate,
                    ItemRec *__restrict__ rec, uint32_t *__restrict__ long_flag,
                    float bm_factor, unsigned long long *__restrict__ bm_stat,
                    uint16_t *__restrict__ border, uint32_t *__restrict__ qtq,
                    int rec_slots, int kl, int tq_sched) {
    // The members of ScoreArgs, in its order, as separate parameters: a by-value struct
    // cannot carry __restrict__, and without it the plain and few-block instantiations
    // spill (8 and 3 VGPRs against 2, 37 and 20 scratch instructions against 14:
    // profiles/scorer_refactor_isa.txt).  launch_score unpacks the struct; the item
    // functions take it by reference.
    const ScoreArgs a{post, si, min_cls, nb, block_docs, n_terms, n_docs, doc_lo,
                      q_terms, cu_q, k, cand_key, cand_n, n_items, n_q, qhist, ablate, rec,
                      long_flag, bm_factor, bm_stat, border, qtq, rec_slots, kl, tq_sched};
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ScoreShared &sh = *reinterpret_cast<ScoreShared *>(smem);
    if ((uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char *)smem) != 0) {
        // scatter_apply addresses the accumulators from LDS address 0 (folded away when
        // the segment starts there, as it does): otherwise fail every item loudly
        for (int item = blockIdx.x; item < n_items; item += gridDim.x)
            if (threadIdx.x == 0) a.cand_n[item] = -1;
        return;
    }
    if (threadIdx.x == 0) {  // (the first item's barriers publish them)
        sh.bm_cnt[0] = sh.bm_cnt[1] = 0ull;
        sh.tqn = 0;
    }
    // items block-major: item = b * n_q + q (the shared threshold, see score_item)
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int q = item % n_q, r_ = item / n_q;
        const int b = (EXT == EXT_BM || EXT == EXT_PK) && a.border
                          ? (int)a.border[(int64_t)q * a.nb + r_] : r_;
        score_item<EXT>(sh, q, b, a, a.rec ? a.rec + (int64_t)item * a.rec_slots : nullptr);
        __syncthreads();  // every wave is done with the LDS of this item
        // the item's threshold into the query's running one, here rather than inside the
        // selection: qtq and the value read at the item's start need no registers across
        // the scatter (they cost the instantiation spills)
        if (threadIdx.x == 0) {
            const uint32_t t = sh.tqn;
            if (a.qtq && t > sh.tqe) atomicMax(&a.qtq[q], t);
            sh.tqn = 0;
        }
    }
    if ((EXT == EXT_BM || EXT == EXT_PK) && a.bm_stat && threadIdx.x == 0 && sh.bm_cnt[0]) {
        atomicAdd(&a.bm_stat[0], sh.bm_cnt[0]);
        atomicAdd(&a.bm_stat[1], sh.bm_cnt[1]);
    }
}

// The items of the long queries (score_long_item), after score_blocks_kernel on the
// same stream: it gave them no candidates and raised *long_flag (0: every workgroup
// leaves at once).  Persistent: every workgroup lists the long queries of each round of
// SC_THREADS queries in query order (a block scan: the same list in every workgroup)
// and takes its share of their (query, block) items.
__global__ void __launch_bounds__(SC_THREADS)
score_long_kernel(ScoreArgs a) {
    if (__builtin_amdgcn_readfirstlane(*a.long_flag) == 0) return;
    const int n_q = a.n_q, nb = a.nb;
    const int32_t *__restrict__ cu_q = a.cu_q;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ScoreShared &sh = *reinterpret_cast<ScoreShared *>(smem);
    uint32_t *list = &sh.wtab[0][0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int r0 = 0; r0 < n_q; r0 += SC_THREADS) {
        const int q = r0 + tid;
        int nt = 0;
        if (q < n_q) nt = cu_q[q + 1] - cu_q[q];
        const uint32_t is_long = nt > MAX_TERMS && nt <= LONG_TERMS ? 1u : 0u;
        const uint32_t incl = wave_prefix_sum(is_long);
        if (lane == 63) sh.wsum[wave] = incl;
        __syncthreads();
        uint32_t base = incl - is_long, n = 0;
        for (int w2 = 0; w2 < SC_WAVES; ++w2) {
            const uint32_t x = sh.wsum[w2];
            if (w2 < wave) base += x;
            n += x;
        }
        if (is_long) list[base] = (uint32_t)q;
        __syncthreads();
        const int n_items = (int)n * nb;
        for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
            const int lq = (int)list[it % n], b = it / n;
            score_long_item(sh, lq, b, a);
            __syncthreads();  // the item's LDS (and the list) stay consistent
        }
        __syncthreads();  // the list and wsum are rewritten by the next round
    }
}


// ---------------------------------------------------------------------------
// host: the launcher
// ---------------------------------------------------------------------------
namespace {

// Kernels using more than 64 KiB of dynamic LDS must opt in: once per process and device.
void enable_score_lds() {
    static std::atomic<uint64_t> set_on{0};
    constexpr int LDS = (int)sizeof(ScoreShared);
    dynamic_lds_once(set_on, {{(const void *)score_blocks_kernel<0>, LDS},
                              {(const void *)score_blocks_kernel<EXT_BM>, LDS},
                              {(const void *)score_blocks_kernel<EXT_FEW>, LDS},
                              {(const void *)score_blocks_kernel<EXT_PK>, LDS},
                              {(const void *)score_long_kernel, LDS}});
}

}  // namespace

void launch_score(const ScoreLaunch &L) {
    static_assert(sizeof(ScoreShared) <= 160 * 1024, "ScoreShared exceeds LDS");
    enable_score_lds();
    const ScoreArgs &a = L.a;
    hipStream_t s = L.stream;
    // (the order kernel reads no packed array: the plain tables)
    SubIndex plain = a.si;
    plain.pk_fs = nullptr, plain.pk_fwt = nullptr, plain.pk_fh = nullptr, plain.pk_data = nullptr;
    if (a.border) {
        hipLaunchKernelGGL(block_order_kernel, dim3(a.n_q), dim3(256), 0, s, plain, a.nb,
                           a.n_terms, a.q_terms, a.cu_q, a.border);
        check_launch("block_order");
    }
    if (a.rec) {
        hipLaunchKernelGGL(item_setup_kernel, dim3(a.n_items), dim3(128), 0, s, a.si, a.min_cls,
                           a.nb, a.n_terms, a.q_terms, a.cu_q, a.n_q,
                           a.rec, a.border, a.rec_slots);
        check_launch("item_setup");
    }
    const dim3 grid(std::min(a.n_items, n_cu()));
    hipLaunchKernelGGL(L.pk    ? score_blocks_kernel<EXT_PK>
                       : L.ext ? score_blocks_kernel<EXT_BM>
                       : L.few ? score_blocks_kernel<EXT_FEW>
                               : score_blocks_kernel<0>,
                       grid, dim3(SC_THREADS), sizeof(ScoreShared), s, a.post, a.si, a.min_cls,
                       a.nb, a.block_docs, a.n_terms, a.n_docs, a.doc_lo, a.q_terms, a.cu_q, a.k,
                       a.cand_key, a.cand_n, a.n_items, a.n_q, a.qhist, a.ablate, a.rec,
                       a.long_flag, a.bm_factor, a.bm_stat, a.border, a.qtq, a.rec_slots, a.kl,
                       a.tq_sched);
    check_launch("score_blocks");
    // (the long queries read the plain postings: no packed arrays.  The kernel gets the
    // whole struct where it once got 16 values; it reads none of the other members)
    ScoreArgs la = a;
    la.si = plain;
    hipLaunchKernelGGL(score_long_kernel, grid, dim3(SC_THREADS), sizeof(ScoreShared), s, la);
    check_launch("score_long");
    if (a.ablate & AB_STAMPS) {
        unsigned long long ph[12];
        DI_HIP(hipStreamSynchronize(s));
        DI_HIP(hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_sb_phase), sizeof ph));
        fprintf(stderr, "score_blocks phase cycles (workgroup 0, cumulative): setup %llu "
                        "scatter %llu hist %llu [count %llu] write %llu ties %llu copy %llu "
                        "tq-select %llu [tq-read %llu] scatter-loop slowest wave %llu mean wave %llu\n",
                ph[0], ph[1], ph[2], ph[6], ph[3], ph[4], ph[5], ph[7], ph[8], ph[9], ph[10]);
    }
}

}  // namespace di
