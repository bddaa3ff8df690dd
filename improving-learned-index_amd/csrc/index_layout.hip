// index_layout.hip -- the blocked device layout of the quantized index (the ten arrays
// build_index() of index.hip uploads: post, post_flat, tb_start, eblk, epos, seg, lid, wmeta,
// emax, wmax) built on the device from the CSR di_index_create takes, byte for byte the
// host route's, gfx950.  build_index() is the specification; what runs here:
//   il_check     term_off[0] >= 0 and monotone (error word), its first and last offset
//   il_input     the largest doc over all postings (doc_hi = 0), and per term the place of
//                its first zero value (atomicMin: a minimum, no position handed out)
//   il_count     kept postings (before the term's first zero, doc in [doc_lo, doc_hi)) per
//                tile of IB_TILE postings; il_scan: their exclusive scan
//   il_compact   the kept postings, in order, as 16-byte records (doc_in_block << 8 | value,
//                term, block, 0); a posting's term by a search of term_off (one search a wave,
//                a lane past that term's end searches on)
//   il_hist / il_scan / il_scatter   (ib_sort.h) the stable radix sort by (term, block):
//                ceil(bits(nb - 1) / 8) passes on the block, then ceil(bits(n_terms - 1) / 8)
//                on the term (none with one block: the input is term-major).  Inside every
//                (term, block) sublist the input order stays.  32 B read + 16 B written per
//                posting and pass, two 16-byte record buffers of scratch.
//   il_heads     run heads of the sorted key -> (scan) entry numbers; il_entries writes
//                eblk / epos and the entry's term, il_tbstart tb_start by a search of those
//   il_long      sublists of >= wlong_min postings -> (scan) lid (il_lid)
//   il_segment   one workgroup per long sublist: seg (whole-sublist class prefixes), emax,
//                wmax, and its words placed stably by wave segment (counts, then ballot
//                ranks plus LDS counters in wave and round order)
//   il_deal      emit_group: one wave per group (a short sublist, or one wave segment of a
//                long one): a stable counting sort by (class, bank) in LDS, then the greedy
//                deal run wave-uniform -- lane k holds the head and count of bucket k of the
//                class, the pick is a few scalar bit operations, the picked lane writes its
//                head into an LDS order list -- and a coalesced store of the encoded words.
//                A long sublist's segments are dealt twice (classes, and flat as one class).
// Deviation from the host route: a group of more than 2048 postings (a doc repeated inside
// a term so that a 2048-doc wave segment overfills, or DI_WLONG_MIN above 2049 with such a
// short sublist) is DI_EINVAL through the error word; build_index() takes both silently.
// LDS: il_deal 3 KiB per 64-thread workgroup for groups up to 128 postings (short sublists
// at the default wlong_min), 18 KiB for groups up to 2048 (8 workgroups a CU); il_segment
// 0.5 KiB.  No atomic hands out a position anywhere: counts, minima and maxima only.
#include <hip/hip_runtime.h>

#include <cstring>

#include "di_common.h"
#include "ib_sort.h"
#include "index_layout.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int IL_ERR_OFF = 1;    // term_off[0] < 0 or term_off not monotone
constexpr int IL_ERR_GROUP = 2;  // a group of more than IL_GROUP_MAX postings
constexpr int IL_GROUP_MAX = 2048, IL_GROUP_SHORT = 128;
constexpr uint32_t IL_NO = 0xFFFFFFFFu;

struct IlCtrl {
    int32_t err;
    uint32_t max_doc, has_zero, pad;
    int64_t first, last;
};

struct IlIn {
    const int64_t *term_off;
    int64_t n_terms;
    const uint32_t *pdoc;
    const uint8_t *pval;
    int64_t first, n;  // postings [first, first + n) of pdoc / pval
    uint32_t doc_lo, doc_hi, bd;
    const unsigned long long *zfirst;  // per term the place of its first zero (null: none)
};

__global__ void __launch_bounds__(IB_THREADS)
il_check_kernel(const int64_t *__restrict__ term_off, int64_t n_terms, IlCtrl *__restrict__ ctrl) {
    bool bad = false;
    for (int64_t t = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; t < n_terms;
         t += (int64_t)gridDim.x * IB_THREADS)
        bad |= term_off[t + 1] < term_off[t];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bad |= term_off[0] < 0;
        ctrl->first = term_off[0];
        ctrl->last = term_off[n_terms];
    }
    if (bad) atomicOr(&ctrl->err, IL_ERR_OFF);
}

// The term of posting p: the last t in [lo, n_terms) with term_off[t] <= p.
__device__ __forceinline__ int64_t il_term_from(const int64_t *__restrict__ term_off, int64_t lo,
                                                int64_t n_terms, int64_t p) {
    int64_t hi = n_terms;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (term_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(IB_THREADS)
il_input_kernel(IlIn in, unsigned long long *__restrict__ zfirst, IlCtrl *__restrict__ ctrl) {
    uint32_t m = 0;
    bool zero = false;
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < in.n;
         i += (int64_t)gridDim.x * IB_THREADS) {
        const int64_t p = in.first + i;
        m = max(m, in.pdoc[p]);
        if (in.pval[p] == 0) {
            zero = true;
            const int64_t t = il_term_from(in.term_off, 0, in.n_terms, p);
            atomicMin(&zfirst[t], (unsigned long long)p);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if (lane_id() == 0 && m > 0) atomicMax(&ctrl->max_doc, m);
    if (zero) atomicOr(&ctrl->has_zero, 1u);
}

// Is posting first + i kept?  -> its value, its doc relative to doc_lo, and (want_term, or
// where zeros cut terms short) its term.  Uniform control flow: every lane of a wave calls it.
__device__ __forceinline__ bool il_kept(const IlIn &in, int64_t i, bool want_term, uint32_t &rel,
                                        uint32_t &val, uint32_t &term) {
    const int64_t i_wave = i - lane_id();  // the wave's first posting
    int64_t t0 = 0;
    const bool terms = want_term || in.zfirst;
    if (terms && i_wave < in.n) t0 = il_term_from(in.term_off, 0, in.n_terms, in.first + i_wave);
    if (i >= in.n) return false;
    const int64_t p = in.first + i;
    val = in.pval[p];
    const uint32_t d = in.pdoc[p];
    if (val == 0 || d < in.doc_lo || d >= in.doc_hi) return false;
    rel = d - in.doc_lo;
    if (!terms) return true;
    int64_t t = t0;
    if (p >= in.term_off[t0 + 1]) t = il_term_from(in.term_off, t0 + 1, in.n_terms, p);
    term = (uint32_t)t;
    return !in.zfirst || (unsigned long long)p < in.zfirst[t];
}

__global__ void __launch_bounds__(IB_THREADS)
il_count_kernel(IlIn in, int64_t n_tiles, uint32_t *__restrict__ tile_kept) {
    __shared__ uint32_t wsum[IB_WAVES];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t kept = 0;  // of this wave (the same in all its lanes)
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i = tile * IB_TILE + (int64_t)r * IB_THREADS + threadIdx.x;
            uint32_t rel, val, term;
            kept += (uint32_t)__popcll(__ballot(il_kept(in, i, false, rel, val, term)));
        }
        if (lane_id() == 0) wsum[wave_id()] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
            for (int w = 0; w < IB_WAVES; ++w) s += wsum[w];
            tile_kept[tile] = s;
        }
        __syncthreads();  // wsum is free again
    }
}

__global__ void __launch_bounds__(IB_THREADS)
il_compact_kernel(IlIn in, int64_t n_tiles, const int64_t *__restrict__ tile_off, int64_t cap,
                  uint4 *__restrict__ out) {
    __shared__ uint32_t wcnt[IB_WAVES];
    const int lane = lane_id(), wave = wave_id();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t run = tile_off[tile];
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i0 = tile * IB_TILE + (int64_t)r * IB_THREADS;
            if (i0 >= in.n) break;  // (the same for the whole workgroup)
            uint32_t rel = 0, val = 0, term = 0;
            const bool keep = il_kept(in, i0 + threadIdx.x, true, rel, val, term);
            const uint64_t m = __ballot(keep);
            if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (int w = 0; w < IB_WAVES; ++w) {
                if (w < wave) before += wcnt[w];
                all += wcnt[w];
            }
            if (keep) {
                const int64_t pos = run + before + __popcll(m & ((1ull << lane) - 1));
                if (pos >= 0 && pos < cap)
                    out[pos] = make_uint4(((rel % in.bd) << 8) | val, term, rel / in.bd, 0u);
            }
            run += all;
            __syncthreads();  // wcnt is free again
        }
    }
}

// head[i] = 1 where sorted record i starts a run of its key (term, block)
__global__ void __launch_bounds__(IB_THREADS)
il_heads_kernel(const uint4 *__restrict__ src, int64_t n, uint32_t *__restrict__ head) {
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * IB_THREADS) {
        bool h = true;
        if (i > 0) {
            const uint4 a = src[i - 1], b = src[i];
            h = a.y != b.y || a.z != b.z;
        }
        head[i] = h ? 1u : 0u;
    }
}

// Entry e = the run heads before record i: its block, its start, its term.
__global__ void __launch_bounds__(IB_THREADS)
il_entries_kernel(const uint4 *__restrict__ src, int64_t n, const uint32_t *__restrict__ head,
                  const int64_t *__restrict__ off, int64_t n_ent, uint16_t *__restrict__ eblk,
                  uint32_t *__restrict__ epos, uint32_t *__restrict__ eterm) {
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * IB_THREADS) {
        if (i == n - 1) epos[n_ent] = (uint32_t)n;
        if (!head[i]) continue;
        const int64_t e = off[i];
        if (e < 0 || e >= n_ent) continue;  // (never: the scan counted the heads)
        const uint4 r = src[i];
        eblk[e] = (uint16_t)r.z;
        epos[e] = (uint32_t)i;
        eterm[e] = r.y;
    }
}

// tb_start[t] = the entries of the terms before t (the first e with eterm[e] >= t)
__global__ void __launch_bounds__(IB_THREADS)
il_tbstart_kernel(const uint32_t *__restrict__ eterm, int64_t n_ent, int64_t n_terms,
                  uint32_t *__restrict__ tb_start) {
    for (int64_t t = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; t <= n_terms;
         t += (int64_t)gridDim.x * IB_THREADS) {
        int64_t lo = 0, hi = n_ent;  // the first e in [0, n_ent] with eterm[e] >= t
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)eterm[mid] < t) lo = mid + 1; else hi = mid;
        }
        tb_start[t] = (uint32_t)lo;
    }
}

__global__ void __launch_bounds__(IB_THREADS)
il_long_kernel(const uint32_t *__restrict__ epos, int64_t n_ent, uint32_t wlong_min,
               uint32_t *__restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; e < n_ent;
         e += (int64_t)gridDim.x * IB_THREADS)
        flag[e] = epos[e + 1] - epos[e] >= wlong_min ? 1u : 0u;
}

__global__ void __launch_bounds__(IB_THREADS)
il_lid_kernel(const uint32_t *__restrict__ flag, const int64_t *__restrict__ off, int64_t n_ent,
              int64_t n_long, uint32_t *__restrict__ lid, uint32_t *__restrict__ long_ent) {
    for (int64_t e = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; e < n_ent;
         e += (int64_t)gridDim.x * IB_THREADS) {
        const int64_t id = off[e];
        const bool is_long = flag[e] && id >= 0 && id < n_long;
        lid[e] = is_long ? (uint32_t)id : IL_NO;
        if (is_long) long_ent[id] = (uint32_t)e;
    }
}

__device__ __forceinline__ int il_cls(uint32_t w) { return 7 - (31 - __clz((int)(w & 255u))); }
__device__ __forceinline__ uint32_t il_encode(uint32_t w) {
    return (((w >> 8) << 10) | (w & 255u)) ^ IL_POST_X;
}

// One workgroup per long sublist: the whole-sublist metadata, and its words placed by wave
// segment (stable) into segw[s0 ...); segoff[id * 17 + w] = where segment w starts.
__global__ void __launch_bounds__(IB_THREADS)
il_segment_kernel(const uint4 *__restrict__ src, const uint32_t *__restrict__ epos,
                  const uint32_t *__restrict__ long_ent, int64_t n_long, uint32_t S,
                  uint32_t *__restrict__ segw, uint32_t *__restrict__ segoff,
                  uint16_t *__restrict__ seg, uint8_t *__restrict__ emax,
                  uint8_t *__restrict__ wmax, IlCtrl *__restrict__ ctrl) {
    __shared__ uint32_t ccnt[8], wtot[IL_WSEG], wmx[IL_WSEG], run[IL_WSEG];
    __shared__ uint32_t wcnt[IB_WAVES][IL_WSEG];
    const int lane = lane_id(), wave = wave_id();
    for (int64_t id = blockIdx.x; id < n_long; id += gridDim.x) {
        const uint32_t e = long_ent[id];
        const uint32_t s0 = epos[e], len = epos[e + 1] - s0;
        if (threadIdx.x < 8) ccnt[threadIdx.x] = 0;
        if (threadIdx.x < IL_WSEG) {
            wtot[threadIdx.x] = 0;
            wmx[threadIdx.x] = 0;
            for (int w = 0; w < IB_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < len; i += IB_THREADS) {  // (counts and maxima)
            const uint32_t x = src[(int64_t)s0 + i].x;
            const uint32_t w = min((x >> 8) / S, (uint32_t)IL_WSEG - 1);
            atomicAdd(&ccnt[il_cls(x)], 1u);
            atomicAdd(&wtot[w], 1u);
            atomicMax(&wmx[w], x & 255u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t r = 0, mx = 0, big = 0;
            for (int c = 0; c < 8; ++c) seg[(int64_t)e * 8 + c] = (uint16_t)(r += ccnt[c]);
            r = 0;
            for (int w = 0; w < IL_WSEG; ++w) {
                run[w] = r;
                segoff[id * (IL_WSEG + 1) + w] = r;
                r += wtot[w];
                big = max(big, wtot[w]);
                mx = max(mx, wmx[w]);
                wmax[id * IL_WSEG + w] = (uint8_t)wmx[w];
            }
            segoff[id * (IL_WSEG + 1) + IL_WSEG] = r;
            emax[e] = (uint8_t)mx;
            if (big > (uint32_t)IL_GROUP_MAX) atomicOr(&ctrl->err, IL_ERR_GROUP);
        }
        __syncthreads();
        for (uint32_t i0 = 0; i0 < len; i0 += IB_THREADS) {
            const uint32_t i = i0 + threadIdx.x;
            const bool valid = i < len;
            const uint32_t x = valid ? src[(int64_t)s0 + i].x : 0u;
            const uint32_t w = min((x >> 8) / S, (uint32_t)IL_WSEG - 1);
            uint64_t same = __ballot(valid);  // the valid lanes of this wave in segment w
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint64_t m = __ballot(valid && ((w >> b) & 1u));
                same &= ((w >> b) & 1u) ? m : ~m;
            }
            const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
            if (valid && rank == 0) wcnt[wave][w] = (uint32_t)__popcll(same);
            __syncthreads();
            if (valid) {
                uint32_t before = 0;
                for (int u = 0; u < wave; ++u) before += wcnt[u][w];
                const uint32_t pos = run[w] + before + rank;
                if (pos < len) segw[(int64_t)s0 + pos] = x;  // (always: the counts add up)
            }
            __syncthreads();
            if (threadIdx.x < IL_WSEG) {
                uint32_t all = 0;
                for (int u = 0; u < IB_WAVES; ++u) {
                    all += wcnt[u][threadIdx.x];
                    wcnt[u][threadIdx.x] = 0;
                }
                run[threadIdx.x] += all;
            }
            __syncthreads();
        }
    }
}

// emit_group of build_index() by one wave.  in[0, n) holds the group's words in group order
// (overwritten: the order list lives there); the encoded words go to dst[0, n), the class
// ends (+ base) to cum[0, 8) when given.  All 64 lanes call it; n <= CAP.
template <int CAP>
__device__ __forceinline__ void il_deal(uint32_t *in, uint32_t *bk, uint32_t *start,
                                        uint32_t *cur, int n, bool one_class, bool x4,
                                        uint32_t *__restrict__ dst, uint32_t base,
                                        uint16_t *__restrict__ cum) {
    const int lane = threadIdx.x;  // (one wave a workgroup)
    auto key_of = [&](uint32_t w) {
        return (uint32_t)(one_class ? 0 : il_cls(w)) * 32u + ((w >> 8) & 31u);
    };
    // the buckets' sizes (counts) and starts: stable counting sort by (class, bank)
#pragma unroll
    for (int j = 0; j < 4; ++j) start[lane * 4 + j] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) atomicAdd(&start[key_of(in[i])], 1u);
    __syncthreads();
    {
        uint32_t c[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (c[j] = start[lane * 4 + j]);
        uint32_t at = wave_prefix_sum(s) - s;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            start[lane * 4 + j] = at;
            cur[lane * 4 + j] = at;
            at += c[j];
        }
        if (lane == 63) start[256] = at;
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < n;
        const uint32_t w = valid ? in[i] : 0u;
        const uint32_t key = key_of(w);
        uint64_t same = __ballot(valid);  // the valid lanes with this key
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint64_t m = __ballot(valid && ((key >> b) & 1u));
            same &= ((key >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
        uint32_t pos = 0;
        if (valid) pos = cur[key] + rank;
        __syncthreads();  // (every lane read its cursor)
        if (valid) {
            if (pos < (uint32_t)CAP) bk[pos] = w;  // (always: pos < n)
            if (rank == 0) cur[key] += (uint32_t)__popcll(same);
        }
        __syncthreads();
    }
    // the sequential greedy deal, wave-uniform: lane k holds bucket k of the class
    uint16_t *order = reinterpret_cast<uint16_t *>(in);
    uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0, cursor = 0, rp = 0;
    const uint32_t reset = x4 ? 127u : 31u;
    for (int c = 0; c < 8; ++c) {
        uint32_t head = 0, count = 0;
        if (lane < 32) {
            head = start[c * 32 + lane];
            count = start[c * 32 + lane + 1] - head;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)(start[c * 32 + 32] - start[c * 32]));
        uint32_t avail = (uint32_t)__ballot(count > 0);
        for (uint32_t i = 0; i < total && avail; ++i) {  // (avail != 0: the counts add up)
            if ((rp & reset) == 0) u0 = u1 = u2 = u3 = 0;
            const uint32_t slot = x4 ? (rp & 3u) : 0u;
            const uint32_t used = slot == 0 ? u0 : slot == 1 ? u1 : slot == 2 ? u2 : u3;
            uint32_t cand = avail & ~used;
            if (!cand) cand = avail;  // every bank left is taken in this set
            const uint32_t rot = __builtin_rotateright32(cand, cursor);
            const uint32_t k = ((uint32_t)__builtin_ctz(rot) + cursor) & 31u;
            if ((uint32_t)lane == k) {
                if (rp < (uint32_t)CAP) order[rp] = (uint16_t)head;  // (always: rp < n)
                ++head;
                --count;
            }
            avail = (uint32_t)__ballot(count > 0);
            const uint32_t bit = 1u << k;
            u0 |= slot == 0 ? bit : 0u;
            u1 |= slot == 1 ? bit : 0u;
            u2 |= slot == 2 ? bit : 0u;
            u3 |= slot == 3 ? bit : 0u;
            cursor = (k + 1) & 31u;
            ++rp;
        }
        if (cum && lane == 0) cum[c] = (uint16_t)(base + rp);
    }
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
        const uint32_t at = order[j];
        dst[j] = il_encode(bk[at < (uint32_t)CAP ? at : 0]);
    }
    __syncthreads();  // in, bk and the counters are free again
}

// One wave per group.  LONG: group g = (long sublist g / 16, wave segment g % 16), its words
// in segw; else group g = entry g, skipped when it is long, its words the sorted records'.
template <int CAP, bool LONG>
__global__ void __launch_bounds__(64)
il_deal_kernel(const uint4 *__restrict__ src, const uint32_t *__restrict__ segw,
               const uint32_t *__restrict__ segoff, const uint32_t *__restrict__ epos,
               const uint32_t *__restrict__ lid, const uint32_t *__restrict__ long_ent,
               int64_t n_groups, bool x4, uint32_t *__restrict__ post,
               uint32_t *__restrict__ flat, uint16_t *__restrict__ seg,
               uint16_t *__restrict__ wmeta, uint8_t *__restrict__ emax,
               IlCtrl *__restrict__ ctrl) {
    __shared__ uint32_t in[CAP], bk[CAP], start[260], cur[256];
    const int lane = threadIdx.x;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        int64_t o;  // where the group starts in post / flat
        uint32_t n, base = 0;
        uint16_t *cum;
        if (LONG) {
            const int64_t id = g / IL_WSEG;
            const int w = (int)(g % IL_WSEG);
            const uint32_t a = segoff[id * (IL_WSEG + 1) + w];
            o = (int64_t)epos[long_ent[id]] + a;
            n = segoff[id * (IL_WSEG + 1) + w + 1] - a;
            base = a;
            cum = wmeta + id * (IL_WSEG * 8) + w * 8;
        } else {
            if (lid[g] != IL_NO) continue;
            o = epos[g];
            n = epos[g + 1] - epos[g];
            cum = seg + g * 8;
        }
        if (n > (uint32_t)CAP) {  // (documented deviation: DI_EINVAL)
            if (lane == 0) atomicOr(&ctrl->err, IL_ERR_GROUP);
            continue;
        }
        if (!LONG && n == 1) {  // the common sublist of a large vocabulary
            if (lane == 0) {
                const uint32_t w = src[o].x;
                const int c0 = il_cls(w);
                post[o] = il_encode(w);
                if (flat) flat[o] = il_encode(w);
                for (int c = 0; c < 8; ++c) cum[c] = c >= c0 ? 1 : 0;
                emax[g] = (uint8_t)(w & 255u);
            }
            continue;
        }
        auto load = [&] {
            uint32_t mx = 0;
            for (uint32_t i = lane; i < n; i += 64) {
                const uint32_t w = LONG ? segw[o + i] : src[o + i].x;
                in[i] = w;
                mx = max(mx, w & 255u);
            }
            __syncthreads();
            return mx;
        };
        uint32_t mx = load();
        if (!LONG) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
            if (lane == 0) emax[g] = (uint8_t)mx;
        }
        il_deal<CAP>(in, bk, start, cur, (int)n, false, x4, post + o, base, cum);
        if (!flat) continue;
        if (LONG) {
            load();
            il_deal<CAP>(in, bk, start, cur, (int)n, true, x4, flat + o, 0u, nullptr);
        } else {
            for (uint32_t i = lane; i < n; i += 64) flat[o + i] = post[o + i];
        }
    }
}

struct Scratch {
    DevBuf ctrl, zfirst, cnt, off, csum, sort_a, sort_b, head, eterm, long_ent, segoff;
    Timer *timer;
    bool timing;
    hipStream_t s;
};

// off[0, len) = the exclusive scan of cnt[0, len) -> the total (waits for s)
int64_t il_scan(Scratch &k, const uint32_t *cnt, int64_t len, int64_t *off) {
    if (len <= 0) return 0;
    const int64_t n_chunks = (len + IB_SCAN_CHUNK - 1) / IB_SCAN_CHUNK;
    DI_REQUIRE(n_chunks <= (int64_t)INT32_MAX, DI_ERANGE, "too many postings for one scan");
    k.csum.reserve((size_t)(n_chunks + 1) * 8);
    {
        TimedLaunch tl(*k.timer, k.timing, "il_scan", k.s);
        hipLaunchKernelGGL(ib_scan_sum_kernel, dim3((unsigned)n_chunks), dim3(IB_THREADS), 0, k.s,
                           cnt, len, k.csum.as<int64_t>());
        check_launch("ib_scan_sum");
        hipLaunchKernelGGL(ib_scan_chunks_kernel, dim3(1), dim3(IB_THREADS), 0, k.s,
                           k.csum.as<int64_t>(), n_chunks);
        check_launch("ib_scan_chunks");
        hipLaunchKernelGGL(ib_scan_apply_kernel, dim3((unsigned)n_chunks), dim3(IB_THREADS), 0,
                           k.s, cnt, len, k.csum.as<int64_t>(), off);
        check_launch("ib_scan_apply");
    }
    int64_t total = 0;
    read_back(total, k.csum.as<int64_t>() + n_chunks, k.s, k.timer);
    return total;
}

// One stable radix pass src -> dst on the 8-bit digit of .y (the term) or .z (the block).
void il_sort_pass(Scratch &k, const uint4 *src, uint4 *dst, int64_t n, bool on_y, int shift) {
    const int64_t n_tiles = (n + IB_TILE - 1) / IB_TILE, cells = 256 * n_tiles;
    k.cnt.reserve((size_t)cells * 4);
    k.off.reserve((size_t)cells * 8);
    {
        TimedLaunch tl(*k.timer, k.timing, "il_hist", k.s);
        hipLaunchKernelGGL(ib_hist_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0, k.s,
                           src, n, n_tiles, on_y, shift, k.cnt.as<uint32_t>());
        check_launch("il_hist");
    }
    const int64_t total = il_scan(k, k.cnt.as<uint32_t>(), cells, k.off.as<int64_t>());
    DI_REQUIRE(total == n, DI_EHIP, "il_hist counted %lld of %lld postings", (long long)total,
               (long long)n);
    {
        TimedLaunch tl(*k.timer, k.timing, "il_scatter", k.s);
        hipLaunchKernelGGL(ib_scatter_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0, k.s,
                           src, dst, n, n_tiles, on_y, shift, k.off.as<int64_t>(),
                           (const int32_t *)nullptr, (int64_t)0);
        check_launch("il_scatter");
    }
}

int digit_passes(int64_t top) {  // 8-bit digits of the values 0 .. top
    int p = 0;
    for (; top > 0; top >>= 8) ++p;
    return p;
}

void zero_fill(DevBuf &b, size_t bytes, int byte, hipStream_t s) {
    b.reserve(bytes);
    DI_HIP(hipMemsetAsync(b.p, byte, bytes, s));
}

template <int CAP, bool LONG>
void launch_deal(Scratch &k, const uint4 *src, const uint32_t *segw, int64_t n_groups, bool x4,
                 IndexLayout &out, uint32_t *flat) {
    if (n_groups <= 0) return;
    TimedLaunch tl(*k.timer, k.timing, "il_deal", k.s);
    hipLaunchKernelGGL((il_deal_kernel<CAP, LONG>), dim3(grid_for(n_groups, 1)), dim3(64), 0, k.s,
                       src, segw, k.segoff.as<uint32_t>(), out.epos->as<uint32_t>(),
                       out.lid->as<uint32_t>(), k.long_ent.as<uint32_t>(), n_groups, x4,
                       out.post->as<uint32_t>(), flat, out.seg->as<uint16_t>(),
                       out.wmeta->as<uint16_t>(), out.emax->as<uint8_t>(), k.ctrl.as<IlCtrl>());
    check_launch("il_deal");
}

}  // namespace

void build_layout_device(const int64_t *term_off, int64_t n_terms, const uint32_t *pdoc,
                         const uint8_t *pval, uint32_t doc_lo, uint32_t doc_hi, hipStream_t s,
                         bool timing, Timer &timer, IndexLayout &out) {
    DI_REQUIRE(n_terms >= 0, DI_EINVAL, "n_terms < 0");
    DI_REQUIRE(n_terms < (int64_t)0xFFFFFFFF, DI_ERANGE, "n_terms %lld >= 2^32",
               (long long)n_terms);
    Scratch k;
    k.timer = &timer;
    k.timing = timing;
    k.s = s;
    zero_fill(k.ctrl, sizeof(IlCtrl), 0, s);
    IlCtrl *ctrl = k.ctrl.as<IlCtrl>();
    IlCtrl h{};
    {
        TimedLaunch tl(timer, timing, "il_check", s);
        hipLaunchKernelGGL(il_check_kernel, dim3(grid_for(n_terms, IB_THREADS)), dim3(IB_THREADS),
                           0, s, term_off, n_terms, ctrl);
        check_launch("il_check");
    }
    read_back(h, ctrl, s, &timer);
    DI_REQUIRE(!(h.err & IL_ERR_OFF), DI_EINVAL, "term_off[0] < 0 or term_off not monotone");
    IlIn in{term_off, n_terms, pdoc, pval, h.first, h.last - h.first, doc_lo, doc_hi, 0, nullptr};
    const int64_t n = in.n, n_tiles = (n + IB_TILE - 1) / IB_TILE;
    if (n > 0) {
        zero_fill(k.zfirst, (size_t)n_terms * 8, 0xFF, s);
        {
            TimedLaunch tl(timer, timing, "il_input", s);
            hipLaunchKernelGGL(il_input_kernel, dim3(grid_for(n, IB_THREADS * 8)),
                               dim3(IB_THREADS), 0, s, in, k.zfirst.as<unsigned long long>(), ctrl);
            check_launch("il_input");
        }
        read_back(h, ctrl, s, &timer);
        if (h.has_zero) in.zfirst = k.zfirst.as<unsigned long long>();
    }
    if (doc_hi == 0) doc_hi = n > 0 ? h.max_doc + 1 : doc_lo;
    DI_REQUIRE(doc_hi >= doc_lo, DI_EINVAL, "doc_hi < doc_lo");
    const uint32_t nd = doc_hi - doc_lo;
    const int nb = (int)((nd + (uint32_t)IL_BLOCK_DOCS - 1) / IL_BLOCK_DOCS);
    DI_REQUIRE(nb <= 65535, DI_ERANGE, "%u docs in one shard: more than 65535 blocks", nd);
    const uint32_t bd =
        nb ? (uint32_t)std::min<uint64_t>(IL_BLOCK_DOCS, ((nd + nb - 1) / nb + 63) / 64 * 64)
           : (uint32_t)IL_BLOCK_DOCS;
    in.doc_hi = doc_hi;
    in.bd = bd;
    out.n_docs = nd;
    out.doc_lo = doc_lo;
    out.nb = nb;
    out.block_docs = (int)bd;

    // the kept postings as records, in input order
    int64_t total = 0;
    if (n > 0) {
        k.cnt.reserve((size_t)n_tiles * 4);
        k.off.reserve((size_t)n_tiles * 8);
        {
            TimedLaunch tl(timer, timing, "il_count", s);
            hipLaunchKernelGGL(il_count_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0, s,
                               in, n_tiles, k.cnt.as<uint32_t>());
            check_launch("il_count");
        }
        total = il_scan(k, k.cnt.as<uint32_t>(), n_tiles, k.off.as<int64_t>());
        DI_REQUIRE(total >= 0 && total <= n, DI_EHIP, "il_count kept %lld of %lld postings",
                   (long long)total, (long long)n);
    }
    DI_REQUIRE(total < (int64_t)IL_NO, DI_ERANGE,
               "more than 2^32 postings / (term, block) entries in one shard");
    const uint4 *src = nullptr;
    if (total > 0) {
        k.sort_a.reserve((size_t)total * sizeof(uint4));
        // (with one block nothing is sorted: the second buffer only takes il_segment's words)
        k.sort_b.reserve((size_t)total * (nb > 1 ? sizeof(uint4) : sizeof(uint32_t)));
        {
            TimedLaunch tl(timer, timing, "il_compact", s);
            hipLaunchKernelGGL(il_compact_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0,
                               s, in, n_tiles, k.off.as<int64_t>(), total, k.sort_a.as<uint4>());
            check_launch("il_compact");
        }
        // stable by (term, block); with one block the records are in that order already
        src = k.sort_a.as<uint4>();
        if (nb > 1) {
            const int pb = digit_passes(nb - 1), pt = digit_passes(n_terms - 1);
            for (int p = 0; p < pb + pt; ++p) {
                uint4 *dst = (src == k.sort_a.as<uint4>() ? k.sort_b : k.sort_a).as<uint4>();
                il_sort_pass(k, src, dst, total, p >= pb, p >= pb ? 8 * (p - pb) : 8 * p);
                src = dst;
            }
        }
    }
    // the other record buffer: a long sublist's words by wave segment
    uint32_t *segw = (src == k.sort_a.as<uint4>() ? k.sort_b : k.sort_a).as<uint32_t>();

    // entries = the run heads of (term, block)
    int64_t n_ent = 0;
    if (total > 0) {
        k.head.reserve((size_t)total * 4);
        k.off.reserve((size_t)total * 8);
        {
            TimedLaunch tl(timer, timing, "il_heads", s);
            hipLaunchKernelGGL(il_heads_kernel, dim3(grid_for(total, IB_THREADS)), dim3(IB_THREADS),
                               0, s, src, total, k.head.as<uint32_t>());
            check_launch("il_heads");
        }
        n_ent = il_scan(k, k.head.as<uint32_t>(), total, k.off.as<int64_t>());
        DI_REQUIRE(n_ent > 0 && n_ent <= total, DI_EHIP, "il_heads found %lld entries",
                   (long long)n_ent);
    }
    out.n_post = total;
    out.n_ent = n_ent;
    zero_fill(*out.eblk, (size_t)std::max<int64_t>(n_ent, 1) * 2, 0, s);
    zero_fill(*out.epos, ((size_t)n_ent + 1) * 4, 0, s);
    out.tb_start->reserve(((size_t)n_terms + 1) * 4);
    k.eterm.reserve((size_t)std::max<int64_t>(n_ent, 1) * 4);
    if (total > 0) {
        TimedLaunch tl(timer, timing, "il_entries", s);
        hipLaunchKernelGGL(il_entries_kernel, dim3(grid_for(total, IB_THREADS)), dim3(IB_THREADS),
                           0, s, src, total, k.head.as<uint32_t>(), k.off.as<int64_t>(), n_ent,
                           out.eblk->as<uint16_t>(), out.epos->as<uint32_t>(),
                           k.eterm.as<uint32_t>());
        check_launch("il_entries");
    }
    {
        TimedLaunch tl(timer, timing, "il_entries", s);
        hipLaunchKernelGGL(il_tbstart_kernel, dim3(grid_for(n_terms + 1, IB_THREADS)),
                           dim3(IB_THREADS), 0, s, k.eterm.as<uint32_t>(), n_ent, n_terms,
                           out.tb_start->as<uint32_t>());
        check_launch("il_tbstart");
    }

    // long sublists get ids in entry order (DI_WLONG_MIN, as build_index())
    uint32_t wlong_min = IL_WLONG_MIN;
    if (const char *e = std::getenv("DI_WLONG_MIN")) wlong_min = (uint32_t)std::max(1, std::atoi(e));
    bool deal_x4 = true, flat_runs = true;
    if (const char *e = std::getenv("DI_DEAL_X4")) deal_x4 = std::atoi(e) != 0;
    if (const char *e = std::getenv("DI_DEAL_CLASSES")) flat_runs = std::atoi(e) == 0;
    int64_t n_long = 0;
    zero_fill(*out.lid, (size_t)std::max<int64_t>(n_ent, 1) * 4, 0xFF, s);
    if (n_ent > 0) {
        k.long_ent.reserve((size_t)n_ent * 4);
        {
            TimedLaunch tl(timer, timing, "il_long", s);
            hipLaunchKernelGGL(il_long_kernel, dim3(grid_for(n_ent, IB_THREADS)), dim3(IB_THREADS),
                               0, s, out.epos->as<uint32_t>(), n_ent, wlong_min,
                               k.head.as<uint32_t>());
            check_launch("il_long");
        }
        n_long = il_scan(k, k.head.as<uint32_t>(), n_ent, k.off.as<int64_t>());
        DI_REQUIRE(n_long >= 0 && n_long <= n_ent, DI_EHIP, "il_long found %lld long sublists",
                   (long long)n_long);
        TimedLaunch tl(timer, timing, "il_long", s);
        hipLaunchKernelGGL(il_lid_kernel, dim3(grid_for(n_ent, IB_THREADS)), dim3(IB_THREADS), 0, s,
                           k.head.as<uint32_t>(), k.off.as<int64_t>(), n_ent, n_long,
                           out.lid->as<uint32_t>(), k.long_ent.as<uint32_t>());
        check_launch("il_lid");
    }
    out.n_long = n_long;
    out.has_flat = flat_runs;

    // the order inside every sublist, the class offsets and the maxima
    const size_t nl1 = (size_t)std::max<int64_t>(n_long, 1);
    zero_fill(*out.seg, (size_t)std::max<int64_t>(n_ent * 8, 8) * 2, 0, s);
    zero_fill(*out.wmeta, nl1 * IL_WSEG * 8 * 2, 0, s);
    zero_fill(*out.emax, (size_t)std::max<int64_t>(n_ent, 1), 0, s);
    zero_fill(*out.wmax, nl1 * IL_WSEG, 0, s);
    const size_t post_words = (size_t)std::max<int64_t>(total, 4);
    out.post->reserve(post_words * 4);
    if (flat_runs) out.post_flat->reserve(post_words * 4);
    if (total < 4) {  // (the host route's padding: the encoding of the word 0)
        const uint32_t pad[4] = {IL_POST_X, IL_POST_X, IL_POST_X, IL_POST_X};
        DI_HIP(hipMemcpyAsync(out.post->p, pad, 16, hipMemcpyHostToDevice, s));
        if (flat_runs) DI_HIP(hipMemcpyAsync(out.post_flat->p, pad, 16, hipMemcpyHostToDevice, s));
        DI_HIP(hipStreamSynchronize(s));  // (pad is a local)
    }
    uint32_t *flat = flat_runs ? out.post_flat->as<uint32_t>() : nullptr;
    if (n_long > 0) {
        k.segoff.reserve((size_t)n_long * (IL_WSEG + 1) * 4);
        const uint32_t S = (bd + IL_WSEG - 1) / IL_WSEG;
        TimedLaunch tl(timer, timing, "il_segment", s);
        hipLaunchKernelGGL(il_segment_kernel, dim3(grid_for(n_long, 1)), dim3(IB_THREADS), 0, s,
                           src, out.epos->as<uint32_t>(), k.long_ent.as<uint32_t>(), n_long, S,
                           segw, k.segoff.as<uint32_t>(), out.seg->as<uint16_t>(),
                           out.emax->as<uint8_t>(), out.wmax->as<uint8_t>(), ctrl);
        check_launch("il_segment");
    }
    if (n_ent > n_long) {
        if (wlong_min <= (uint32_t)IL_GROUP_SHORT + 1)
            launch_deal<IL_GROUP_SHORT, false>(k, src, segw, n_ent, deal_x4, out, flat);
        else
            launch_deal<IL_GROUP_MAX, false>(k, src, segw, n_ent, deal_x4, out, flat);
    }
    launch_deal<IL_GROUP_MAX, true>(k, src, segw, n_long * IL_WSEG, deal_x4, out, flat);
    read_back(h, ctrl, s, &timer);
    DI_REQUIRE(!(h.err & IL_ERR_GROUP), DI_EINVAL,
               "a group of more than %d postings (a doc repeated inside a term, or DI_WLONG_MIN "
               "above %d): the device layout route does not take it",
               IL_GROUP_MAX, IL_GROUP_MAX + 1);
}

}  // namespace di
