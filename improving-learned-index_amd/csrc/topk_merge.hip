// topk_merge.hip -- merge_topk: one workgroup per query selects the top-k of the
// query's candidate lists (the <= NB * k block candidates of the quantized scorer, the
// float index's block lists, or a caller's lists through di_topk_merge) by the 64-bit key
// word(32) | ~doc(32) and writes doc / score / key.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdlib>

#include "di_common.h"
#include "topk_common.h"
#include "topk_merge.h"

namespace di {

// ---------------------------------------------------------------------------
// merge: per query, the top-k of n_lists candidate lists by 64-bit key
// ---------------------------------------------------------------------------
constexpr int MG_LDS_KEYS = 16384;  // fast path: every candidate fits in LDS

// Selection without a sort (fast path, > MG_SEL_MIN candidates, see the kernel):
// a 4096-bin histogram of the keys' score bits, then counting ranks.
constexpr int MG_SEL_MIN = 1024;
constexpr int MG_SEL_BINS = 4096;   // 16 KiB of LDS after the key array
constexpr int MG_SEL_KEYS = 2048;   // + 16 KiB: up to 2048 selected keys
constexpr int MG_SEL_CAP = 8192;    // key arrays up to 64 KiB (+32 KiB within the LDS max)

template <int THREADS>
struct alignas(16) MergeHead {  // 16-byte multiple: the u64 key array follows it
    RadixScratch<THREADS / 64> rs;
    int32_t off[1025];
    uint32_t cnt;
    int32_t bad;
    uint32_t thr, above;
    uint32_t wtot[THREADS / 64];
};

// keys: the LDS key array holds `cap` entries (power of two, <= MG_LDS_KEYS)
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
merge_topk_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ counts,
                  int n_lists, int k_in, int k, int64_t list_stride, int64_t cnt_stride,
                  int64_t q_stride, int64_t cq_stride, int cap,
                  uint64_t *__restrict__ out_key, uint32_t *__restrict__ out_doc,
                  uint32_t *__restrict__ out_score, int32_t *__restrict__ out_n, int mode,
                  int select, const int32_t *__restrict__ cu_q) {
    // key i of list l of query q: keys[q*q_stride + l*list_stride + i]
    // its count:                  counts[q*cq_stride + l*cnt_stride]
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MergeHead<THREADS> &sh = *reinterpret_cast<MergeHead<THREADS> *>(smem);
    static_assert(sizeof(MergeHead<THREADS>) % 16 == 0, "key array must stay 16-byte aligned");
    uint64_t *lk = reinterpret_cast<uint64_t *>(smem + sizeof(MergeHead<THREADS>));
    const int q = blockIdx.x, tid = threadIdx.x;
    const int32_t *cnt0 = counts + (int64_t)q * cq_stride;
    auto cnt = [&](int l) { return cnt0[(int64_t)l * cnt_stride]; };
    const uint64_t *src0 = keys + (int64_t)q * q_stride;

    if (tid == 0) sh.bad = 0;
    __syncthreads();
    int64_t total = 0;
    const bool fast_lists = n_lists <= 1024;
    if (fast_lists) {
        // list offsets by a block scan (thread t owns lists LPT t .. LPT t + LPT - 1):
        // a serial scan by one thread cost ~10 us per query at 269 lists
        constexpr int LPT = (1024 + THREADS - 1) / THREADS;
        int c[LPT];
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int l = tid * LPT + j;
            c[j] = l < n_lists ? cnt(l) : 0;
            if (c[j] < 0) sh.bad = 1;
            c[j] = min(max(c[j], 0), k_in);
            run += (uint32_t)c[j];
        }
        const uint32_t incl = wave_prefix_sum(run);
        const int lane = tid & 63, w = tid >> 6;
        if (lane == 63) sh.wtot[w] = incl;
        __syncthreads();
        uint32_t base = incl - run;
        for (int v = 0; v < w; ++v) base += sh.wtot[v];
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int l = tid * LPT + j;
            base += (uint32_t)c[j];
            if (l < n_lists) sh.off[l + 1] = (int32_t)base;
        }
        if (tid == 0) sh.off[0] = 0;
        __syncthreads();
        total = sh.off[n_lists];
    } else {
        int64_t part = 0;
        for (int l = tid; l < n_lists; l += THREADS) {
            int c = cnt(l);
            if (c < 0) sh.bad = 1;
            part += min(max(c, 0), k_in);
        }
        if (tid == 0) sh.cnt = 0;
        __syncthreads();
        atomicAdd(&sh.cnt, (uint32_t)part);
        __syncthreads();
        total = sh.cnt;
        __syncthreads();
    }
    if (sh.bad) {
        if (tid == 0) out_n[q] = -1;
        return;
    }
    const int take = (int)min<int64_t>(total, k);
    uint64_t *ok = out_key ? out_key + (int64_t)q * k : nullptr;
    if (fast_lists && total <= cap) {
        // flattened over the lists, 8 loads per lane in flight (clamped addresses:
        // unconditional loads), list of key i by binary search over the offsets
        constexpr int U = 8;
        const int tot = (int)total;
        for (int base = 0; base < tot; base += U * THREADS) {
            uint64_t v[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int i = min(base + j * THREADS + tid, tot - 1);
                int lo = 0, hi = n_lists - 1;  // last list with off[l] <= i
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (sh.off[mid] <= i) lo = mid;
                    else hi = mid - 1;
                }
                v[j] = src0[(int64_t)lo * list_stride + (i - sh.off[lo])];
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int i = base + j * THREADS + tid;
                if (i < tot) lk[i] = v[j];
            }
        }
        __syncthreads();
    }
    // Over the LDS capacity (many lists, e.g. the early blocks of an 8.8 M-doc query
    // emitted full lists before the shared threshold rose): two passes over the lists, a
    // wave per list -- the score histogram of every key, then only the keys in bins at or
    // above the take-th key's bin into LDS -- and the selection below on those.  Every
    // key >= the take-th largest is kept, so the result is the same.  Wide keys (score
    // bits past 4095), or more kept keys than the LDS holds: the radix select below.
    // (select bit 2: on; DI_PROFILE_MERGE=2 turns it off, A/B)
    bool over = !(fast_lists && total <= cap);
    if (over && fast_lists && (select & 2) && cap > MG_SEL_MIN && cap <= MG_SEL_CAP) {
        uint32_t *hist = reinterpret_cast<uint32_t *>(lk + cap);
        auto bin = [](uint64_t x) { return (uint32_t)(x >> 48) & (MG_SEL_BINS - 1); };
        for (int i = tid; i < MG_SEL_BINS; i += THREADS) hist[i] = 0;
        if (tid == 0) sh.cnt = 0;
        __syncthreads();
        const int lane = tid & 63, w = tid >> 6;
        constexpr int UL = 4;  // loads per lane in flight
        bool big = false;
        for (int l = w; l < n_lists; l += WAVES) {
            const int o = sh.off[l], c = sh.off[l + 1] - o;
            const uint64_t *src = src0 + (int64_t)l * list_stride;
            for (int i0 = 0; i0 < c; i0 += UL * 64) {
                uint64_t v[UL];
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    const int i = i0 + u * 64 + lane;
                    v[u] = i < c ? src[i] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < UL; ++u) {
                    if (i0 + u * 64 + lane < c) {
                        big |= (v[u] >> 60) != 0;
                        atomicAdd(&hist[bin(v[u])], 1u);
                    }
                }
            }
        }
        if (!__syncthreads_or(big)) {
            // T = the bin of the take-th largest key, n_keep = the keys in bins >= T
            constexpr int BPT = MG_SEL_BINS / THREADS;
            const int top = MG_SEL_BINS - 1 - tid * BPT;
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j) c += hist[top - j];
            const uint32_t incl = wave_prefix_sum(c);
            if (lane == 63) sh.wtot[w] = incl;
            __syncthreads();
            uint32_t run = incl - c;
            for (int v = 0; v < w; ++v) run += sh.wtot[v];
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                const uint32_t h = hist[top - j];
                if (run < (uint32_t)take && run + h >= (uint32_t)take) {
                    sh.thr = (uint32_t)(top - j);
                    sh.above = run + h;
                }
                run += h;
            }
            __syncthreads();
            const uint32_t T = sh.thr, n_keep = sh.above;
            if (n_keep <= (uint32_t)cap) {
                for (int l = w; l < n_lists; l += WAVES) {
                    const int o = sh.off[l], c2 = sh.off[l + 1] - o;
                    const uint64_t *src = src0 + (int64_t)l * list_stride;
                    for (int i0 = 0; i0 < c2; i0 += UL * 64) {
                        uint64_t v[UL];
#pragma unroll
                        for (int u = 0; u < UL; ++u) {
                            const int i = i0 + u * 64 + lane;
                            v[u] = i < c2 ? src[i] : 0ull;
                        }
#pragma unroll
                        for (int u = 0; u < UL; ++u) {
                            uint32_t pos;
                            const bool keep = i0 + u * 64 + lane < c2 && bin(v[u]) >= T;
                            if (wave_append(keep, &sh.cnt, pos)) lk[pos] = v[u];
                        }
                    }
                }
                __syncthreads();
                total = n_keep;
                over = false;
            }
        }
        __syncthreads();  // (the histogram area is reused by the selection)
    }
    if (over) {
        // slow path: radix select the take-th largest key straight from global
        uint64_t prefix = 0, mask = 0;
        uint32_t need = (uint32_t)take;
        for (int shift = 56; shift >= 0; shift -= 8) {
            radix_clear<THREADS, WAVES>(sh.rs);
            __syncthreads();
            RunLen rl;
            for (int l = 0; l < n_lists; ++l) {
                int c = min(cnt(l), k_in);
                const uint64_t *s = src0 + (int64_t)l * list_stride;
                for (int i = tid; i < c; i += THREADS) {
                    uint64_t x = s[i];
                    if ((x & mask) == prefix) rl.add(sh.rs, (uint32_t)(x >> shift) & 255u);
                }
            }
            rl.flush(sh.rs);
            __syncthreads();
            radix_pick<THREADS, WAVES>(sh.rs, need);
            prefix |= (uint64_t)sh.rs.bin << shift;
            mask |= (uint64_t)255 << shift;
            need -= sh.rs.above;
            __syncthreads();
        }
        // keys are unique: exactly `take` keys are >= prefix
        if (tid == 0) sh.cnt = 0;
        __syncthreads();
        for (int l = 0; l < n_lists; ++l) {
            int c = min(cnt(l), k_in);
            const uint64_t *s = src0 + (int64_t)l * list_stride;
            for (int i = tid; i < c; i += THREADS) {
                uint64_t x = s[i];
                if (x >= prefix) {
                    uint32_t pos = atomicAdd(&sh.cnt, 1u);
                    if (pos < (uint32_t)cap) lk[pos] = x;
                }
            }
        }
        __syncthreads();
        total = take;
    }
    // a long query's keys are wide (score_long_item)
    const bool wide = mode == DECODE_QUANT && cu_q && cu_q[q + 1] - cu_q[q] > DI_SHORT_QUERY_TERMS;
    auto emit = [&](int i, uint64_t x) {  // output rank i
        if (ok) ok[i] = x;
        if (mode == DECODE_QUANT) {
            out_doc[(int64_t)q * k + i] =
                wide ? 0xFFFFFFu - (uint32_t)(x & 0xFFFFFFu) : 0xFFFFFFFFu - (uint32_t)x;
            out_score[(int64_t)q * k + i] = (uint32_t)(x >> (wide ? 44 : 48));
        } else if (mode == DECODE_SPARSE) {
            out_doc[(int64_t)q * k + i] = 0xFFFFFFu - (uint32_t)(x & 0xFFFFFFu);
            out_score[(int64_t)q * k + i] = (uint32_t)(x >> 32);  // f32 bits
        }
    };
    if (select && fast_lists && total > MG_SEL_MIN && cap <= MG_SEL_CAP && take < total) {
        // Selection by counting instead of a sort.  Every key below 2^60 (score <
        // 4096)?  Then bin = key bits 48..59 (the score) orders the keys up to ties
        // inside a bin: a histogram gives the bin T of the take-th largest key and
        // every bin's start rank; the keys of bins >= T are placed bin by bin, and a
        // key's rank is its bin's start + the keys of its own bin that are larger.
        bool big = false;
        for (int i = tid; i < total; i += THREADS) big |= (lk[i] >> 60) != 0;
        if (!__syncthreads_or(big)) {
            uint32_t *hist = reinterpret_cast<uint32_t *>(lk + cap);
            uint64_t *out = reinterpret_cast<uint64_t *>(hist + MG_SEL_BINS);
            auto bin = [](uint64_t x) { return (uint32_t)(x >> 48) & (MG_SEL_BINS - 1); };
            for (int i = tid; i < MG_SEL_BINS; i += THREADS) hist[i] = 0;
            __syncthreads();
            for (int i = tid; i < total; i += THREADS) atomicAdd(&hist[bin(lk[i])], 1u);
            __syncthreads();
            // thread t owns BPT consecutive bins from the top, in descending order
            constexpr int BPT = MG_SEL_BINS / THREADS;
            const int top = MG_SEL_BINS - 1 - tid * BPT;
            uint32_t hc[BPT], c = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j) c += (hc[j] = hist[top - j]);
            const uint32_t incl = wave_prefix_sum(c);
            const int lane = tid & 63, w = tid >> 6;
            if (lane == 63) sh.wtot[w] = incl;
            __syncthreads();
            uint32_t run = incl - c;
            for (int v = 0; v < w; ++v) run += sh.wtot[v];
            // counts -> start ranks (keys in higher bins); T = the take-th key's bin
#pragma unroll
            for (int j = 0; j < BPT; ++j) {
                if (run < (uint32_t)take && run + hc[j] >= (uint32_t)take) {
                    sh.thr = (uint32_t)(top - j);
                    sh.above = run + hc[j];  // keys in bins >= T
                }
                hist[top - j] = run;
                run += hc[j];
            }
            __syncthreads();
            const uint32_t T = sh.thr, n_sel = sh.above;
            if (n_sel <= (uint32_t)MG_SEL_KEYS) {
                // place (hist[b] becomes the end of bin b = the start of bin b - 1)
                for (int i = tid; i < total; i += THREADS) {
                    const uint64_t x = lk[i];
                    const uint32_t b = bin(x);
                    if (b >= T) out[atomicAdd(&hist[b], 1u)] = x;
                }
                __syncthreads();
                for (int p = tid; p < (int)n_sel; p += THREADS) {
                    const uint64_t x = out[p];
                    const uint32_t b = bin(x);
                    const uint32_t lo = b == MG_SEL_BINS - 1 ? 0u : hist[b + 1], hi = hist[b];
                    uint32_t r = lo;
                    for (uint32_t j = lo; j < hi; ++j) r += out[j] > x;
                    if (r < (uint32_t)take) emit((int)r, x);
                }
                if (tid == 0) out_n[q] = take;
                return;
            }
            __syncthreads();  // (the sort below reuses nothing of this)
        }
    }
    int n2 = 64;
    while (n2 < total) n2 <<= 1;
    for (int i = (int)total + tid; i < n2; i += THREADS) lk[i] = 0;
    __syncthreads();
    bitonic_sort_desc<THREADS>(lk, n2);
    for (int i = tid; i < take; i += THREADS) emit(i, lk[i]);
    if (tid == 0) out_n[q] = take;
}

// Merge of few short lists (n_lists <= MS_LISTS, all candidates <= MS_U per thread,
// k <= MG_SEL_KEYS; the 4-block x 1000-candidate retrieve merge): the candidates stay
// in registers (MS_U per thread), the score histogram and the selected keys are the
// only LDS -- 33 KiB instead of the general kernel's 77 KiB, so four workgroups share
// a CU instead of two.  Same selection as merge_topk_kernel's counting path; keys at or
// past score 4096 (wide keys), more than MG_SEL_KEYS selected keys or at most
// MG_SEL_MIN candidates take a radix select over the registers and a sort of the take
// winners in the same LDS.  Output identical to merge_topk_kernel (the keys are unique
// and totally ordered).
constexpr int MS_LISTS = 64;  // (MS_U: candidates per thread, 8, or 16 for the few-block
                               // emit-above lists of up to 2 k keys)

template <int THREADS>
struct alignas(16) MergeSelHead {
    union {
        RadixScratch<THREADS / 64> rs;
        uint32_t hist[MG_SEL_BINS];
    } u;
    int32_t off[MS_LISTS + 1];
    uint32_t thr, above, cnt, pad;
};

template <int THREADS, int MS_U = 8>
__global__ void __launch_bounds__(THREADS)
merge_sel_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ counts,
                 int n_lists, int k_in, int k, int64_t list_stride, int64_t cnt_stride,
                 int64_t q_stride, int64_t cq_stride, uint64_t *__restrict__ out_key,
                 uint32_t *__restrict__ out_doc, uint32_t *__restrict__ out_score,
                 int32_t *__restrict__ out_n, int mode, const int32_t *__restrict__ cu_q) {
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MergeSelHead<THREADS> &sh = *reinterpret_cast<MergeSelHead<THREADS> *>(smem);
    static_assert(sizeof(MergeSelHead<THREADS>) % 16 == 0, "key array must stay 16-byte aligned");
    uint64_t *out = reinterpret_cast<uint64_t *>(smem + sizeof(MergeSelHead<THREADS>));
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int32_t *cnt0 = counts + (int64_t)q * cq_stride;
    const uint64_t *src0 = keys + (int64_t)q * q_stride;

    // list offsets (one wave; n_lists <= 64); a negative count marks a rejected query
    if (tid < 64) {
        int c = lane < n_lists ? cnt0[(int64_t)lane * cnt_stride] : 0;
        const bool bad = __any(c < 0);
        c = min(max(c, 0), k_in);
        const uint32_t incl = wave_prefix_sum((uint32_t)c);
        if (lane < n_lists) sh.off[lane + 1] = (int32_t)incl;
        if (lane == 0) {
            sh.off[0] = 0;
            sh.cnt = bad ? 1u : 0u;
        }
    }
    __syncthreads();
    if (sh.cnt) {
        if (tid == 0) out_n[q] = -1;
        return;
    }
    const int total = sh.off[n_lists];
    const int take = min(total, k);
    // the candidates, MS_U per thread (i = j THREADS + tid), in registers
    uint64_t v[MS_U];
#pragma unroll
    for (int j = 0; j < MS_U; ++j) {
        const int i = min(j * THREADS + tid, max(total - 1, 0));
        int lo = 0, hi = n_lists - 1;  // last list with off[l] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sh.off[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        v[j] = total > 0 ? src0[(int64_t)lo * list_stride + (i - sh.off[lo])] : 0;
    }
    auto valid = [&](int j) { return j * THREADS + tid < total; };
    const bool wide = mode == DECODE_QUANT && cu_q && cu_q[q + 1] - cu_q[q] > DI_SHORT_QUERY_TERMS;
    uint64_t *ok = out_key ? out_key + (int64_t)q * k : nullptr;
    auto emit = [&](int i, uint64_t x) {  // output rank i
        if (ok) ok[i] = x;
        if (mode == DECODE_QUANT) {
            out_doc[(int64_t)q * k + i] =
                wide ? 0xFFFFFFu - (uint32_t)(x & 0xFFFFFFu) : 0xFFFFFFFFu - (uint32_t)x;
            out_score[(int64_t)q * k + i] = (uint32_t)(x >> (wide ? 44 : 48));
        } else if (mode == DECODE_SPARSE) {
            out_doc[(int64_t)q * k + i] = 0xFFFFFFu - (uint32_t)(x & 0xFFFFFFu);
            out_score[(int64_t)q * k + i] = (uint32_t)(x >> 32);  // f32 bits
        }
    };
    bool big = false;
#pragma unroll
    for (int j = 0; j < MS_U; ++j) big |= valid(j) && (v[j] >> 60) != 0;
    const bool counting = !__syncthreads_or(big) && total > MG_SEL_MIN && take < total;
    if (counting) {
        // counting selection (merge_topk_kernel's): bin = key bits 48..59 (the score)
        uint32_t *hist = sh.u.hist;
        auto bin = [](uint64_t x) { return (uint32_t)(x >> 48) & (MG_SEL_BINS - 1); };
        for (int i = tid; i < MG_SEL_BINS; i += THREADS) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MS_U; ++j)
            if (valid(j)) atomicAdd(&hist[bin(v[j])], 1u);
        __syncthreads();
        constexpr int BPT = MG_SEL_BINS / THREADS;
        const int top = MG_SEL_BINS - 1 - tid * BPT;
        uint32_t hc[BPT], c = 0;
#pragma unroll
        for (int j = 0; j < BPT; ++j) c += (hc[j] = hist[top - j]);
        const uint32_t incl = wave_prefix_sum(c);
        const int w = tid >> 6;
        __syncthreads();  // (every thread read its bins; the wave totals go to off's tail)
        uint32_t *wtot = reinterpret_cast<uint32_t *>(out);  // (out is idle until placing)
        if (lane == 63) wtot[w] = incl;
        __syncthreads();
        uint32_t run = incl - c;
        for (int u = 0; u < w; ++u) run += wtot[u];
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            if (run < (uint32_t)take && run + hc[j] >= (uint32_t)take) {
                sh.thr = (uint32_t)(top - j);
                sh.above = run + hc[j];  // keys in bins >= T
            }
            hist[top - j] = run;
            run += hc[j];
        }
        __syncthreads();
        const uint32_t T = sh.thr, n_sel = sh.above;
        if (n_sel <= (uint32_t)MG_SEL_KEYS) {
#pragma unroll
            for (int j = 0; j < MS_U; ++j)
                if (valid(j) && bin(v[j]) >= T) out[atomicAdd(&hist[bin(v[j])], 1u)] = v[j];
            __syncthreads();
            for (int p = tid; p < (int)n_sel; p += THREADS) {
                const uint64_t x = out[p];
                const uint32_t b = bin(x);
                const uint32_t lo = b == MG_SEL_BINS - 1 ? 0u : hist[b + 1], hi = hist[b];
                uint32_t r = lo;
                for (uint32_t j = lo; j < hi; ++j) r += out[j] > x;
                if (r < (uint32_t)take) emit((int)r, x);
            }
            if (tid == 0) out_n[q] = take;
            return;
        }
        __syncthreads();  // (the radix select below reuses the histogram's LDS)
    }
    // radix select of the take-th largest key over the registers, then the take winners
    // (keys are unique: exactly `take` are >= the selected prefix) sorted in LDS
    uint64_t prefix = 0, mask = 0;
    uint32_t need = (uint32_t)take;
    if (take < total) {
        for (int shift = 56; shift >= 0; shift -= 8) {
            radix_clear<THREADS, WAVES>(sh.u.rs);
            __syncthreads();
            RunLen rl;
#pragma unroll
            for (int j = 0; j < MS_U; ++j)
                if (valid(j) && (v[j] & mask) == prefix)
                    rl.add(sh.u.rs, (uint32_t)(v[j] >> shift) & 255u);
            rl.flush(sh.u.rs);
            __syncthreads();
            radix_pick<THREADS, WAVES>(sh.u.rs, need);
            prefix |= (uint64_t)sh.u.rs.bin << shift;
            mask |= (uint64_t)255 << shift;
            need -= sh.u.rs.above;
            __syncthreads();
        }
    }
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MS_U; ++j)
        if (valid(j) && v[j] >= prefix) out[atomicAdd(&sh.cnt, 1u)] = v[j];
    int n2 = 64;
    while (n2 < take) n2 <<= 1;
    __syncthreads();
    for (int i = take + tid; i < n2; i += THREADS) out[i] = 0;
    __syncthreads();
    bitonic_sort_desc<THREADS>(out, n2);
    for (int i = tid; i < take; i += THREADS) emit(i, out[i]);
    if (tid == 0) out_n[q] = take;
}

// Kernels using more than 64 KiB of dynamic LDS must opt in: once per process and device.
static void enable_merge_lds() {
    static std::atomic<uint64_t> set_on{0};
    dynamic_lds_once(
        set_on,
        {{(const void *)merge_topk_kernel<256>, (int)(sizeof(MergeHead<256>) + MG_LDS_KEYS * 8)},
         {(const void *)merge_topk_kernel<512>, (int)(sizeof(MergeHead<512>) + MG_LDS_KEYS * 8)},
         {(const void *)merge_sel_kernel<512, 16>, (int)(sizeof(MergeSelHead<512>) + MG_SEL_KEYS * 8)},
         {(const void *)merge_sel_kernel<512>, (int)(sizeof(MergeSelHead<512>) + MG_SEL_KEYS * 8)}});
}

void launch_merge(const uint64_t *keys, const int32_t *counts, int n_q, int n_lists, int k_in,
                  int k, uint64_t *out_key, uint32_t *out_doc, uint32_t *out_score,
                  int32_t *out_n, int mode, hipStream_t s, bool lists_major,
                  const int32_t *cu_q) {
    if (n_q == 0) return;
    enable_merge_lds();
    int64_t ls = k_in, cs = 1, qs = (int64_t)n_lists * k_in, cqs = n_lists;
    if (lists_major) {
        ls = (int64_t)n_q * k_in;
        cs = n_q;
        qs = k_in;
        cqs = 1;
    }
    // few short lists: the register-resident merge (DI_PROFILE_MERGE=0: the general one, A/B)
    // (DI_PROFILE_MERGE=2: the radix select for candidates past the LDS capacity instead
    // of the two-pass histogram filter, A/B)
    static const bool sel_ok = [] {
        const char *e = std::getenv("DI_PROFILE_MERGE");
        return !(e && e[0] == '0');
    }();
    static const int two_pass = [] {
        const char *e = std::getenv("DI_PROFILE_MERGE");
        return (e && e[0] == '2') ? 0 : 2;
    }();
    if (sel_ok && n_lists <= MS_LISTS && (int64_t)n_lists * k_in <= (int64_t)16 * 512 &&
        k <= MG_SEL_KEYS) {
        auto kern = (int64_t)n_lists * k_in <= (int64_t)8 * 512 ? merge_sel_kernel<512, 8>
                                                                : merge_sel_kernel<512, 16>;
        hipLaunchKernelGGL(kern, dim3(n_q), dim3(512),
                           sizeof(MergeSelHead<512>) + (size_t)MG_SEL_KEYS * 8, s, keys, counts,
                           n_lists, k_in, k, ls, cs, qs, cqs, out_key, out_doc, out_score, out_n,
                           mode, cu_q);
        check_launch("merge_sel");
        return;
    }
    // LDS key capacity: all candidates when they fit, else the k survivors of the
    // slow path's radix select
    // (many lists: the score_blocks shared threshold leaves ~k + a few candidates per
    // query, so an 8192-key array -- the selection path's maximum -- usually holds them)
    // (DI_MERGE_CAP: the LDS key array past MG_LDS_KEYS candidates, A/B; default
    // MG_SEL_CAP)
    static const int64_t over_cap = [] {
        const char *e = std::getenv("DI_MERGE_CAP");
        return e ? std::max<int64_t>(64, std::atoll(e)) : (int64_t)MG_SEL_CAP;
    }();
    int64_t want = (int64_t)n_lists * k_in;
    if (n_lists > 1024 || want > MG_LDS_KEYS) want = std::max<int64_t>(k, over_cap);
    int cap = 64;
    while (cap < want) cap <<= 1;
    // workgroup size of the merge: 512 measured best for the 4-block x 1000-candidate
    // bench merge (0.68 vs 0.73 ms at 1024, 0.86 at 256; small arrays keep 256);
    // score-histogram selection before the sort (a full sort of 4000 candidates took
    // 0.80 ms, selection 0.17)
    const int select = 1 | two_pass;
    // (the histogram follows the keys; only for cap <= MG_SEL_CAP, inside the attribute's max)
    const size_t sel_lds = cap > MG_SEL_MIN && cap <= MG_SEL_CAP ? (size_t)MG_SEL_BINS * 4 + MG_SEL_KEYS * 8 : 0;
    if (cap <= 256) {
        size_t lds = sizeof(MergeHead<256>) + (size_t)cap * 8 + sel_lds;
        hipLaunchKernelGGL(merge_topk_kernel<256>, dim3(n_q), dim3(256), lds, s, keys, counts,
                           n_lists, k_in, k, ls, cs, qs, cqs, cap, out_key, out_doc, out_score,
                           out_n, mode, select, cu_q);
    } else {
        size_t lds = sizeof(MergeHead<512>) + (size_t)cap * 8 + sel_lds;
        hipLaunchKernelGGL(merge_topk_kernel<512>, dim3(n_q), dim3(512), lds, s, keys, counts,
                           n_lists, k_in, k, ls, cs, qs, cqs, cap, out_key, out_doc, out_score,
                           out_n, mode, select, cu_q);
    }
    check_launch("merge_topk");
}

}  // namespace di

using namespace di;

extern "C" {

int di_topk_merge(const uint64_t *keys, const int32_t *counts, int32_t n_q, int32_t n_lists,
                  int32_t k, uint64_t *out_key, int32_t *out_n, int device, void *hip_stream,
                  uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(keys && counts && out_key && out_n && n_q >= 0 && n_lists > 0, DI_EINVAL,
                   "bad argument");
        DI_REQUIRE(k > 0 && k <= DI_MAX_TOPK, DI_ERANGE, "k=%d outside [1, %d]", k,
                   DI_MAX_TOPK);
        DeviceScope ds(device);
        hipStream_t s = (hipStream_t)hip_stream;
        const bool dev = flags & DI_F_DEVICE_PTRS;
        DevBuf bk, bc, bo, bn;
        const uint64_t *dk = stage_in(keys, (size_t)n_q * n_lists * k, dev, bk, s);
        const int32_t *dc = stage_in(counts, (size_t)n_q * n_lists, dev, bc, s);
        StagedOut<uint64_t> ok(out_key, (size_t)n_q * k, dev, bo);
        StagedOut<int32_t> on(out_n, (size_t)n_q, dev, bn);
        launch_merge(dk, dc, n_q, n_lists, k, k, ok.d, nullptr, nullptr, on.d, DECODE_NONE, s,
                     (flags & DI_F_LISTS_MAJOR) != 0);
        ok.copy_back(s);
        on.copy_back(s);
        if (!(flags & DI_F_ASYNC) || !dev) DI_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"
