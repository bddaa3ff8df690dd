// pair_order.hip -- the entry order of DeepPairwiseImpact on the device, gfx950.
//
// Replaces, for a packed batch, the host ordering of
//   DeepPairwiseImpact.compute_term_impacts   src/deep_impact/models/pairwise_impact.py:98-129
// per document: its T terms (position = the term's place in the map) and the pairs whose
// score does not round to 0.000 (position T + j, j the pair's index in
// itertools.combinations order), sorted by raw score descending, equal scores by position.
//
// Every entry is one 64-bit key
//   order-preserving score bits (as segment_order_kernel) << 32 | ~(position << 11 | r)
// (r: a single's rank among the sorted terms, 0 for a pair), so keys are unique, a plain
// descending sort is the stable order, and a sorted key names its entry.  Three passes:
//   pair_count   entries per document (pair_count_kernel), offsets and the routes'
//                work lists (pair_scan_kernel)
//   pair_order   LDS route: one workgroup builds, sorts (bitonic_sort_desc) and writes a
//                document of up to DI_PAIR_ORDER_LDS_KEYS entries; large route: the keys
//                go to a global scratch and are sorted in runs of that many
//   pair_merge   large route: merge passes over ping-pong buffers (merge-path partition,
//                8 outputs per thread) until one run is left, then the entries
// The scores are read again from the inputs when an entry is written: the key folds -0.0
// into +0.0, the output keeps the bits.
#include <hip/hip_runtime.h>

#include "di_common.h"
#include "pair_order.h"
#include "topk_common.h"

namespace di {

namespace {

constexpr int PO_LDS_KEYS = DI_PAIR_ORDER_LDS_KEYS;  // keys of one LDS sort (128 KiB)
constexpr int PO_SMALL_KEYS = 2048;                  // documents up to here: 256 threads
constexpr int PO_SMALL_THREADS = 256, PO_BIG_THREADS = 1024;
constexpr int PO_MAX_T = DI_PAIR_ORDER_MAX_TERMS;  // 11 bits of r, 21 bits of position
constexpr int PO_ITEMS = 8, PO_MERGE_THREADS = 256, PO_TILE = PO_ITEMS * PO_MERGE_THREADS;
static_assert(PO_LDS_KEYS % PO_TILE == 0, "a merge tile must not straddle two runs");
static_assert((int64_t)PO_MAX_T * (PO_MAX_T + 1) / 2 < (1ll << 21), "position bits");

constexpr int ERR_CU = 1, ERR_POS = 2;
// info words of pair_scan_kernel
enum {
    PO_N_OUT, PO_N_SMALL, PO_N_MID, PO_N_LARGE, PO_KEYS, PO_RUNS, PO_TILES, PO_MAX_RUNS, PO_INFO
};

// numpy's round(np.float32, 3), as enc_pairwise.hip
__device__ __forceinline__ float po_round3(float x) {
    return __fdiv_rn(rintf(__fmul_rn(x, 1000.0f)), 1000.0f);
}
__device__ __forceinline__ bool po_kept(float x) { return po_round3(x) != 0.0f; }

__device__ __forceinline__ uint32_t po_score_bits(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0) u = 0;  // -0.0 == +0.0 (on the bits: denormals stay apart)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t po_key(float x, uint32_t pos, uint32_t r) {
    return ((uint64_t)po_score_bits(x) << 32) | (uint32_t)~((pos << 11) | r);
}

// One document's arrays.
struct PoDoc {
    int t0, T;
    int64_t p0, P;
};
__device__ __forceinline__ PoDoc po_doc(const int32_t *cu_terms, const int64_t *cu_pairs, int d) {
    PoDoc x;
    x.t0 = cu_terms[d];
    x.T = cu_terms[d + 1] - x.t0;
    x.p0 = cu_pairs[d];
    x.P = (int64_t)x.T * (x.T - 1) / 2;
    return x;
}

// Entries per document: T + the kept pairs.  One workgroup per document.  Checks the
// offsets as di_encode_pairwise does (a violation sets an error bit, gives the document
// no entries, and the later kernels do nothing).
__global__ void __launch_bounds__(256)
pair_count_kernel(const float *__restrict__ pair, const int32_t *__restrict__ cu_terms,
                  const int64_t *__restrict__ cu_pairs, const int32_t *__restrict__ single_pos,
                  int n_docs, int64_t n_terms, int64_t n_pairs, int32_t *__restrict__ cnt,
                  int32_t *__restrict__ err) {
    __shared__ uint32_t part[4];
    __shared__ uint32_t bad_pos;
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = cu_terms[d], t1 = cu_terms[d + 1], T = t1 - t0;
    const int64_t p0 = cu_pairs[d], p1 = cu_pairs[d + 1];
    int bad = 0;
    if (t0 < 0 || T < 0 || t1 > n_terms || T > PO_MAX_T || p0 < 0 || p1 > n_pairs ||
        p1 - p0 != T * (T - 1) / 2)
        bad = ERR_CU;
    if (d == 0 && (t0 != 0 || p0 != 0)) bad = ERR_CU;
    if (d == n_docs - 1 && (t1 != n_terms || p1 != n_pairs)) bad = ERR_CU;
    if (tid == 0) bad_pos = 0;
    __syncthreads();
    if (bad) {  // (the same for every thread of the workgroup)
        if (tid == 0) {
            atomicOr(err, bad);
            cnt[d] = 0;
        }
        return;
    }
    if (single_pos)
        for (int r = tid; r < T; r += 256) {
            const int32_t p = single_pos[t0 + r];
            if (p < 0 || p >= T) bad_pos = 1;
        }
    const int64_t P = p1 - p0;
    uint32_t c = 0;
    for (int64_t i = tid; i < P; i += 256) c += po_kept(pair[p0 + i]) ? 1u : 0u;
    c = wave_sum(c);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        if (bad_pos) atomicOr(err, ERR_POS);
        cnt[d] = bad_pos ? 0 : (int32_t)(T + part[0] + part[1] + part[2] + part[3]);
    }
}

__device__ __forceinline__ int po_runs(int64_t n) {
    return (int)((n + PO_LDS_KEYS - 1) / PO_LDS_KEYS);
}
__device__ __forceinline__ int64_t po_tiles(int64_t n) { return (n + PO_TILE - 1) / PO_TILE; }

// Offsets of the documents' entries and the large route's work lists.  One workgroup;
// thread t owns a contiguous run of documents (as pair_prep_kernel).
__global__ void __launch_bounds__(256)
pair_scan_kernel(const int32_t *__restrict__ cnt, int n_docs, int64_t *__restrict__ out_cu,
                 int64_t *__restrict__ info, int32_t *__restrict__ ldoc,
                 int64_t *__restrict__ lkey, int64_t *__restrict__ lrun,
                 int64_t *__restrict__ ltile) {
    __shared__ int64_t part[PO_INFO][256];
    const int t = threadIdx.x;
    const int d0 = (int)((int64_t)n_docs * t / 256), d1 = (int)((int64_t)n_docs * (t + 1) / 256);
    int64_t v[PO_INFO] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int d = d0; d < d1; ++d) {
        const int64_t n = cnt[d];
        v[PO_N_OUT] += n;
        if (n <= PO_SMALL_KEYS) {
            v[PO_N_SMALL] += 1;
        } else if (n <= PO_LDS_KEYS) {
            v[PO_N_MID] += 1;
        } else {
            v[PO_N_LARGE] += 1;
            v[PO_KEYS] += n;
            v[PO_RUNS] += po_runs(n);
            v[PO_TILES] += po_tiles(n);
            v[PO_MAX_RUNS] = max(v[PO_MAX_RUNS], (int64_t)po_runs(n));
        }
    }
    for (int k = 0; k < PO_INFO; ++k) part[k][t] = v[k];
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < PO_INFO; ++k) {
            int64_t run = 0;
            for (int i = 0; i < 256; ++i) {
                const int64_t x = part[k][i];
                if (k == PO_MAX_RUNS) {
                    run = max(run, x);
                } else {
                    part[k][i] = run;
                    run += x;
                }
            }
            info[k] = run;
        }
        const int64_t nl = info[PO_N_LARGE];
        out_cu[n_docs] = info[PO_N_OUT];
        lkey[nl] = info[PO_KEYS];
        lrun[nl] = info[PO_RUNS];
        ltile[nl] = info[PO_TILES];
    }
    __syncthreads();
    int64_t at = part[PO_N_OUT][t], li = part[PO_N_LARGE][t], k0 = part[PO_KEYS][t],
            r0 = part[PO_RUNS][t], l0 = part[PO_TILES][t];
    for (int d = d0; d < d1; ++d) {
        const int64_t n = cnt[d];
        out_cu[d] = at;
        at += n;
        if (n > PO_LDS_KEYS) {
            ldoc[li] = d;
            lkey[li] = k0;
            lrun[li] = r0;
            ltile[li] = l0;
            ++li;
            k0 += n;
            r0 += po_runs(n);
            l0 += po_tiles(n);
        }
    }
}

// The slot of a kept element in an array that `*counter` (LDS) appends to: one atomic
// per wave.  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t po_append(bool keep, uint32_t *counter) {
    const uint64_t mask = __ballot(keep);
    const int lane = lane_id();
    uint32_t base = 0;
    if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
        base = __shfl(base, leader, 64);
    }
    return base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// The keys of document x into dst[0 .. n): singles at [0, T), kept pairs appended in any
// order (the key carries the position).  *counter (LDS) must be T at entry, behind a
// barrier.  Nothing is written at or beyond n.
template <int THREADS>
__device__ __forceinline__ void po_build_keys(const PoDoc &x, const float *__restrict__ single,
                                              const float *__restrict__ pair,
                                              const int32_t *__restrict__ single_pos,
                                              uint64_t *dst, uint32_t n, uint32_t *counter) {
    const int tid = threadIdx.x;
    for (int r = tid; r < x.T; r += THREADS) {
        const uint32_t pos = single_pos ? (uint32_t)single_pos[x.t0 + r] : (uint32_t)r;
        if ((uint32_t)r < n) dst[r] = po_key(single[x.t0 + r], pos, (uint32_t)r);
    }
    for (int64_t base = 0; base < x.P; base += THREADS) {
        const int64_t j = base + tid;
        float v = 0.f;
        bool keep = false;
        if (j < x.P) {
            v = pair[x.p0 + j];
            keep = po_kept(v);
        }
        const uint32_t slot = po_append(keep, counter);
        if (keep && slot < n) dst[slot] = po_key(v, (uint32_t)(x.T + j), 0u);
    }
}

// Entry of a sorted key -> out_first / out_second / out_score[at].  (a, b) of a pair's
// index j = a (2T - a - 1) / 2 + (b - a - 1): a float root, corrected by at most one step
// either way on the integers (as pair_score_kernel).
__device__ __forceinline__ void po_emit(uint64_t key, const PoDoc &x,
                                        const float *__restrict__ single,
                                        const float *__restrict__ pair, int do_round, int64_t at,
                                        int32_t *__restrict__ out_first,
                                        int32_t *__restrict__ out_second,
                                        float *__restrict__ out_score) {
    const uint32_t low = ~(uint32_t)key;
    const int64_t pos = low >> 11;
    int32_t f = -1, g = -1;
    float v = 0.f;
    if (pos < x.T) {
        const int r = (int)(low & 2047u);
        if (r < x.T) {
            f = x.t0 + r;
            v = single[x.t0 + r];
        }
    } else if (pos - x.T < x.P) {
        const int64_t j = pos - x.T, T = x.T;
        auto first = [&](int64_t a) { return a * (2 * T - a - 1) / 2; };  // index of (a, a+1)
        const double s = (double)(2 * T - 1);
        int64_t a = (int64_t)((s - sqrt(s * s - 8.0 * (double)j)) * 0.5);
        a = min(max(a, (int64_t)0), T - 2);
        while (a > 0 && first(a) > j) --a;
        while (a < T - 2 && first(a + 1) <= j) ++a;
        f = x.t0 + (int)a;
        g = x.t0 + (int)(a + 1 + (j - first(a)));
        v = pair[x.p0 + j];
    }
    out_first[at] = f;
    out_second[at] = g;
    out_score[at] = do_round ? po_round3(v) : v;
}

// LDS route: one workgroup per document with lo < entries <= hi (the other documents'
// workgroups leave at once).  Keys [n2] in dynamic LDS, n2 the power of two >= entries;
// padding keys are 0, below every real key.
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
pair_order_lds_kernel(const float *__restrict__ single, const float *__restrict__ pair,
                      const int32_t *__restrict__ cu_terms, const int64_t *__restrict__ cu_pairs,
                      const int32_t *__restrict__ single_pos, const int64_t *__restrict__ out_cu,
                      int lo, int hi, int do_round, int64_t out_cap,
                      int32_t *__restrict__ out_first, int32_t *__restrict__ out_second,
                      float *__restrict__ out_score, const int32_t *__restrict__ err) {
    extern __shared__ uint64_t keys[];
    __shared__ uint32_t counter;
    if (*err) return;
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t o = out_cu[d], n64 = out_cu[d + 1] - o;
    if (n64 <= lo || n64 > hi) return;
    const int n = (int)n64;
    const PoDoc x = po_doc(cu_terms, cu_pairs, d);
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n2; i += THREADS) keys[i] = 0;
    if (tid == 0) counter = (uint32_t)x.T;
    __syncthreads();
    po_build_keys<THREADS>(x, single, pair, single_pos, keys, (uint32_t)n, &counter);
    __syncthreads();
    bitonic_sort_desc<THREADS>(keys, n2);
    for (int i = tid; i < n; i += THREADS)
        if (o + i < out_cap)
            po_emit(keys[i], x, single, pair, do_round, o + i, out_first, out_second, out_score);
}

__device__ __forceinline__ int po_find(const int64_t *off, int n, int64_t i) {
    int lo = 0, hi = n;  // last l with off[l] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Large route, 1: the keys of large document l into the scratch at lkey[l].  One
// workgroup per document; the append counter lives in LDS.
__global__ void __launch_bounds__(PO_BIG_THREADS)
pair_keys_kernel(const float *__restrict__ single, const float *__restrict__ pair,
                 const int32_t *__restrict__ cu_terms, const int64_t *__restrict__ cu_pairs,
                 const int32_t *__restrict__ single_pos, const int32_t *__restrict__ ldoc,
                 const int64_t *__restrict__ lkey, uint64_t *__restrict__ keys,
                 const int32_t *__restrict__ err) {
    __shared__ uint32_t counter;
    if (*err) return;
    const int l = blockIdx.x, d = ldoc[l];
    const PoDoc x = po_doc(cu_terms, cu_pairs, d);
    const int64_t n = lkey[l + 1] - lkey[l];
    if (threadIdx.x == 0) counter = (uint32_t)x.T;
    __syncthreads();
    po_build_keys<PO_BIG_THREADS>(x, single, pair, single_pos, keys + lkey[l], (uint32_t)n,
                                  &counter);
}

// Large route, 2: one workgroup sorts one run of up to PO_LDS_KEYS keys in place.
__global__ void __launch_bounds__(PO_BIG_THREADS)
pair_runs_kernel(int n_large, const int64_t *__restrict__ lkey, const int64_t *__restrict__ lrun,
                 uint64_t *__restrict__ keys, const int32_t *__restrict__ err) {
    extern __shared__ uint64_t s[];
    if (*err) return;
    const int tid = threadIdx.x;
    const int l = po_find(lrun, n_large, blockIdx.x);
    const int64_t q = blockIdx.x - lrun[l], n = lkey[l + 1] - lkey[l];
    const int64_t b = q * PO_LDS_KEYS;
    if (b >= n) return;
    const int m = (int)min((int64_t)PO_LDS_KEYS, n - b);
    uint64_t *g = keys + lkey[l] + b;
    int m2 = 2;
    while (m2 < m) m2 <<= 1;
    for (int i = tid; i < m2; i += PO_BIG_THREADS) s[i] = i < m ? g[i] : 0;
    __syncthreads();
    bitonic_sort_desc<PO_BIG_THREADS>(s, m2);
    for (int i = tid; i < m; i += PO_BIG_THREADS) g[i] = s[i];
}

// This thread's outputs [o0, o0 + cnt) of a large document's pass over runs of w keys:
// the merge of the runs [base, base + w) and [base + w, base + 2w) that hold o0, cut at
// the document's n keys (the second may be empty: an odd run count copies its last run).
struct PoMerge {
    const uint64_t *A, *B;
    int64_t la, lb, i, j;
    __device__ __forceinline__ PoMerge(const uint64_t *src, int64_t n, int64_t w, int64_t o0) {
        const int64_t base = o0 / (2 * w) * (2 * w);
        A = src + base;
        la = min(w, n - base);
        B = A + la;
        lb = min(w, n - base - la);
        const int64_t k = o0 - base;  // diagonal: i + j = k
        int64_t lo = max((int64_t)0, k - lb), hi = min(k, la);
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (A[mid] > B[k - 1 - mid]) lo = mid + 1; else hi = mid;
        }
        i = lo;
        j = k - lo;
    }
    __device__ __forceinline__ uint64_t next() {
        const bool take_a = j >= lb || (i < la && A[i] > B[j]);
        return take_a ? A[i++] : B[j++];
    }
};

// Large route, 3: one merge pass src -> dst.  One workgroup per tile of PO_TILE outputs
// (a tile lies inside one pair of runs), PO_ITEMS consecutive outputs per thread.
__global__ void __launch_bounds__(PO_MERGE_THREADS)
pair_merge_kernel(int n_large, const int64_t *__restrict__ lkey, const int64_t *__restrict__ ltile,
                  const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int64_t w,
                  const int32_t *__restrict__ err) {
    if (*err) return;
    const int l = po_find(ltile, n_large, blockIdx.x);
    const int64_t n = lkey[l + 1] - lkey[l];
    const int64_t o0 = (blockIdx.x - ltile[l]) * PO_TILE + (int64_t)threadIdx.x * PO_ITEMS;
    if (o0 >= n) return;
    const int cnt = (int)min((int64_t)PO_ITEMS, n - o0);
    PoMerge m(src + lkey[l], n, w, o0);
    uint64_t *out = dst + lkey[l] + o0;
    for (int t = 0; t < cnt; ++t) out[t] = m.next();
}

// Large route, 4: the entries of the sorted keys.
__global__ void __launch_bounds__(PO_MERGE_THREADS)
pair_emit_kernel(int n_large, const int32_t *__restrict__ ldoc, const int64_t *__restrict__ lkey,
                 const int64_t *__restrict__ ltile, const uint64_t *__restrict__ keys,
                 const float *__restrict__ single, const float *__restrict__ pair,
                 const int32_t *__restrict__ cu_terms, const int64_t *__restrict__ cu_pairs,
                 const int64_t *__restrict__ out_cu, int do_round, int64_t out_cap,
                 int32_t *__restrict__ out_first, int32_t *__restrict__ out_second,
                 float *__restrict__ out_score, const int32_t *__restrict__ err) {
    if (*err) return;
    const int l = po_find(ltile, n_large, blockIdx.x);
    const int d = ldoc[l];
    const int64_t n = lkey[l + 1] - lkey[l], o = out_cu[d];
    const PoDoc x = po_doc(cu_terms, cu_pairs, d);
    const int64_t i0 = (blockIdx.x - ltile[l]) * PO_TILE;
    for (int64_t i = i0 + threadIdx.x; i < min(n, i0 + PO_TILE); i += PO_MERGE_THREADS)
        if (o + i < out_cap)
            po_emit(keys[lkey[l] + i], x, single, pair, do_round, o + i, out_first, out_second,
                    out_score);
}

}  // namespace

void PairOrderWs::reserve_docs(int n_docs) {
    const size_t nd = (size_t)std::max(n_docs, 1);
    cnt.reserve(nd * 4);
    info.reserve(PO_INFO * 8);
    ldoc.reserve(nd * 4);
    loff.reserve(3 * (nd + 1) * 8);
    err.reserve(16);
}

void pairwise_order_run(PairOrderWs &ws, Timer *timer, bool timing, const float *single,
                        const float *pair, const int32_t *cu_terms, const int64_t *cu_pairs,
                        const int32_t *single_pos, int n_docs, int64_t n_terms, int64_t n_pairs,
                        int64_t *out_cu, int32_t *out_first, int32_t *out_second,
                        float *out_score, int64_t out_cap, int64_t *n_out, bool out_dev,
                        bool round3, hipStream_t s) {
    Timer none;
    Timer &tm = timer ? *timer : none;
    timing = timing && timer;
    *n_out = 0;
    if (n_docs == 0) {
        const int64_t zero = 0;
        DI_HIP(hipMemcpyAsync(out_cu, &zero, 8,
                              out_dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost, s));
        DI_HIP(hipStreamSynchronize(s));
        return;
    }
    ws.reserve_docs(n_docs);
    int32_t *d_cnt = ws.cnt.as<int32_t>(), *d_err = ws.err.as<int32_t>();
    int64_t *d_info = ws.info.as<int64_t>();
    int32_t *d_ldoc = ws.ldoc.as<int32_t>();
    int64_t *d_lkey = ws.loff.as<int64_t>(), *d_lrun = d_lkey + (n_docs + 1),
            *d_ltile = d_lrun + (n_docs + 1);
    StagedOut<int64_t> cu(out_cu, (size_t)n_docs + 1, out_dev, ws.o_cu);
    int64_t *d_cu = cu.d;
    DI_HIP(hipMemsetAsync(d_err, 0, 4, s));
    {
        TimedLaunch tl(tm, timing, "pair_count", s);
        hipLaunchKernelGGL(pair_count_kernel, dim3(n_docs), dim3(256), 0, s, pair, cu_terms,
                           cu_pairs, single_pos, n_docs, n_terms, n_pairs, d_cnt, d_err);
        check_launch("pair_count");
        hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(256), 0, s, d_cnt, n_docs, d_cu, d_info,
                           d_ldoc, d_lkey, d_lrun, d_ltile);
        check_launch("pair_scan");
    }
    int64_t info[PO_INFO];
    int32_t err = 0;
    DI_HIP(hipMemcpyAsync(info, d_info, sizeof info, hipMemcpyDeviceToHost, s));
    cu.copy_back(s);
    read_back(err, d_err, s, &tm);
    DI_REQUIRE(!(err & ERR_CU), DI_EINVAL,
               "cu_terms / cu_pairs: every document needs T <= %d terms and T (T - 1) / 2 pairs, "
               "ending at n_terms and n_pairs", PO_MAX_T);
    DI_REQUIRE(!(err & ERR_POS), DI_EINVAL, "single_pos must be a position inside its document");
    const int64_t total = info[PO_N_OUT];
    *n_out = total;
    DI_REQUIRE(total <= out_cap, DI_ERANGE, "%lld entries do not fit out_cap %lld",
               (long long)total, (long long)out_cap);
    if (total == 0) return;
    DI_REQUIRE(out_first && out_second && out_score, DI_EINVAL, "null output");
    StagedOut<int32_t> first(out_first, (size_t)total, out_dev, ws.o_first),
        second(out_second, (size_t)total, out_dev, ws.o_second);
    StagedOut<float> score(out_score, (size_t)total, out_dev, ws.o_score);
    int32_t *d_first = first.d, *d_second = second.d;
    float *d_score = score.d;
    if (!out_dev) out_cap = total;
    const int n_large = (int)info[PO_N_LARGE];
    const int rnd = round3 ? 1 : 0;
    uint64_t *kA = nullptr, *kB = nullptr;
    if (n_large) {
        ws.keyA.reserve((size_t)info[PO_KEYS] * 8);
        ws.keyB.reserve((size_t)info[PO_KEYS] * 8);
        kA = ws.keyA.as<uint64_t>();
        kB = ws.keyB.as<uint64_t>();
    }
    const size_t big_lds = (size_t)PO_LDS_KEYS * 8;
    {
        TimedLaunch tl(tm, timing, "pair_order", s);
        if (info[PO_N_SMALL]) {
            hipLaunchKernelGGL(pair_order_lds_kernel<PO_SMALL_THREADS>, dim3(n_docs),
                               dim3(PO_SMALL_THREADS), (size_t)PO_SMALL_KEYS * 8, s, single, pair,
                               cu_terms, cu_pairs, single_pos, d_cu, 0, PO_SMALL_KEYS, rnd, out_cap,
                               d_first, d_second, d_score, d_err);
            check_launch("pair_order (small)");
        }
        if (info[PO_N_MID]) {
            auto k = pair_order_lds_kernel<PO_BIG_THREADS>;
            DI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds));
            hipLaunchKernelGGL(k, dim3(n_docs), dim3(PO_BIG_THREADS), big_lds, s, single, pair,
                               cu_terms, cu_pairs, single_pos, d_cu, PO_SMALL_KEYS, PO_LDS_KEYS,
                               rnd, out_cap, d_first, d_second, d_score, d_err);
            check_launch("pair_order (LDS)");
        }
        if (n_large) {
            hipLaunchKernelGGL(pair_keys_kernel, dim3(n_large), dim3(PO_BIG_THREADS), 0, s, single,
                               pair, cu_terms, cu_pairs, single_pos, d_ldoc, d_lkey, kA, d_err);
            check_launch("pair_keys");
            auto k = pair_runs_kernel;
            DI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds));
            hipLaunchKernelGGL(k, dim3((unsigned)info[PO_RUNS]), dim3(PO_BIG_THREADS), big_lds, s,
                               n_large, d_lkey, d_lrun, kA, d_err);
            check_launch("pair_runs");
        }
    }
    if (n_large) {
        TimedLaunch tl(tm, timing, "pair_merge", s);
        const unsigned tiles = (unsigned)info[PO_TILES];
        for (int64_t w = PO_LDS_KEYS; w < info[PO_MAX_RUNS] * PO_LDS_KEYS; w *= 2) {
            hipLaunchKernelGGL(pair_merge_kernel, dim3(tiles), dim3(PO_MERGE_THREADS), 0, s,
                               n_large, d_lkey, d_ltile, kA, kB, w, d_err);
            check_launch("pair_merge");
            std::swap(kA, kB);
        }
        hipLaunchKernelGGL(pair_emit_kernel, dim3(tiles), dim3(PO_MERGE_THREADS), 0, s, n_large,
                           d_ldoc, d_lkey, d_ltile, kA, single, pair, cu_terms, cu_pairs, d_cu, rnd,
                           out_cap, d_first, d_second, d_score, d_err);
        check_launch("pair_emit");
    }
    first.copy_back(s);
    second.copy_back(s);
    score.copy_back(s);
    DI_HIP(hipStreamSynchronize(s));
    tm.resolve();
}

}  // namespace di

using namespace di;

extern "C" int di_pairwise_order(const float *single, const float *pair, const int32_t *cu_terms,
                                 const int64_t *cu_pairs, const int32_t *single_pos,
                                 int32_t n_docs, int64_t n_terms, int64_t n_pairs,
                                 int64_t *out_cu, int32_t *out_first, int32_t *out_second,
                                 float *out_score, int64_t out_cap, int64_t *n_out, int device,
                                 void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(cu_terms && cu_pairs && out_cu && n_out && n_docs >= 0 && out_cap >= 0,
                   DI_EINVAL, "bad argument");
        check_device(device);
        DeviceScope ds(device);
        const bool dev = flags & DI_F_DEVICE_PTRS;
        hipStream_t s = (hipStream_t)hip_stream;
        if (!dev) {  // the checks of di_encode_pairwise, with the document in the message
            DI_REQUIRE(cu_pairs[0] == 0, DI_EINVAL, "cu_pairs[0] must be 0");
            n_terms = check_cu(cu_terms, n_docs, "cu_terms");
            for (int d = 0; d < n_docs; ++d) {
                const int64_t T = (int64_t)cu_terms[d + 1] - cu_terms[d];
                DI_REQUIRE(cu_pairs[d + 1] - cu_pairs[d] == T * (T - 1) / 2, DI_EINVAL,
                           "cu_pairs: document %d has %lld terms, so %lld pairs", d, (long long)T,
                           (long long)(T * (T - 1) / 2));
                DI_REQUIRE(T <= PO_MAX_T, DI_ERANGE, "document %d has %lld terms > %d", d,
                           (long long)T, PO_MAX_T);
            }
            n_pairs = cu_pairs[n_docs];
        }
        DI_REQUIRE(n_terms >= 0 && n_terms < (1ll << 31) && n_pairs >= 0, DI_EINVAL,
                   "n_terms=%lld n_pairs=%lld", (long long)n_terms, (long long)n_pairs);
        DI_REQUIRE((n_terms == 0 || single) && (n_pairs == 0 || pair), DI_EINVAL, "null input");
        PairOrderWs ws;
        DevBuf b_single, b_pair, b_ct, b_cp, b_sp;
        const float *d_single = stage_in(single, (size_t)n_terms, dev, b_single, s);
        const float *d_pair = stage_in(pair, (size_t)n_pairs, dev, b_pair, s);
        const int32_t *d_ct = stage_in(cu_terms, (size_t)n_docs + 1, dev, b_ct, s);
        const int64_t *d_cp = stage_in(cu_pairs, (size_t)n_docs + 1, dev, b_cp, s);
        const int32_t *d_sp = single_pos && n_terms
            ? stage_in(single_pos, (size_t)n_terms, dev, b_sp, s) : nullptr;
        pairwise_order_run(ws, nullptr, false, d_single, d_pair, d_ct, d_cp, d_sp, n_docs, n_terms,
                           n_pairs, out_cu, out_first, out_second, out_score, out_cap, n_out, dev,
                           flags & DI_F_ROUND3, s);
    });
}
