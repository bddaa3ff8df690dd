// rerank.hip -- second-stage re-ranking with the impact model on the device, gfx950: a
// store of every encoded passage's (term id, impact) pairs and the scorer of
// (query, candidate passage) pairs over it.
//
// Replaces, for the candidates of a group of queries, the reference's
//   ReRanker.cache / ReRanker.save   src/deep_impact/evaluation/reranker.py:39,48-50
//   ReRanker.score                   src/deep_impact/evaluation/reranker.py:52-53
// (one Python dict per passage, one generator sum per candidate).  The order of line 91
// is di_segment_order's (cross.hip).
//
// Store layout: keys[n_terms] 64-bit, term id << 32 | impact bits, passage d's at
// [off[d], off[d + 1]), sorted descending (bitonic_sort_desc), so the term ids descend and
// are distinct; off[n_docs + 1] int64.  Both buffers grow by reallocation: indices stay.
//   rerank_sort    one workgroup per appended passage: keys built and sorted in LDS,
//                  neighbours compared for a repeated id, written behind the store's end
//   rerank_score   one wave per candidate: the passage's keys staged in LDS by coalesced
//                  loads (up to TS_LDS_T; a longer one is searched in global memory), lane
//                  j binary-searches query term j, and the matched impacts are added in
//                  lane order -- the query's order -- by a ballot-ordered loop; queries
//                  longer than a wave go in chunks of 64 that carry the sum.
#include <hip/hip_runtime.h>

#include "di_common.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int TS_MAX_T = DI_TERM_STORE_MAX_TERMS;  // 16 KiB of keys in LDS
constexpr int TS_SORT_THREADS = 256;
constexpr int TS_SCORE_THREADS = 256, TS_WAVES = TS_SCORE_THREADS / 64;
constexpr int TS_LDS_T = 256;  // keys of a passage the scorer stages in LDS (2 KiB a wave)

constexpr int TS_ERR_CU = 1;     // cu_terms not starting at 0, decreasing or past its end
constexpr int TS_ERR_LONG = 2;   // a passage of more than TS_MAX_T pairs
constexpr int TS_ERR_DUP = 4;    // a term id twice in one passage
constexpr int TS_ERR_CAND = 8;   // a candidate index outside the store
constexpr int TS_ERR_QUERY = 16; // cu_q decreasing, or a query of too many terms

// Passage d of an append: its keys sorted into keys[term0 + cu_terms[d] ...) and its end
// into off[doc0 + d + 1].  `total` is cu_terms[n_docs] as the host read it: no key is
// written outside [term0, term0 + total).  A violation sets an error bit and writes
// nothing (the host then leaves the store's counts as they were).
__global__ void __launch_bounds__(TS_SORT_THREADS)
rerank_sort_kernel(const uint32_t *__restrict__ term_ids, const float *__restrict__ impacts,
                   const int32_t *__restrict__ cu_terms, int64_t total, int64_t doc0,
                   int64_t term0, uint64_t *__restrict__ keys, int64_t *__restrict__ off,
                   int32_t *__restrict__ err) {
    __shared__ uint64_t s[TS_MAX_T];
    const int d = blockIdx.x, tid = threadIdx.x;
    const int64_t t0 = cu_terms[d], t1 = cu_terms[d + 1];
    const int64_t T64 = t1 - t0;
    int bad = 0;
    if (t0 < 0 || T64 < 0 || t1 > total || (d == 0 && t0 != 0))
        bad = TS_ERR_CU;
    else if (T64 > TS_MAX_T)
        bad = TS_ERR_LONG;
    if (bad) {  // (the same for every thread of the workgroup)
        if (tid == 0) atomicOr(err, bad);
        return;
    }
    if (tid == 0) off[doc0 + d + 1] = term0 + t1;
    const int T = (int)T64;
    if (T == 0) return;
    int n2 = 2;
    while (n2 < T) n2 <<= 1;
    // padding keys are 0, not above any real key
    for (int i = tid; i < n2; i += TS_SORT_THREADS)
        s[i] = i < T ? ((uint64_t)term_ids[t0 + i] << 32) | __float_as_uint(impacts[t0 + i]) : 0;
    __syncthreads();
    bitonic_sort_desc<TS_SORT_THREADS>(s, n2);
    bool dup = false;
    for (int i = tid; i < T; i += TS_SORT_THREADS) {
        const uint64_t k = s[i];
        if (i + 1 < T && (uint32_t)(k >> 32) == (uint32_t)(s[i + 1] >> 32)) dup = true;
        keys[term0 + t0 + i] = k;
    }
    if (dup) atomicOr(err, TS_ERR_DUP);
}

// The impact of `term` among T keys whose ids descend; false when it is not there.
template <class Keys>
__device__ __forceinline__ bool ts_find(Keys k, int T, uint32_t term, float *v) {
    int lo = 0, hi = T;  // first key with id <= term
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(k[mid] >> 32) > term) lo = mid + 1; else hi = mid;
    }
    if (lo >= T) return false;
    const uint64_t x = k[lo];
    *v = __uint_as_float((uint32_t)x);
    return (uint32_t)(x >> 32) == term;
}

// One wave per candidate c (TS_WAVES candidates a workgroup).
__global__ void __launch_bounds__(TS_SCORE_THREADS)
rerank_score_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ off,
                    int64_t n_docs, const uint32_t *__restrict__ q_terms,
                    const int32_t *__restrict__ cu_q, int n_q,
                    const int32_t *__restrict__ cand_doc, const int32_t *__restrict__ cu_cand,
                    int64_t n_c, float *__restrict__ out_score, int32_t *__restrict__ out_match,
                    int32_t *__restrict__ err) {
    __shared__ uint64_t staged[TS_WAVES][TS_LDS_T];
    const int lane = lane_id(), w = wave_id();
    const int64_t c = (int64_t)blockIdx.x * TS_WAVES + w;
    bool live = c < n_c;
    int q0 = 0, q1 = 0, T = 0;
    int64_t o = 0;
    if (live) {
        int lo = 0, hi = n_q;  // last query with cu_cand[q] <= c
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cu_cand[mid] <= c) lo = mid; else hi = mid;
        }
        q0 = cu_q[lo];
        q1 = cu_q[lo + 1];
        const int32_t doc = cand_doc[c];
        int bad = 0;
        if (q0 < 0 || q1 < q0 || q1 - q0 > DI_MAX_QUERY_TERMS) bad |= TS_ERR_QUERY;
        if (doc < 0 || doc >= n_docs) bad |= TS_ERR_CAND;
        if (bad) {
            if (lane == 0) {
                atomicOr(err, bad);
                out_score[c] = 0.f;
                out_match[c] = 0;
            }
            live = false;
        } else {
            o = off[doc];
            T = (int)(off[doc + 1] - o);
        }
    }
    const bool in_lds = T <= TS_LDS_T;  // (T = 0 for a wave without a candidate)
    if (in_lds)
        for (int i = lane; i < T; i += 64) staged[w][i] = keys[o + i];
    __syncthreads();  // the workgroup's only barrier: every wave reaches it
    if (!live) return;
    float acc = 0.f;
    int cnt = 0;
    for (int base = q0; base < q1; base += 64) {
        const int j = base + lane;
        bool have = false;
        float v = 0.f;
        if (j < q1) {
            const uint32_t term = q_terms[j];
            have = in_lds ? ts_find(&staged[w][0], T, term, &v) : ts_find(keys + o, T, term, &v);
        }
        uint64_t m = __ballot(have);
        while (m) {  // lane order is query order; one rounded add per match
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            acc = __fadd_rn(acc, __shfl(v, l, 64));
            ++cnt;
        }
    }
    if (lane == 0) {
        out_score[c] = acc;
        out_match[c] = cnt;
    }
}

}  // namespace
}  // namespace di

struct di_term_store {
    int device = 0;
    int64_t n_docs = 0, n_terms = 0;
    di::DevBuf keys, off;  // the store
    di::DevBuf err, in_ids, in_imp, in_cu, in_q, in_cq, in_cand, in_cc, o_score, o_match;
    di::Timer timer;
};

using namespace di;

namespace {

void ts_reserve(di_term_store *ts, int64_t n_docs, int64_t n_terms, hipStream_t s) {
    const bool fresh = !ts->off.p;
    grow_keep(ts->off, (size_t)(std::max<int64_t>(n_docs, 1) + 1) * 8,
              fresh ? 0 : (size_t)(ts->n_docs + 1) * 8, s);
    if (fresh) {
        DI_HIP(hipMemsetAsync(ts->off.p, 0, 8, s));  // off[0] = 0
        DI_HIP(hipStreamSynchronize(s));
    }
    grow_keep(ts->keys, (size_t)std::max<int64_t>(n_terms, 1) * 8, (size_t)ts->n_terms * 8, s);
}

}  // namespace

extern "C" {

int di_term_store_create(int device, di_term_store **out) {
    return guard([&] {
        DI_REQUIRE(out, DI_EINVAL, "null output");
        *out = nullptr;
        check_device(device);
        DeviceScope ds(device);
        di_term_store *ts = new di_term_store;
        ts->device = device;
        try {
            ts->err.reserve(4);
            ts_reserve(ts, 1, 1, nullptr);
        } catch (...) {
            delete ts;
            throw;
        }
        *out = ts;
    });
}

int di_term_store_reserve(di_term_store *ts, int64_t n_docs, int64_t n_terms) {
    return guard([&] {
        DI_REQUIRE(ts && n_docs >= 0 && n_terms >= 0, DI_EINVAL, "bad argument");
        DI_REQUIRE(n_docs < (1ll << 31), DI_ERANGE, "a store holds fewer than 2^31 passages");
        DeviceScope ds(ts->device);
        ts_reserve(ts, std::max(n_docs, ts->n_docs), std::max(n_terms, ts->n_terms), nullptr);
    });
}

int di_term_store_append(di_term_store *ts, const uint32_t *term_ids, const float *impacts,
                         const int32_t *cu_terms, int32_t n_docs, int64_t *first_doc,
                         void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(ts && cu_terms && first_doc && n_docs >= 0, DI_EINVAL, "bad argument");
        DeviceScope ds(ts->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        *first_doc = ts->n_docs;
        if (n_docs == 0) return;
        // the offsets are checked on the host before anything changes (with device
        // pointers a copy of them is read back: 4 bytes a passage)
        std::vector<int32_t> h_cu;
        const int64_t total =
            check_cu(host_cu(cu_terms, n_docs, dev, h_cu, s), n_docs, "cu_terms", TS_MAX_T);
        DI_REQUIRE(total == 0 || (term_ids && impacts), DI_EINVAL, "null input");
        DI_REQUIRE(ts->n_docs + n_docs < (1ll << 31), DI_ERANGE,
                   "a store holds fewer than 2^31 passages");
        ts_reserve(ts, ts->n_docs + n_docs, ts->n_terms + total, s);
        const uint32_t *d_ids = stage_in(term_ids, (size_t)total, dev, ts->in_ids, s);
        const float *d_imp = stage_in(impacts, (size_t)total, dev, ts->in_imp, s);
        const int32_t *d_cu = stage_in(cu_terms, (size_t)n_docs + 1, dev, ts->in_cu, s);
        DI_HIP(hipMemsetAsync(ts->err.p, 0, 4, s));
        {
            TimedLaunch tl(ts->timer, timing, "ts_sort", s);
            hipLaunchKernelGGL(rerank_sort_kernel, dim3(n_docs), dim3(TS_SORT_THREADS), 0, s,
                               d_ids, d_imp, d_cu, total, ts->n_docs, ts->n_terms,
                               ts->keys.as<uint64_t>(), ts->off.as<int64_t>(),
                               ts->err.as<int32_t>());
            check_launch("rerank_sort");
        }
        int32_t e = 0;
        read_back(e, ts->err.p, s, &ts->timer);
        DI_REQUIRE(!(e & TS_ERR_CU), DI_EINVAL, "cu_terms must start at 0 and not decrease");
        DI_REQUIRE(!(e & TS_ERR_LONG), DI_ERANGE, "a passage has more than %d terms", TS_MAX_T);
        DI_REQUIRE(!(e & TS_ERR_DUP), DI_EINVAL, "a passage holds the same term id twice");
        ts->n_docs += n_docs;
        ts->n_terms += total;
    });
}

int di_term_store_info(const di_term_store *ts, int64_t *n_docs, int64_t *n_terms,
                       int64_t *device_bytes) {
    return guard([&] {
        DI_REQUIRE(ts, DI_EINVAL, "null handle");
        if (n_docs) *n_docs = ts->n_docs;
        if (n_terms) *n_terms = ts->n_terms;
        if (device_bytes) *device_bytes = (int64_t)(ts->keys.bytes + ts->off.bytes);
    });
}

int di_term_store_score(di_term_store *ts, const uint32_t *q_terms, const int32_t *cu_q,
                        int32_t n_q, const int32_t *cand_doc, const int32_t *cu_cand,
                        float *out_score, int32_t *out_match, void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(ts && cu_q && cu_cand && n_q >= 0, DI_EINVAL, "bad argument");
        DeviceScope ds(ts->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        if (n_q == 0) return;
        int64_t n_c = 0, n_qt = 0;
        if (!dev) {
            n_c = check_cu(cu_cand, n_q, "cu_cand");
            n_qt = check_cu(cu_q, n_q, "cu_q", DI_MAX_QUERY_TERMS);
        } else {
            int32_t last = 0;
            read_back(last, cu_cand + n_q, s);
            n_c = last;
            DI_REQUIRE(n_c >= 0, DI_EINVAL, "cu_cand ends at %lld", (long long)n_c);
        }
        if (n_c == 0) return;
        DI_REQUIRE(cand_doc && out_score && out_match && (n_qt == 0 || q_terms), DI_EINVAL,
                   "null argument");
        const uint32_t *d_q = stage_in(q_terms, (size_t)n_qt, dev, ts->in_q, s);
        const int32_t *d_cq = stage_in(cu_q, (size_t)n_q + 1, dev, ts->in_cq, s);
        const int32_t *d_cand = stage_in(cand_doc, (size_t)n_c, dev, ts->in_cand, s);
        const int32_t *d_cc = stage_in(cu_cand, (size_t)n_q + 1, dev, ts->in_cc, s);
        StagedOut<float> score(out_score, (size_t)n_c, dev, ts->o_score);
        StagedOut<int32_t> match(out_match, (size_t)n_c, dev, ts->o_match);
        DI_HIP(hipMemsetAsync(ts->err.p, 0, 4, s));
        {
            TimedLaunch tl(ts->timer, timing, "ts_score", s);
            const int64_t blocks = (n_c + TS_WAVES - 1) / TS_WAVES;
            hipLaunchKernelGGL(rerank_score_kernel, dim3((unsigned)blocks), dim3(TS_SCORE_THREADS),
                               0, s, ts->keys.as<uint64_t>(), ts->off.as<int64_t>(), ts->n_docs,
                               d_q, d_cq, n_q, d_cand, d_cc, n_c, score.d, match.d,
                               ts->err.as<int32_t>());
            check_launch("rerank_score");
        }
        score.copy_back(s);
        match.copy_back(s);
        int32_t e = 0;
        read_back(e, ts->err.p, s, &ts->timer);
        DI_REQUIRE(!(e & TS_ERR_CAND), DI_EINVAL,
                   "a candidate index is outside the store's %lld passages",
                   (long long)ts->n_docs);
        DI_REQUIRE(!(e & TS_ERR_QUERY), DI_ERANGE,
                   "cu_q must not decrease and a query has at most %d terms", DI_MAX_QUERY_TERMS);
    });
}

int di_term_store_timing(di_term_store *ts, const char *name, di_timing *out, int reset) {
    return guard([&] {
        DI_REQUIRE(ts && name && out, DI_EINVAL, "bad argument");
        ts->timer.get(name, out, reset != 0);
    });
}

int di_term_store_destroy(di_term_store *ts) {
    return guard([&] {
        if (!ts) return;
        DeviceScope ds(ts->device);
        delete ts;
    });
}

}  // extern "C"
