// index_build.hip -- the quantized inverted index (the CSR di_index_create takes, the
// bytes of inverted_index.dat) assembled on the device from (term id, impact) pairs per
// document, e.g. di_encode's DI_F_ROUND3 output buffer, gfx950.
//
// Replaces, for inputs that are already on the device, the text route
//   quantize_file (reference src/deep_impact/indexing/quantize.py:13-47) and
//   InvertedIndexCreator (src/deep_impact/inverted_index/create.py:12-55).
// The builder keeps every appended pair as (term id, doc, impact), 12 bytes, in document
// order: pair i of an append goes to end + i, its document found by a search of cu_terms.
//   ib_max       max(0, impacts) and a flag for a non-finite impact
//   ib_quantize  val = int(double(impact) * (255 / max)), quantize.py:37-45 in fp64 (the
//                arithmetic of quantize_kernel, enc_misc.hip); kept iff val > 0; the kept
//                pairs of every tile of IB_TILE pairs and of every term id are counted
//                (counts only: the order of the atomic adds reaches no position)
//   ib_scan      exclusive scan of the tile counts (three kernels, int64)
//   ib_compact   the kept pairs, in order, as 16-byte records (doc, term id, 255 - val):
//                a record's place is its tile's offset + the kept pairs before it in the
//                tile (wave ballots, the waves' counts added in wave order)
// The kept records are therefore still in ascending doc order, and the reference order --
// per term row value descending, doc ascending (create.py:41, a stable sort of a
// doc-ordered list) -- is a *stable* sort of them by (row, 255 - val).  It is built as a
// least-significant-digit radix sort with 8-bit digits: one pass on 255 - val, then
// ceil(bits(n_rows - 1) / 8) passes on the row.  Every pass:
//   ib_hist      per tile of IB_TILE records a 256-bin digit histogram (LDS counters)
//   ib_scan      one exclusive scan over (digit, tile)
//   ib_scatter   a record goes to scan[digit][tile] + the records of that digit before it
//                in the tile.  The tile is walked 256 records at a time; inside a wave the
//                rank among equal digits comes from eight ballots, across the four waves
//                and across the rounds from LDS counters added in wave and round order.
// Why it is stable and run-to-run identical: every place is a sum of counts of records
// that precede it in the input order; no atomic hands out a slot.  Work per kept posting
// and pass: two 16-byte reads, one 16-byte store, eight ballots, two LDS accesses.
// The first pass also replaces the term id by its row (term_row), so the records of
// ib_compact stay as they are and postings can be asked for again.
//
// The pairwise model (DeepPairwiseImpact.compute_term_impacts, pairwise_impact.py:98-129):
// di_index_builder_append_pairwise takes di_encode_pairwise's unrounded single and pair
// scores.  The singles go the way above (rounded by ib_append); a pair whose round3 score
// is not zero (:122) is the posting of the term t_a + '|' + t_b, kept as the record
// (id_a, id_b, doc, score), 16 bytes, in document order:
//   ib_pair_count   kept pairs per tile of IB_TILE flat pair indices (ballots)
//   ib_scan         their exclusive scan
//   ib_pair_place   a kept pair's document by a search of cu_pairs, its (a, b) by the closed
//                   form of the combination index; placed at tile offset + kept pairs before
// At quantize the maximum runs over singles and pairs, and the kept pair records
// (ib_pair_quantize, ib_pair_compact, as above) get dense term numbers: a stable radix sort
// by (id_a, id_b) with the passes above (ceil(bits(n_terms - 1) / 8) a half), run heads
// flagged (ib_pair_heads) and scanned, and ib_pair_number writes record i as the kept
// posting (doc, n_terms + u, 255 - val) behind the single ones, u the rank of its key.  A
// key's records stay in ascending doc order, so the postings sort needs nothing new.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>

#include "di_common.h"
#include "ib_sort.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int IB_ERR_TERM = 1;       // a term id >= n_terms
constexpr int IB_ERR_RANGE = 2;      // a value above 255
constexpr int IB_ERR_NONFINITE = 4;  // a NaN or infinite impact

struct Ctrl {
    int32_t err;
    uint32_t max_bits;
};

// numpy's round(np.float32, 3), as enc_misc.hip (DI_F_ROUND3) and enc_pairwise.hip
__device__ __forceinline__ float ib_round3(float x) {
    return __fdiv_rn(rintf(__fmul_rn(x, 1000.0f)), 1000.0f);
}

__global__ void __launch_bounds__(IB_THREADS)
ib_append_kernel(const uint32_t *__restrict__ term_ids, const float *__restrict__ impacts,
                 const int32_t *__restrict__ cu_terms, int n_docs, int64_t total, uint32_t doc0,
                 int64_t base, int64_t cap, bool do_round, uint32_t *__restrict__ o_tid,
                 uint32_t *__restrict__ o_doc, float *__restrict__ o_imp) {
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * IB_THREADS) {
        int lo = 0, hi = n_docs;  // the last document with cu_terms[d] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cu_terms[mid] <= i) lo = mid; else hi = mid;
        }
        const int64_t pos = base + i;
        if (pos < cap) {  // (always: the buffers hold base + total pairs)
            o_tid[pos] = term_ids[i];
            o_doc[pos] = doc0 + (uint32_t)lo;
            o_imp[pos] = do_round ? ib_round3(impacts[i]) : impacts[i];
        }
    }
}

__global__ void __launch_bounds__(IB_THREADS)
ib_max_kernel(const float *__restrict__ v, int64_t n, Ctrl *__restrict__ ctrl) {
    float m = 0.f;  // find_max_value starts at 0 (quantize.py:17)
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * IB_THREADS) {
        const float x = v[i];
        bad |= !isfinite(x);
        m = fmaxf(m, x);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    // non-negative floats order like their bit patterns (-0.0 -> 0)
    if (lane_id() == 0 && m > 0.f) atomicMax(&ctrl->max_bits, __float_as_uint(m));
    if (bad) atomicOr(&ctrl->err, IB_ERR_NONFINITE);
}

__global__ void __launch_bounds__(IB_THREADS)
ib_quantize_kernel(const uint32_t *__restrict__ tid, const float *__restrict__ imp, int64_t n,
                   int64_t n_tiles, int64_t n_terms, double scale, uint8_t *__restrict__ qval,
                   uint32_t *__restrict__ tile_kept, unsigned long long *__restrict__ tcount,
                   Ctrl *__restrict__ ctrl) {
    __shared__ uint32_t wsum[IB_WAVES];
    int err = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t kept = 0;  // of this wave (the same in all its lanes)
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i = tile * IB_TILE + (int64_t)r * IB_THREADS + threadIdx.x;
            bool keep = false;
            if (i < n) {
                double p = __dmul_rn((double)imp[i], scale);
                p = fmin(fmax(p, -2147483648.0), 2147483647.0);
                const int32_t val = (int32_t)p;  // truncates toward zero, as Python int()
                const uint32_t t = tid[i];
                if (t >= n_terms) err |= IB_ERR_TERM;
                if (val > 255) err |= IB_ERR_RANGE;
                keep = val > 0 && t < n_terms;
                qval[i] = (uint8_t)(val > 0 ? min(val, 255) : 0);
                if (keep) atomicAdd(&tcount[t], 1ull);
            }
            kept += (uint32_t)__popcll(__ballot(keep));
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
    if (err) atomicOr(&ctrl->err, err);
}

__global__ void __launch_bounds__(IB_THREADS)
ib_compact_kernel(const uint32_t *__restrict__ tid, const uint32_t *__restrict__ doc,
                  const uint8_t *__restrict__ qval, int64_t n, int64_t n_tiles, int64_t n_terms,
                  const int64_t *__restrict__ tile_off, int64_t cap, uint4 *__restrict__ out) {
    __shared__ uint32_t wcnt[IB_WAVES];
    const int lane = lane_id(), wave = wave_id();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t run = tile_off[tile];
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i0 = tile * IB_TILE + (int64_t)r * IB_THREADS;
            if (i0 >= n) break;  // (the same for the whole workgroup)
            const int64_t i = i0 + threadIdx.x;
            uint32_t q = 0, t = 0;
            if (i < n) {
                q = qval[i];
                t = tid[i];
            }
            const bool keep = q > 0 && t < n_terms;
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
                if (pos >= 0 && pos < cap) out[pos] = make_uint4(doc[i], t, 255u - q, 0u);
            }
            run += all;
            __syncthreads();  // wcnt is free again
        }
    }
}

// Four records a thread: the docs as one 16-byte store and the values as one 4-byte store
// where the outputs are aligned for it (vec), else one by one.
__global__ void __launch_bounds__(IB_THREADS)
ib_extract_kernel(const uint4 *__restrict__ src, int64_t n, uint32_t *__restrict__ pdoc,
                  uint8_t *__restrict__ pval, bool vec) {
    for (int64_t q = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; q * 4 < n;
         q += (int64_t)gridDim.x * IB_THREADS) {
        const int64_t i = q * 4;
        if (vec && i + 3 < n) {
            const uint4 a = src[i], b = src[i + 1], c = src[i + 2], d = src[i + 3];
            *reinterpret_cast<uint4 *>(pdoc + i) = make_uint4(a.x, b.x, c.x, d.x);
            *reinterpret_cast<uchar4 *>(pval + i) =
                make_uchar4((uint8_t)(255u - a.z), (uint8_t)(255u - b.z), (uint8_t)(255u - c.z),
                            (uint8_t)(255u - d.z));
        } else {
            for (int64_t j = i; j < n && j < i + 4; ++j) {
                const uint4 a = src[j];
                pdoc[j] = a.x;
                pval[j] = (uint8_t)(255u - a.z);
            }
        }
    }
}

// ---- pair terms (di_index_builder_append_pairwise) ----
// tile_kept[tile] = the pairs of a tile of IB_TILE flat pair indices whose round3 score
// is not zero (pairwise_impact.py:122).
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_count_kernel(const float *__restrict__ pair, int64_t n, int64_t n_tiles,
                     uint32_t *__restrict__ tile_kept) {
    __shared__ uint32_t wsum[IB_WAVES];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t kept = 0;  // of this wave (the same in all its lanes)
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i = tile * IB_TILE + (int64_t)r * IB_THREADS + threadIdx.x;
            const bool keep = i < n && ib_round3(pair[i]) != 0.0f;
            kept += (uint32_t)__popcll(__ballot(keep));
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

// The first pair index of row a of a T-term document's combinations (a < b).
__device__ __forceinline__ int64_t ib_comb_start(int64_t a, int64_t T) {
    return a * (2 * T - a - 1) / 2;
}

// The kept pairs, in order, as records (id(t_a), id(t_b), doc, round3 score) at base + the
// tile's offset + the kept pairs before it in the tile.  Pair i's document is a search of
// cu_pairs (the last d with cu_pairs[d] <= i: a document without pairs is never it), its
// (a, b) the closed form of j = a(2T - a - 1)/2 + (b - a - 1), a from the square root and
// put right in integers.
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_place_kernel(const uint32_t *__restrict__ term_ids, const float *__restrict__ pair,
                     const int32_t *__restrict__ cu_terms, const int64_t *__restrict__ cu_pairs,
                     int n_docs, int64_t n, int64_t n_tiles, const int64_t *__restrict__ tile_off,
                     uint32_t doc0, int64_t base, int64_t cap, uint32_t *__restrict__ o_a,
                     uint32_t *__restrict__ o_b, uint32_t *__restrict__ o_doc,
                     float *__restrict__ o_imp) {
    __shared__ uint32_t wcnt[IB_WAVES];
    const int lane = lane_id(), wave = wave_id();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t run = base + tile_off[tile];
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i0 = tile * IB_TILE + (int64_t)r * IB_THREADS;
            if (i0 >= n) break;  // (the same for the whole workgroup)
            const int64_t i = i0 + threadIdx.x;
            float v = 0.f;
            if (i < n) v = ib_round3(pair[i]);
            const bool keep = i < n && v != 0.0f;
            const uint64_t m = __ballot(keep);
            if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (int w = 0; w < IB_WAVES; ++w) {
                if (w < wave) before += wcnt[w];
                all += wcnt[w];
            }
            if (keep) {
                int lo = 0, hi = n_docs;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (cu_pairs[mid] <= i) lo = mid; else hi = mid;
                }
                const int64_t T = cu_terms[lo + 1] - cu_terms[lo], j = i - cu_pairs[lo];
                const double w2 = (double)(2 * T - 1);
                int64_t a = (int64_t)((w2 - sqrt(fmax(w2 * w2 - 8.0 * (double)j, 0.0))) * 0.5);
                a = a < 0 ? 0 : (a > T - 2 ? T - 2 : a);
                while (a > 0 && ib_comb_start(a, T) > j) --a;
                while (a < T - 2 && ib_comb_start(a + 1, T) <= j) ++a;
                const int64_t bb = a + 1 + (j - ib_comb_start(a, T));
                const int64_t pos = run + before + __popcll(m & ((1ull << lane) - 1));
                // (always: the host checked cu_pairs against T(T - 1)/2, the counts add up)
                if (T >= 2 && bb > a && bb < T && pos >= base && pos < cap) {
                    o_a[pos] = term_ids[cu_terms[lo] + a];
                    o_b[pos] = term_ids[cu_terms[lo] + bb];
                    o_doc[pos] = doc0 + (uint32_t)lo;
                    o_imp[pos] = v;
                }
            }
            run += all;
            __syncthreads();  // wcnt is free again
        }
    }
}

// ib_quantize_kernel for pair records: both ids are checked, nothing is counted per term
// (a pair term has no number yet).
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_quantize_kernel(const uint32_t *__restrict__ pa, const uint32_t *__restrict__ pb,
                        const float *__restrict__ imp, int64_t n, int64_t n_tiles,
                        int64_t n_terms, double scale, uint8_t *__restrict__ qval,
                        uint32_t *__restrict__ tile_kept, Ctrl *__restrict__ ctrl) {
    __shared__ uint32_t wsum[IB_WAVES];
    int err = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t kept = 0;
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i = tile * IB_TILE + (int64_t)r * IB_THREADS + threadIdx.x;
            bool keep = false;
            if (i < n) {
                double p = __dmul_rn((double)imp[i], scale);
                p = fmin(fmax(p, -2147483648.0), 2147483647.0);
                const int32_t val = (int32_t)p;  // truncates toward zero, as Python int()
                const bool ids_ok = pa[i] < n_terms && pb[i] < n_terms;
                if (!ids_ok) err |= IB_ERR_TERM;
                if (val > 255) err |= IB_ERR_RANGE;
                keep = val > 0 && ids_ok;
                qval[i] = (uint8_t)(keep ? min(val, 255) : 0);
            }
            kept += (uint32_t)__popcll(__ballot(keep));
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
    if (err) atomicOr(&ctrl->err, err);
}

// ib_compact_kernel for pair records -> sort records (doc, id_a, id_b, 255 - val).
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_compact_kernel(const uint32_t *__restrict__ pa, const uint32_t *__restrict__ pb,
                       const uint32_t *__restrict__ doc, const uint8_t *__restrict__ qval,
                       int64_t n, int64_t n_tiles, const int64_t *__restrict__ tile_off,
                       int64_t cap, uint4 *__restrict__ out) {
    __shared__ uint32_t wcnt[IB_WAVES];
    const int lane = lane_id(), wave = wave_id();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int64_t run = tile_off[tile];
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i0 = tile * IB_TILE + (int64_t)r * IB_THREADS;
            if (i0 >= n) break;  // (the same for the whole workgroup)
            const int64_t i = i0 + threadIdx.x;
            const uint32_t q = i < n ? qval[i] : 0u;
            const bool keep = q > 0;
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
                if (pos >= 0 && pos < cap) out[pos] = make_uint4(doc[i], pa[i], pb[i], 255u - q);
            }
            run += all;
            __syncthreads();  // wcnt is free again
        }
    }
}

// head[i] = 1 where sorted pair record i starts a run of its key (id_a, id_b)
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_heads_kernel(const uint4 *__restrict__ src, int64_t n, uint32_t *__restrict__ head) {
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

// Pair number u = the run heads before and at record i, minus one (off: the exclusive scan
// of head).  The record joins the kept postings as (doc, n_terms + u, 255 - val); a run's
// head writes its key and where the run starts.
__global__ void __launch_bounds__(IB_THREADS)
ib_pair_number_kernel(const uint4 *__restrict__ src, int64_t n, const uint32_t *__restrict__ head,
                      const int64_t *__restrict__ off, int64_t n_terms, int64_t n_runs,
                      uint4 *__restrict__ kept, uint32_t *__restrict__ first,
                      uint32_t *__restrict__ second, int64_t *__restrict__ start) {
    for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * IB_THREADS) {
        const uint4 r = src[i];
        const uint32_t h = head[i];
        const int64_t u = off[i] + h - 1;
        if (u < 0 || u >= n_runs) continue;  // (never: record 0 is a head)
        kept[i] = make_uint4(r.x, (uint32_t)(n_terms + u), r.w, 0u);
        if (h) {
            first[u] = r.y;
            second[u] = r.z;
            start[u] = i;
        }
    }
}

}  // namespace
}  // namespace di

struct di_index_builder {
    int device = 0;
    int64_t n_docs = 0, n_pairs = 0;  // documents and pairs appended
    di::DevBuf tid, doc, imp;         // the pairs, in document order
    std::vector<int64_t> empty_docs;  // doc ids of the documents without a pair
    // the last quantize: the kept records in document order, the kept pairs per term id
    int64_t n_kept = -1, n_terms = 0;
    di::DevBuf kept;
    std::vector<int64_t> tcount;
    // pair terms (append_pairwise): the pairs kept by round3 as (id_a, id_b, doc, score),
    // 16 bytes, in document order
    int64_t n_precs = 0;
    di::DevBuf pa, pb, pdoc, pimp;
    // the last quantize: the distinct kept pair keys in ascending key order, pair u = term
    // id (n_terms - n_pair_terms) + u of the kept records, its count in tcount
    std::vector<uint32_t> pt_first, pt_second;
    // scratch
    di::DevBuf in_ids, in_imp, in_cu, ctrl, qval, cnt, off, csum, dcount, sort_a, sort_b, d_row,
        o_doc, o_val, o_off;
    di::DevBuf in_pair, in_cup, p_qval, p_cnt, p_off, p_first, p_second, p_start;
    di::Timer timer;
};

using namespace di;

namespace {

void ib_reserve(di_index_builder *b, int64_t n_pairs, hipStream_t s) {
    const size_t need = at_least_one(n_pairs) * 4, used = (size_t)b->n_pairs * 4;
    grow_keep(b->tid, need, used, s);
    grow_keep(b->doc, need, used, s);
    grow_keep(b->imp, need, used, s);
}

// off[0, len) = the exclusive scan of cnt[0, len) -> the total (waits for s)
int64_t ib_scan(di_index_builder *b, const uint32_t *cnt, int64_t len, int64_t *off, bool timing,
                hipStream_t s) {
    const int64_t n_chunks = (len + IB_SCAN_CHUNK - 1) / IB_SCAN_CHUNK;
    DI_REQUIRE(n_chunks <= (int64_t)INT32_MAX, DI_ERANGE, "too many postings for one scan");
    b->csum.reserve((size_t)(n_chunks + 1) * 8);
    {
        TimedLaunch tl(b->timer, timing, "ib_scan", s);
        hipLaunchKernelGGL(ib_scan_sum_kernel, dim3((unsigned)n_chunks), dim3(IB_THREADS), 0, s, cnt,
                           len, b->csum.as<int64_t>());
        check_launch("ib_scan_sum");
        hipLaunchKernelGGL(ib_scan_chunks_kernel, dim3(1), dim3(IB_THREADS), 0, s,
                           b->csum.as<int64_t>(), n_chunks);
        check_launch("ib_scan_chunks");
        hipLaunchKernelGGL(ib_scan_apply_kernel, dim3((unsigned)n_chunks), dim3(IB_THREADS), 0, s,
                           cnt, len, b->csum.as<int64_t>(), off);
        check_launch("ib_scan_apply");
    }
    int64_t total = 0;
    read_back(total, b->csum.as<int64_t>() + n_chunks, s, &b->timer);
    return total;
}

// One stable radix pass src -> dst on the 8-bit digit of .y or .z from bit `shift` on.
void ib_sort_pass(di_index_builder *b, const uint4 *src, uint4 *dst, int64_t n, bool on_y,
                  int shift, const int32_t *d_row, int64_t n_terms, bool timing,
                  const char *hist_name, const char *scatter_name, hipStream_t s) {
    const int64_t n_tiles = (n + IB_TILE - 1) / IB_TILE, cells = 256 * n_tiles;
    b->cnt.reserve((size_t)cells * 4);
    b->off.reserve((size_t)cells * 8);
    {
        TimedLaunch tl(b->timer, timing, hist_name, s);
        hipLaunchKernelGGL(ib_hist_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0, s, src,
                           n, n_tiles, on_y, shift, b->cnt.as<uint32_t>());
        check_launch("ib_hist");
    }
    const int64_t total = ib_scan(b, b->cnt.as<uint32_t>(), cells, b->off.as<int64_t>(), timing, s);
    DI_REQUIRE(total == n, DI_EHIP, "ib_hist counted %lld of %lld postings", (long long)total,
               (long long)n);
    {
        TimedLaunch tl(b->timer, timing, scatter_name, s);
        hipLaunchKernelGGL(ib_scatter_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0, s,
                           src, dst, n, n_tiles, on_y, shift, b->off.as<int64_t>(), d_row, n_terms);
        check_launch("ib_scatter");
    }
}

void ib_pair_reserve(di_index_builder *b, int64_t n_recs, hipStream_t s) {
    const size_t need = at_least_one(n_recs) * 4, used = (size_t)b->n_precs * 4;
    grow_keep(b->pa, need, used, s);
    grow_keep(b->pb, need, used, s);
    grow_keep(b->pdoc, need, used, s);
    grow_keep(b->pimp, need, used, s);
}

}  // namespace

extern "C" {

int di_index_builder_create(int device, di_index_builder **out) {
    return guard([&] {
        DI_REQUIRE(out, DI_EINVAL, "null output");
        *out = nullptr;
        check_device(device);
        DeviceScope ds(device);
        std::unique_ptr<di_index_builder> b(new di_index_builder);
        b->device = device;
        b->ctrl.reserve(sizeof(Ctrl));
        ib_reserve(b.get(), 1, nullptr);
        *out = b.release();
    });
}

int di_index_builder_reserve(di_index_builder *b, int64_t n_docs, int64_t n_pairs) {
    return guard([&] {
        DI_REQUIRE(b && n_docs >= 0 && n_pairs >= 0, DI_EINVAL, "bad argument");
        DI_REQUIRE(n_docs <= (int64_t)UINT32_MAX, DI_ERANGE, "doc ids are 32-bit");
        DeviceScope ds(b->device);
        ib_reserve(b, std::max(n_pairs, b->n_pairs), nullptr);
    });
}

int di_index_builder_append(di_index_builder *b, const uint32_t *term_ids, const float *impacts,
                            const int32_t *cu_terms, int32_t n_docs, int64_t *first_doc,
                            void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(b && cu_terms && first_doc && n_docs >= 0, DI_EINVAL, "bad argument");
        DI_REQUIRE(b->n_docs + n_docs <= (int64_t)UINT32_MAX, DI_ERANGE,
                   "%lld docs: doc ids are 32-bit", (long long)(b->n_docs + n_docs));
        DeviceScope ds(b->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        *first_doc = b->n_docs;
        if (n_docs == 0) return;
        // the offsets are checked on the host before anything changes (with device
        // pointers a copy of them is read back: 4 bytes a document)
        std::vector<int32_t> h_cu;
        const int32_t *cu = host_cu(cu_terms, n_docs, dev, h_cu, s);
        const int64_t total = check_cu(cu, n_docs, "cu_terms");
        DI_REQUIRE(total == 0 || (term_ids && impacts), DI_EINVAL, "null input");
        std::vector<int64_t> empty;
        for (int32_t d = 0; d < n_docs; ++d)
            if (cu[d + 1] == cu[d]) empty.push_back(b->n_docs + d);
        if (total > 0) {
            ib_reserve(b, b->n_pairs + total, s);
            const uint32_t *d_ids = stage_in(term_ids, (size_t)total, dev, b->in_ids, s);
            const float *d_imp = stage_in(impacts, (size_t)total, dev, b->in_imp, s);
            const int32_t *d_cu = stage_in(cu_terms, (size_t)n_docs + 1, dev, b->in_cu, s);
            {
                TimedLaunch tl(b->timer, timing, "ib_append", s);
                hipLaunchKernelGGL(ib_append_kernel, dim3(grid_for(total, IB_THREADS)),
                                   dim3(IB_THREADS), 0, s, d_ids, d_imp, d_cu, n_docs, total,
                                   (uint32_t)b->n_docs, b->n_pairs, b->n_pairs + total, false,
                                   b->tid.as<uint32_t>(), b->doc.as<uint32_t>(),
                                   b->imp.as<float>());
                check_launch("ib_append");
            }
            DI_HIP(hipStreamSynchronize(s));
            b->timer.resolve();
        }
        b->empty_docs.insert(b->empty_docs.end(), empty.begin(), empty.end());
        b->n_pairs += total;
        b->n_docs += n_docs;
        b->n_kept = -1;  // (the kept records are those of the pairs before this append)
    });
}

int di_index_builder_append_pairwise(di_index_builder *b, const uint32_t *term_ids,
                                     const float *single, const float *pair,
                                     const int32_t *cu_terms, const int64_t *cu_pairs,
                                     int32_t n_docs, int64_t n_pairs, int64_t *first_doc,
                                     void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(b && cu_terms && cu_pairs && first_doc && n_docs >= 0 && n_pairs >= 0,
                   DI_EINVAL, "bad argument");
        DI_REQUIRE(b->n_docs + n_docs <= (int64_t)UINT32_MAX, DI_ERANGE,
                   "%lld docs: doc ids are 32-bit", (long long)(b->n_docs + n_docs));
        DeviceScope ds(b->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        *first_doc = b->n_docs;
        if (n_docs == 0) return;
        // both offset arrays are checked on the host before anything changes
        std::vector<int32_t> h_cu;
        std::vector<int64_t> h_cup;
        const int32_t *cu = host_cu(cu_terms, n_docs, dev, h_cu, s);
        const int64_t *cup = host_cu(cu_pairs, n_docs, dev, h_cup, s);
        const int64_t total = check_cu(cu, n_docs, "cu_terms");
        const int64_t ptotal = check_cu(cup, n_docs, "cu_pairs");
        DI_REQUIRE(ptotal == n_pairs, DI_EINVAL, "cu_pairs ends at %lld, n_pairs = %lld",
                   (long long)ptotal, (long long)n_pairs);
        std::vector<int64_t> empty;
        for (int32_t d = 0; d < n_docs; ++d) {
            const int64_t T = (int64_t)cu[d + 1] - cu[d];
            DI_REQUIRE(cup[d + 1] - cup[d] == T * (T - 1) / 2, DI_EINVAL,
                       "document %d has %lld terms and %lld pairs, not T(T-1)/2 = %lld", d,
                       (long long)T, (long long)(cup[d + 1] - cup[d]), (long long)(T * (T - 1) / 2));
            if (T == 0) empty.push_back(b->n_docs + d);
        }
        DI_REQUIRE(total == 0 || (term_ids && single), DI_EINVAL, "null input");
        DI_REQUIRE(ptotal == 0 || pair, DI_EINVAL, "null pair scores");
        int64_t kept = 0;
        if (total > 0) {
            ib_reserve(b, b->n_pairs + total, s);
            const uint32_t *d_ids = stage_in(term_ids, (size_t)total, dev, b->in_ids, s);
            const float *d_imp = stage_in(single, (size_t)total, dev, b->in_imp, s);
            const int32_t *d_cu = stage_in(cu_terms, (size_t)n_docs + 1, dev, b->in_cu, s);
            {
                TimedLaunch tl(b->timer, timing, "ib_append", s);
                hipLaunchKernelGGL(ib_append_kernel, dim3(grid_for(total, IB_THREADS)),
                                   dim3(IB_THREADS), 0, s, d_ids, d_imp, d_cu, n_docs, total,
                                   (uint32_t)b->n_docs, b->n_pairs, b->n_pairs + total, true,
                                   b->tid.as<uint32_t>(), b->doc.as<uint32_t>(),
                                   b->imp.as<float>());
                check_launch("ib_append");
            }
            if (ptotal > 0) {
                const float *d_pair = stage_in(pair, (size_t)ptotal, dev, b->in_pair, s);
                const int64_t *d_cup = stage_in(cu_pairs, (size_t)n_docs + 1, dev, b->in_cup, s);
                const int64_t n_tiles = (ptotal + IB_TILE - 1) / IB_TILE;
                b->p_cnt.reserve((size_t)n_tiles * 4);
                b->p_off.reserve((size_t)n_tiles * 8);
                {
                    TimedLaunch tl(b->timer, timing, "ib_pair_append", s);
                    hipLaunchKernelGGL(ib_pair_count_kernel, dim3(grid_for(n_tiles, 1)),
                                       dim3(IB_THREADS), 0, s, d_pair, ptotal, n_tiles,
                                       b->p_cnt.as<uint32_t>());
                    check_launch("ib_pair_count");
                }
                kept = ib_scan(b, b->p_cnt.as<uint32_t>(), n_tiles, b->p_off.as<int64_t>(), timing, s);
                DI_REQUIRE(kept >= 0 && kept <= ptotal, DI_EHIP,
                           "ib_pair_count kept %lld of %lld pairs", (long long)kept,
                           (long long)ptotal);
                if (kept > 0) {
                    ib_pair_reserve(b, b->n_precs + kept, s);
                    TimedLaunch tl(b->timer, timing, "ib_pair_append", s);
                    hipLaunchKernelGGL(ib_pair_place_kernel, dim3(grid_for(n_tiles, 1)),
                                       dim3(IB_THREADS), 0, s, d_ids, d_pair, d_cu, d_cup, n_docs,
                                       ptotal, n_tiles, b->p_off.as<int64_t>(), (uint32_t)b->n_docs,
                                       b->n_precs, b->n_precs + kept, b->pa.as<uint32_t>(),
                                       b->pb.as<uint32_t>(), b->pdoc.as<uint32_t>(),
                                       b->pimp.as<float>());
                    check_launch("ib_pair_place");
                }
            }
            DI_HIP(hipStreamSynchronize(s));
            b->timer.resolve();
        }
        b->empty_docs.insert(b->empty_docs.end(), empty.begin(), empty.end());
        b->n_pairs += total;
        b->n_precs += kept;
        b->n_docs += n_docs;
        b->n_kept = -1;  // (the kept records are those of the pairs before this append)
    });
}

int di_index_builder_pair_terms(const di_index_builder *b, int64_t *n_pair_terms,
                                uint32_t *first_id, uint32_t *second_id, int64_t *count) {
    return guard([&] {
        DI_REQUIRE(b && n_pair_terms, DI_EINVAL, "bad argument");
        DI_REQUIRE(b->n_kept >= 0, DI_EINVAL, "di_index_builder_quantize comes first");
        const size_t n = b->pt_first.size(), n_single = (size_t)b->n_terms - n;
        *n_pair_terms = (int64_t)n;
        if (n == 0) return;
        if (first_id) std::memcpy(first_id, b->pt_first.data(), n * 4);
        if (second_id) std::memcpy(second_id, b->pt_second.data(), n * 4);
        if (count) std::memcpy(count, b->tcount.data() + n_single, n * 8);
    });
}

int di_index_builder_info(const di_index_builder *b, int64_t *n_docs, int64_t *n_pairs) {
    return guard([&] {
        DI_REQUIRE(b, DI_EINVAL, "null handle");
        if (n_docs) *n_docs = b->n_docs;
        if (n_pairs) *n_pairs = b->n_pairs;
    });
}

int di_index_builder_quantize(di_index_builder *b, int64_t n_terms, double max_val,
                              void *hip_stream, uint32_t flags, double *max_used,
                              int64_t *term_count, int64_t *n_kept) {
    return guard([&] {
        DI_REQUIRE(b && n_terms >= 0 && n_kept && (term_count || n_terms == 0), DI_EINVAL,
                   "bad argument");
        DI_REQUIRE(n_terms <= (int64_t)UINT32_MAX, DI_ERANGE, "term ids are 32-bit");
        DI_REQUIRE(b->empty_docs.empty(), DI_EFORMAT,
                   "document %lld has no terms: its impact line is empty (quantize_file raises "
                   "ValueError, quantize.py:21)",
                   (long long)(b->empty_docs.empty() ? 0 : b->empty_docs[0]));
        DeviceScope ds(b->device);
        const bool timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        const int64_t n = b->n_pairs;
        const int64_t n_tiles = (n + IB_TILE - 1) / IB_TILE;
        Ctrl *ctrl = b->ctrl.as<Ctrl>();
        Ctrl h{};
        DI_HIP(hipMemsetAsync(ctrl, 0, sizeof(Ctrl), s));
        if (n > 0) {
            TimedLaunch tl(b->timer, timing, "ib_quantize", s);
            hipLaunchKernelGGL(ib_max_kernel, dim3(grid_for(n, IB_THREADS * 8)), dim3(IB_THREADS),
                               0, s, b->imp.as<float>(), n, ctrl);
            check_launch("ib_max");
        }
        const int64_t np = b->n_precs, np_tiles = (np + IB_TILE - 1) / IB_TILE;
        if (np > 0) {  // the maximum runs over singles and pairs
            TimedLaunch tl(b->timer, timing, "ib_pair_quantize", s);
            hipLaunchKernelGGL(ib_max_kernel, dim3(grid_for(np, IB_THREADS * 8)), dim3(IB_THREADS),
                               0, s, b->pimp.as<float>(), np, ctrl);
            check_launch("ib_max");
        }
        read_back(h, ctrl, s, &b->timer);
        DI_REQUIRE(!(h.err & IB_ERR_NONFINITE), DI_EFORMAT,
                   "an impact is not finite (int() of it raises in quantize.py:45)");
        float mf;
        std::memcpy(&mf, &h.max_bits, 4);
        const double m = max_val > 0.0 ? max_val : (double)mf;
        if (max_used) *max_used = m;
        DI_REQUIRE(m > 0.0, DI_EINVAL,
                   "max impact is 0: the reference divides by zero (quantize.py:37)");
        const double scale = 255.0 / m;
        b->qval.reserve(at_least_one(n));
        b->cnt.reserve(at_least_one(n_tiles) * 4);
        b->off.reserve(at_least_one(n_tiles) * 8);
        b->dcount.reserve(at_least_one(n_terms) * 8);
        DI_HIP(hipMemsetAsync(b->dcount.p, 0, at_least_one(n_terms) * 8, s));
        int64_t total = 0;
        if (n > 0) {
            {
                TimedLaunch tl(b->timer, timing, "ib_quantize", s);
                hipLaunchKernelGGL(ib_quantize_kernel, dim3(grid_for(n_tiles, 1)),
                                   dim3(IB_THREADS), 0, s, b->tid.as<uint32_t>(),
                                   b->imp.as<float>(), n, n_tiles, n_terms, scale,
                                   b->qval.as<uint8_t>(), b->cnt.as<uint32_t>(),
                                   b->dcount.as<unsigned long long>(), ctrl);
                check_launch("ib_quantize");
            }
            read_back(h, ctrl, s, &b->timer);
            DI_REQUIRE(!(h.err & IB_ERR_TERM), DI_EINVAL, "a term id is not below n_terms = %lld",
                       (long long)n_terms);
            DI_REQUIRE(!(h.err & IB_ERR_RANGE), DI_ERANGE,
                       "a value is above 255 with max_val = %.17g (struct.pack('B') fails in "
                       "create.py:45)", m);
            total = ib_scan(b, b->cnt.as<uint32_t>(), n_tiles, b->off.as<int64_t>(), timing, s);
            DI_REQUIRE(total >= 0 && total <= n, DI_EHIP, "ib_quantize kept %lld of %lld pairs",
                       (long long)total, (long long)n);
        }
        int64_t ptotal = 0;  // kept pair records
        if (np > 0) {
            b->p_qval.reserve((size_t)np);
            b->p_cnt.reserve((size_t)np_tiles * 4);
            b->p_off.reserve((size_t)np_tiles * 8);
            {
                TimedLaunch tl(b->timer, timing, "ib_pair_quantize", s);
                hipLaunchKernelGGL(ib_pair_quantize_kernel, dim3(grid_for(np_tiles, 1)),
                                   dim3(IB_THREADS), 0, s, b->pa.as<uint32_t>(),
                                   b->pb.as<uint32_t>(), b->pimp.as<float>(), np, np_tiles, n_terms,
                                   scale, b->p_qval.as<uint8_t>(), b->p_cnt.as<uint32_t>(), ctrl);
                check_launch("ib_pair_quantize");
            }
            read_back(h, ctrl, s, &b->timer);
            DI_REQUIRE(!(h.err & IB_ERR_TERM), DI_EINVAL, "a term id is not below n_terms = %lld",
                       (long long)n_terms);
            DI_REQUIRE(!(h.err & IB_ERR_RANGE), DI_ERANGE,
                       "a value is above 255 with max_val = %.17g (struct.pack('B') fails in "
                       "create.py:45)", m);
            ptotal = ib_scan(b, b->p_cnt.as<uint32_t>(), np_tiles, b->p_off.as<int64_t>(), timing, s);
            DI_REQUIRE(ptotal >= 0 && ptotal <= np, DI_EHIP,
                       "ib_pair_quantize kept %lld of %lld pairs", (long long)ptotal, (long long)np);
        }
        // from here on the result of an earlier quantize is replaced
        b->n_kept = -1;
        b->kept.reserve(at_least_one(total + ptotal) * sizeof(uint4));
        if (total > 0) {
            TimedLaunch tl(b->timer, timing, "ib_compact", s);
            hipLaunchKernelGGL(ib_compact_kernel, dim3(grid_for(n_tiles, 1)), dim3(IB_THREADS), 0,
                               s, b->tid.as<uint32_t>(), b->doc.as<uint32_t>(),
                               b->qval.as<uint8_t>(), n, n_tiles, n_terms, b->off.as<int64_t>(),
                               total, b->kept.as<uint4>());
            check_launch("ib_compact");
        }
        // the kept pair records: sorted by (id_a, id_b), numbered, behind the single ones
        int64_t n_runs = 0;
        std::vector<int64_t> h_start;
        b->pt_first.clear();
        b->pt_second.clear();
        if (ptotal > 0) {
            b->sort_a.reserve((size_t)ptotal * sizeof(uint4));
            b->sort_b.reserve((size_t)ptotal * sizeof(uint4));
            {
                TimedLaunch tl(b->timer, timing, "ib_pair_compact", s);
                hipLaunchKernelGGL(ib_pair_compact_kernel, dim3(grid_for(np_tiles, 1)),
                                   dim3(IB_THREADS), 0, s, b->pa.as<uint32_t>(),
                                   b->pb.as<uint32_t>(), b->pdoc.as<uint32_t>(),
                                   b->p_qval.as<uint8_t>(), np, np_tiles, b->p_off.as<int64_t>(),
                                   ptotal, b->sort_a.as<uint4>());
                check_launch("ib_pair_compact");
            }
            int id_passes = 0;  // per half of the key: both ids are below n_terms
            for (int64_t top = n_terms - 1; top > 0; top >>= 8) ++id_passes;
            uint4 *src = b->sort_a.as<uint4>(), *dst = b->sort_b.as<uint4>();
            for (int p = 0; p < 2 * id_passes; ++p) {  // least significant first: id_b, then id_a
                const bool on_y = p >= id_passes;
                ib_sort_pass(b, src, dst, ptotal, on_y, 8 * (on_y ? p - id_passes : p), nullptr, 0,
                             timing, "ib_pair_hist", "ib_pair_scatter", s);
                std::swap(src, dst);
            }
            b->p_cnt.reserve((size_t)ptotal * 4);
            b->p_off.reserve((size_t)ptotal * 8);
            {
                TimedLaunch tl(b->timer, timing, "ib_pair_number", s);
                hipLaunchKernelGGL(ib_pair_heads_kernel, dim3(grid_for(ptotal, IB_THREADS)),
                                   dim3(IB_THREADS), 0, s, src, ptotal, b->p_cnt.as<uint32_t>());
                check_launch("ib_pair_heads");
            }
            n_runs = ib_scan(b, b->p_cnt.as<uint32_t>(), ptotal, b->p_off.as<int64_t>(), timing, s);
            DI_REQUIRE(n_runs >= 1 && n_runs <= ptotal, DI_EHIP,
                       "ib_pair_heads found %lld runs in %lld records", (long long)n_runs,
                       (long long)ptotal);
            DI_REQUIRE(n_terms + n_runs <= (int64_t)INT32_MAX, DI_ERANGE,
                       "%lld single and %lld pair terms: rows are 31-bit", (long long)n_terms,
                       (long long)n_runs);
            b->p_first.reserve((size_t)n_runs * 4);
            b->p_second.reserve((size_t)n_runs * 4);
            b->p_start.reserve((size_t)n_runs * 8);
            {
                TimedLaunch tl(b->timer, timing, "ib_pair_number", s);
                hipLaunchKernelGGL(ib_pair_number_kernel, dim3(grid_for(ptotal, IB_THREADS)),
                                   dim3(IB_THREADS), 0, s, src, ptotal, b->p_cnt.as<uint32_t>(),
                                   b->p_off.as<int64_t>(), n_terms, n_runs,
                                   b->kept.as<uint4>() + total, b->p_first.as<uint32_t>(),
                                   b->p_second.as<uint32_t>(), b->p_start.as<int64_t>());
                check_launch("ib_pair_number");
            }
            b->pt_first.resize((size_t)n_runs);
            b->pt_second.resize((size_t)n_runs);
            h_start.resize((size_t)n_runs);
            DI_HIP(hipMemcpyAsync(b->pt_first.data(), b->p_first.p, (size_t)n_runs * 4,
                                  hipMemcpyDeviceToHost, s));
            DI_HIP(hipMemcpyAsync(b->pt_second.data(), b->p_second.p, (size_t)n_runs * 4,
                                  hipMemcpyDeviceToHost, s));
            DI_HIP(hipMemcpyAsync(h_start.data(), b->p_start.p, (size_t)n_runs * 8,
                                  hipMemcpyDeviceToHost, s));
        }
        b->tcount.assign((size_t)(n_terms + n_runs), 0);
        if (n_terms > 0)
            DI_HIP(hipMemcpyAsync(b->tcount.data(), b->dcount.p, (size_t)n_terms * 8,
                                  hipMemcpyDeviceToHost, s));
        DI_HIP(hipStreamSynchronize(s));
        b->timer.resolve();
        for (int64_t u = 0; u < n_runs; ++u)  // a run ends where the next one starts
            b->tcount[(size_t)(n_terms + u)] =
                (u + 1 < n_runs ? h_start[(size_t)u + 1] : ptotal) - h_start[(size_t)u];
        if (n_terms > 0) std::memcpy(term_count, b->tcount.data(), (size_t)n_terms * 8);
        b->n_terms = n_terms + n_runs;
        b->n_kept = total + ptotal;
        *n_kept = total + ptotal;
    });
}

int di_index_builder_postings(di_index_builder *b, const int32_t *term_row, int64_t n_rows,
                              void *hip_stream, uint32_t flags, int64_t *term_off, uint32_t *pdoc,
                              uint8_t *pval) {
    return guard([&] {
        DI_REQUIRE(b && n_rows >= 0 && term_off, DI_EINVAL, "bad argument");
        DI_REQUIRE(b->n_kept >= 0, DI_EINVAL, "di_index_builder_quantize comes first");
        DI_REQUIRE(n_rows <= (int64_t)INT32_MAX, DI_ERANGE, "rows are 31-bit");
        const int64_t n = b->n_kept, n_terms = b->n_terms;
        DI_REQUIRE(n == 0 || (pdoc && pval), DI_EINVAL, "null output");
        DI_REQUIRE(n_terms == 0 || term_row, DI_EINVAL, "null term_row");
        // rows: every term with a kept posting has one, and no row is given twice
        std::vector<int64_t> h_off((size_t)n_rows + 1, 0);
        {
            std::vector<uint8_t> seen((size_t)n_rows, 0);
            for (int64_t t = 0; t < n_terms; ++t) {
                const int64_t r = term_row[t];
                DI_REQUIRE(r >= 0 || b->tcount[(size_t)t] == 0, DI_EINVAL,
                           "term id %lld keeps %lld postings and has no row", (long long)t,
                           (long long)b->tcount[(size_t)t]);
                if (r < 0) continue;
                DI_REQUIRE(r < n_rows, DI_EINVAL, "term id %lld: row %lld is not below n_rows = %lld",
                           (long long)t, (long long)r, (long long)n_rows);
                DI_REQUIRE(!seen[(size_t)r], DI_EINVAL, "row %lld is given to two terms",
                           (long long)r);
                seen[(size_t)r] = 1;
                h_off[(size_t)r + 1] = b->tcount[(size_t)t];
            }
            for (int64_t r = 0; r < n_rows; ++r) h_off[(size_t)r + 1] += h_off[(size_t)r];
        }
        DeviceScope ds(b->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        if (dev)
            DI_HIP(hipMemcpyAsync(term_off, h_off.data(), h_off.size() * 8, hipMemcpyHostToDevice, s));
        if (n > 0) {
            int row_passes = 0;
            for (int64_t top = n_rows - 1; top > 0; top >>= 8) ++row_passes;
            const int32_t *d_row = stage_in(term_row, (size_t)n_terms, false, b->d_row, s);
            b->sort_a.reserve((size_t)n * sizeof(uint4));
            if (row_passes > 0) b->sort_b.reserve((size_t)n * sizeof(uint4));
            const uint4 *src = b->kept.as<uint4>();
            for (int p = 0; p <= row_passes; ++p) {
                uint4 *dst = (p % 2 == 0 ? b->sort_a : b->sort_b).as<uint4>();
                const bool by_row = p > 0;
                ib_sort_pass(b, src, dst, n, by_row, by_row ? 8 * (p - 1) : 0,
                             p == 0 ? d_row : nullptr, n_terms, timing, "ib_hist", "ib_scatter", s);
                src = dst;
            }
            StagedOut<uint32_t> o_doc(pdoc, (size_t)n, dev, b->o_doc);
            StagedOut<uint8_t> o_val(pval, (size_t)n, dev, b->o_val);
            const bool vec = (uintptr_t)o_doc.d % 16 == 0 && (uintptr_t)o_val.d % 4 == 0;
            {
                TimedLaunch tl(b->timer, timing, "ib_extract", s);
                hipLaunchKernelGGL(ib_extract_kernel, dim3(grid_for((n + 3) / 4, IB_THREADS)),
                                   dim3(IB_THREADS), 0, s, src, n, o_doc.d, o_val.d, vec);
                check_launch("ib_extract");
            }
            o_doc.copy_back(s);
            o_val.copy_back(s);
        }
        DI_HIP(hipStreamSynchronize(s));
        b->timer.resolve();
        if (!dev) std::memcpy(term_off, h_off.data(), h_off.size() * 8);
    });
}

int di_index_builder_timing(di_index_builder *b, const char *name, di_timing *out, int reset) {
    return guard([&] {
        DI_REQUIRE(b && name && out, DI_EINVAL, "bad argument");
        b->timer.get(name, out, reset != 0);
    });
}

int di_index_builder_destroy(di_index_builder *b) {
    return guard([&] {
        if (!b) return;
        DeviceScope ds(b->device);
        delete b;
    });
}

}  // extern "C"
