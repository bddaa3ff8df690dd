// sparse_build.hip -- the float index (sparse.hip's layout) assembled on the device from
// (term id, impact) pairs per document, e.g. di_encode's output buffer, gfx950.
//
// Replaces SparseSearch._build_inverted_index (reference src/deep_impact/evaluation/
// nano_beir_evaluator.py:78-101) and di_sparse_create's host loop for inputs that are
// already on the device.  The layout is a counting problem, not a sort:
//   sb_append      every pair finds its document by a search of cu_terms; pairs with
//                  impact > 0 (:98) are compacted as (term, doc, impact) behind the
//                  builder's end (one atomic add of a wave's count; the order in that
//                  buffer is arbitrary and does not reach the result)
//   sb_count       one atomic add per posting on the dense n_terms x (nb + 1) table that
//                  becomes blk_off; the returned old count is the posting's slot inside
//                  its (term, block) segment
//   sb_rows / sb_chunk_sum / sb_chunk_scan / sb_term_start
//                  exclusive scan of every row in place (total in its last column) and
//                  of the row totals into term_start (int64)
//   sb_scatter     plain stores: posting -> term_start + blk_off + slot of a staging copy
//   sb_order_short one wave per segment of <= 64 postings: a lane's place is the number
//                  of smaller docs among its wave-mates; an equal doc is a repeat
//   sb_order_long  one workgroup per longer segment (<= 16384 distinct 14-bit docs): an
//                  LDS presence bitmap set with atomicOr (an old bit already set is the
//                  repeat), a prefix sum of the 512 word popcounts, and each posting goes
//                  to prefix[word] + popcount(bits below)
// Every segment ends in ascending doc order whatever slots the atomics handed out, so the
// bytes are those of di_sparse_create.  Work per posting: one search of cu_terms
// (log2 n_docs cached loads), one global atomic, two plain 6-byte stores, and <= 64
// shuffles (short) or one LDS atomic (long).
#include <hip/hip_runtime.h>

#include <memory>

#include "sparse_common.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int SB_THREADS = 256, SB_WAVES = SB_THREADS / 64;
constexpr int SB_MAX_GRID = 1 << 16;  // blocks of a grid-stride launch
constexpr int SB_SHORT = 64;          // postings of a segment one wave orders
constexpr int SB_WORDS = SP_DOCS / 32;  // words of a block's presence bitmap

constexpr int SB_ERR_TERM = 1;  // a term id >= n_terms
constexpr int SB_ERR_DUP = 2;   // a (term, doc) posting twice
constexpr int SB_ERR_SIZE = 4;  // a segment outside the posting arrays (counts wrapped)

struct Ctrl {
    int32_t err;
    uint32_t n_long;
};

__global__ void __launch_bounds__(SB_THREADS)
sb_append_kernel(const uint32_t *__restrict__ term_ids, const float *__restrict__ impacts,
                 const int32_t *__restrict__ cu_terms, int n_docs, int64_t total, uint32_t doc0,
                 int64_t base, int64_t cap, uint32_t *__restrict__ o_tid,
                 uint32_t *__restrict__ o_doc, float *__restrict__ o_imp,
                 unsigned long long *__restrict__ kept) {
    const int lane = lane_id();
    for (int64_t i0 = (int64_t)blockIdx.x * SB_THREADS; i0 < total;
         i0 += (int64_t)gridDim.x * SB_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        float x = 0.f;
        if (i < total) x = impacts[i];
        const bool keep = i < total && x > 0.f;  // false for -0.0, 0.0, negatives, NaN
        const uint64_t m = __ballot(keep);
        if (!m) continue;  // (the same for the whole wave)
        unsigned long long w = 0;
        if (lane == 0) w = atomicAdd(kept, (unsigned long long)__popcll(m));
        w = (unsigned long long)__shfl((long long)w, 0, 64);
        if (!keep) continue;
        int lo = 0, hi = n_docs;  // the last document with cu_terms[d] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cu_terms[mid] <= i) lo = mid; else hi = mid;
        }
        const int64_t pos = base + (int64_t)w + __popcll(m & ((1ull << lane) - 1));
        if (pos < cap) {  // (always: the buffers hold base + total pairs)
            o_tid[pos] = term_ids[i];
            o_doc[pos] = doc0 + (uint32_t)lo;
            o_imp[pos] = x;
        }
    }
}

__global__ void __launch_bounds__(SB_THREADS)
sb_count_kernel(const uint32_t *__restrict__ tid, const uint32_t *__restrict__ doc, int64_t n,
                int64_t n_terms, int64_t stride, uint32_t *__restrict__ table,
                uint32_t *__restrict__ slot, Ctrl *__restrict__ ctrl) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * SB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * SB_THREADS) {
        const uint32_t t = tid[i];
        if (t >= n_terms) {
            bad = true;
            continue;
        }
        slot[i] = atomicAdd(&table[(int64_t)t * stride + doc[i] / SP_DOCS], 1u);
    }
    if (bad) atomicOr(&ctrl->err, SB_ERR_TERM);
}

// One wave per row: counts -> exclusive offsets in place, the row's total in column nb.
__global__ void __launch_bounds__(SB_THREADS)
sb_rows_kernel(uint32_t *__restrict__ table, int64_t n_terms, int nb) {
    const int lane = lane_id();
    for (int64_t t = (int64_t)blockIdx.x * SB_WAVES + wave_id(); t < n_terms;
         t += (int64_t)gridDim.x * SB_WAVES) {
        uint32_t *r = table + t * (nb + 1);
        uint32_t carry = 0;
        for (int b0 = 0; b0 < nb; b0 += 64) {
            const int b = b0 + lane;
            const uint32_t c = b < nb ? r[b] : 0;
            const uint32_t inc = wave_prefix_sum(c);
            if (b < nb) r[b] = carry + inc - c;
            carry += __shfl(inc, 63, 64);
        }
        if (lane == 0) r[nb] = carry;
    }
}

// Inclusive sum over the workgroup's threads in thread order; *total = the workgroup's sum.
__device__ __forceinline__ int64_t block_incl_scan64(int64_t v, int64_t *wtot, int64_t *total) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up((long long)v, d, 64);
        if (lane_id() >= d) v += y;
    }
    __syncthreads();  // wtot is free again
    if (lane_id() == 63) wtot[wave_id()] = v;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < SB_WAVES; ++w) {
        if (w < wave_id()) before += wtot[w];
        all += wtot[w];
    }
    *total = all;
    return v + before;
}

// csum[c] = the postings of terms [c * SB_THREADS, (c + 1) * SB_THREADS)
__global__ void __launch_bounds__(SB_THREADS)
sb_chunk_sum_kernel(const uint32_t *__restrict__ table, int64_t n_terms, int nb,
                    int64_t *__restrict__ csum) {
    __shared__ int64_t wtot[SB_WAVES];
    const int64_t t = (int64_t)blockIdx.x * SB_THREADS + threadIdx.x;
    int64_t total;
    block_incl_scan64(t < n_terms ? (int64_t)table[t * (nb + 1) + nb] : 0, wtot, &total);
    if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

// One workgroup: csum -> its exclusive scan, in place.
__global__ void __launch_bounds__(SB_THREADS)
sb_chunk_scan_kernel(int64_t *__restrict__ csum, int64_t n_chunks) {
    __shared__ int64_t wtot[SB_WAVES];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += SB_THREADS) {
        const int64_t c = c0 + threadIdx.x;
        const int64_t v = c < n_chunks ? csum[c] : 0;
        int64_t total;
        const int64_t inc = block_incl_scan64(v, wtot, &total);
        if (c < n_chunks) csum[c] = carry + inc - v;
        carry += total;
    }
}

__global__ void __launch_bounds__(SB_THREADS)
sb_term_start_kernel(const uint32_t *__restrict__ table, int64_t n_terms, int nb,
                     const int64_t *__restrict__ csum, int64_t *__restrict__ term_start) {
    __shared__ int64_t wtot[SB_WAVES];
    const int64_t t = (int64_t)blockIdx.x * SB_THREADS + threadIdx.x;
    const int64_t v = t < n_terms ? (int64_t)table[t * (nb + 1) + nb] : 0;
    int64_t total;
    const int64_t inc = block_incl_scan64(v, wtot, &total);
    if (t < n_terms) term_start[t] = csum[blockIdx.x] + inc - v;
}

__global__ void __launch_bounds__(SB_THREADS)
sb_scatter_kernel(const uint32_t *__restrict__ tid, const uint32_t *__restrict__ doc,
                  const float *__restrict__ imp, const uint32_t *__restrict__ slot, int64_t n,
                  int64_t n_terms, int64_t stride, const uint32_t *__restrict__ table,
                  const int64_t *__restrict__ term_start, uint16_t *__restrict__ s_doc,
                  float *__restrict__ s_imp) {
    for (int64_t i = (int64_t)blockIdx.x * SB_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * SB_THREADS) {
        const uint32_t t = tid[i];
        if (t >= n_terms) continue;
        const uint32_t d = doc[i];
        const int64_t pos = term_start[t] + table[(int64_t)t * stride + d / SP_DOCS] + slot[i];
        if (pos < n) {  // (always, unless a count wrapped: reported by the order kernels)
            s_doc[pos] = (uint16_t)(d % SP_DOCS);
            s_imp[pos] = imp[i];
        }
    }
}

// One wave per (term, block) segment; the segments of more than SB_SHORT postings are
// listed for sb_order_long (the list's order does not matter).
__global__ void __launch_bounds__(SB_THREADS)
sb_order_short_kernel(const uint32_t *__restrict__ table, const int64_t *__restrict__ term_start,
                      int64_t n_terms, int nb, int64_t n, const uint16_t *__restrict__ s_doc,
                      const float *__restrict__ s_imp, uint16_t *__restrict__ o_doc,
                      float *__restrict__ o_imp, int64_t *__restrict__ long_list,
                      uint32_t long_cap, Ctrl *__restrict__ ctrl) {
    const int lane = lane_id();
    const int64_t n_seg = n_terms * nb;
    for (int64_t seg = (int64_t)blockIdx.x * SB_WAVES + wave_id(); seg < n_seg;
         seg += (int64_t)gridDim.x * SB_WAVES) {
        const int64_t t = seg / nb;
        const uint32_t *r = table + t * (nb + 1) + (seg - t * nb);
        const uint32_t lo = r[0], cnt = r[1] - lo;
        if (cnt == 0) continue;
        const int64_t s = term_start[t] + lo;
        if (s < 0 || s + cnt > n) {
            if (lane == 0) atomicOr(&ctrl->err, SB_ERR_SIZE);
            continue;
        }
        if (cnt > SB_SHORT) {
            if (lane == 0) {
                const uint32_t k = atomicAdd(&ctrl->n_long, 1u);
                if (k < long_cap) long_list[k] = seg;
                else atomicOr(&ctrl->err, SB_ERR_SIZE);
            }
            continue;
        }
        const bool live = lane < (int)cnt;
        const uint32_t d = live ? s_doc[s + lane] : 0xFFFFFFFFu;
        const float x = live ? s_imp[s + lane] : 0.f;
        int place = 0;
        bool dup = false;
        for (int j = 0; j < (int)cnt; ++j) {
            const uint32_t dj = __shfl(d, j, 64);
            place += dj < d;
            dup |= dj == d && j != lane;
        }
        if (live) {
            o_doc[s + place] = (uint16_t)d;
            o_imp[s + place] = x;
            if (dup) atomicOr(&ctrl->err, SB_ERR_DUP);
        }
    }
}

__global__ void __launch_bounds__(SB_THREADS)
sb_order_long_kernel(const uint32_t *__restrict__ table, const int64_t *__restrict__ term_start,
                     int nb, const uint16_t *__restrict__ s_doc, const float *__restrict__ s_imp,
                     uint16_t *__restrict__ o_doc, float *__restrict__ o_imp,
                     const int64_t *__restrict__ long_list, uint32_t long_cap,
                     Ctrl *__restrict__ ctrl) {
    __shared__ uint32_t bits[SB_WORDS];
    __shared__ uint32_t pre[SB_WORDS];
    __shared__ uint32_t wtot[SB_WAVES];
    static_assert(SB_WORDS == 2 * SB_THREADS, "two bitmap words a thread");
    const int tid = threadIdx.x;
    const uint32_t n_long = min(ctrl->n_long, long_cap);
    for (uint32_t k = blockIdx.x; k < n_long; k += gridDim.x) {
        const int64_t seg = long_list[k];
        const int64_t t = seg / nb;
        const uint32_t *r = table + t * (nb + 1) + (seg - t * nb);
        const uint32_t lo = r[0], cnt = r[1] - lo;  // (in bounds: checked when listed)
        const int64_t s = term_start[t] + lo;
        bits[tid] = 0;
        bits[tid + SB_THREADS] = 0;
        __syncthreads();
        bool dup = false;
        for (uint32_t i = tid; i < cnt; i += SB_THREADS) {
            const uint32_t d = s_doc[s + i] & (SP_DOCS - 1);
            const uint32_t bit = 1u << (d & 31);
            dup |= (atomicOr(&bits[d >> 5], bit) & bit) != 0;
        }
        if (dup) atomicOr(&ctrl->err, SB_ERR_DUP);
        __syncthreads();
        const uint32_t w0 = bits[2 * tid], w1 = bits[2 * tid + 1];
        const uint32_t c = __popc(w0) + __popc(w1);
        const uint32_t inc = wave_prefix_sum(c);
        if (lane_id() == 63) wtot[wave_id()] = inc;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave_id(); ++w) before += wtot[w];
        pre[2 * tid] = before + inc - c;
        pre[2 * tid + 1] = before + inc - c + __popc(w0);
        __syncthreads();
        // (with a repeat the places stay below the distinct docs' count <= cnt)
        for (uint32_t i = tid; i < cnt; i += SB_THREADS) {
            const uint32_t d = s_doc[s + i] & (SP_DOCS - 1);
            const uint32_t place = pre[d >> 5] + __popc(bits[d >> 5] & ((1u << (d & 31)) - 1));
            o_doc[s + place] = (uint16_t)d;
            o_imp[s + place] = s_imp[s + i];
        }
        __syncthreads();  // bits, pre and wtot are free again
    }
}

inline int grid_for(int64_t items, int per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block,
                                                       SB_MAX_GRID));
}

}  // namespace
}  // namespace di

struct di_sparse_builder {
    int device = 0;
    int64_t n_docs = 0, n_pairs = 0;  // documents appended, pairs kept
    di::DevBuf tid, doc, imp;         // the kept pairs, in no particular order
    di::DevBuf kept, in_ids, in_imp, in_cu;
    di::Timer timer;
};

using namespace di;

namespace {

void sb_reserve(di_sparse_builder *b, int64_t n_pairs, hipStream_t s) {
    const size_t need = (size_t)std::max<int64_t>(n_pairs, 1) * 4, used = (size_t)b->n_pairs * 4;
    grow_keep(b->tid, need, used, s);
    grow_keep(b->doc, need, used, s);
    grow_keep(b->imp, need, used, s);
}

struct SparseDeleter {
    void operator()(di_sparse *sp) const {
        if (sp->own_stream && sp->stream) (void)hipStreamDestroy(sp->stream);
        delete sp;
    }
};

}  // namespace

extern "C" {

int di_sparse_builder_create(int device, di_sparse_builder **out) {
    return guard([&] {
        DI_REQUIRE(out, DI_EINVAL, "null output");
        *out = nullptr;
        check_device(device);
        DeviceScope ds(device);
        std::unique_ptr<di_sparse_builder> b(new di_sparse_builder);
        b->device = device;
        b->kept.reserve(8);
        sb_reserve(b.get(), 1, nullptr);
        *out = b.release();
    });
}

int di_sparse_builder_reserve(di_sparse_builder *b, int64_t n_docs, int64_t n_pairs) {
    return guard([&] {
        DI_REQUIRE(b && n_docs >= 0 && n_pairs >= 0, DI_EINVAL, "bad argument");
        DI_REQUIRE(n_docs <= (int64_t)DI_MAX_SPARSE_DOCS, DI_ERANGE, "%lld docs > %u",
                   (long long)n_docs, DI_MAX_SPARSE_DOCS);
        DeviceScope ds(b->device);
        sb_reserve(b, std::max(n_pairs, b->n_pairs), nullptr);
    });
}

int di_sparse_builder_append(di_sparse_builder *b, const uint32_t *term_ids,
                             const float *impacts, const int32_t *cu_terms, int32_t n_docs,
                             int64_t *first_doc, void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(b && cu_terms && first_doc && n_docs >= 0, DI_EINVAL, "bad argument");
        DI_REQUIRE(b->n_docs + n_docs <= (int64_t)DI_MAX_SPARSE_DOCS, DI_ERANGE,
                   "%lld docs > %u", (long long)(b->n_docs + n_docs), DI_MAX_SPARSE_DOCS);
        DeviceScope ds(b->device);
        const bool dev = flags & DI_F_DEVICE_PTRS, timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        *first_doc = b->n_docs;
        if (n_docs == 0) return;
        // the offsets are checked on the host before anything changes (with device
        // pointers a copy of them is read back: 4 bytes a document)
        std::vector<int32_t> h_cu;
        const int64_t total = check_cu(host_cu(cu_terms, n_docs, dev, h_cu, s), n_docs, "cu_terms");
        DI_REQUIRE(total == 0 || (term_ids && impacts), DI_EINVAL, "null input");
        if (total > 0) {
            sb_reserve(b, b->n_pairs + total, s);
            const uint32_t *d_ids = stage_in(term_ids, (size_t)total, dev, b->in_ids, s);
            const float *d_imp = stage_in(impacts, (size_t)total, dev, b->in_imp, s);
            const int32_t *d_cu = stage_in(cu_terms, (size_t)n_docs + 1, dev, b->in_cu, s);
            DI_HIP(hipMemsetAsync(b->kept.p, 0, 8, s));
            {
                TimedLaunch tl(b->timer, timing, "sb_append", s);
                hipLaunchKernelGGL(sb_append_kernel, dim3(grid_for(total, SB_THREADS)),
                                   dim3(SB_THREADS), 0, s, d_ids, d_imp, d_cu, n_docs, total,
                                   (uint32_t)b->n_docs, b->n_pairs, b->n_pairs + total,
                                   b->tid.as<uint32_t>(), b->doc.as<uint32_t>(),
                                   b->imp.as<float>(), b->kept.as<unsigned long long>());
                check_launch("sb_append");
            }
            unsigned long long kept = 0;
            read_back(kept, b->kept.p, s, &b->timer);
            DI_REQUIRE((int64_t)kept <= total, DI_EHIP, "sb_append kept %llu of %lld pairs", kept,
                       (long long)total);
            b->n_pairs += (int64_t)kept;
        }
        b->n_docs += n_docs;
    });
}

int di_sparse_builder_info(const di_sparse_builder *b, int64_t *n_docs, int64_t *n_pairs) {
    return guard([&] {
        DI_REQUIRE(b, DI_EINVAL, "null handle");
        if (n_docs) *n_docs = b->n_docs;
        if (n_pairs) *n_pairs = b->n_pairs;
    });
}

int di_sparse_builder_finish(di_sparse_builder *b, int64_t n_terms, void *hip_stream,
                             uint32_t flags, di_sparse **out) {
    return guard([&] {
        DI_REQUIRE(b && out && n_terms >= 0, DI_EINVAL, "bad argument");
        *out = nullptr;
        DI_REQUIRE(n_terms <= (int64_t)UINT32_MAX, DI_ERANGE, "term ids are 32-bit");
        DeviceScope ds(b->device);
        const bool timing = flags & DI_F_TIMING;
        hipStream_t s = (hipStream_t)hip_stream;
        const int64_t n = b->n_pairs;
        const int nb = (int)((b->n_docs + SP_DOCS - 1) / SP_DOCS);
        const int64_t stride = nb + 1, cells = n_terms * stride;
        const int64_t n_chunks = (n_terms + SB_THREADS - 1) / SB_THREADS;
        const int64_t long_cap = std::min<int64_t>(n / (SB_SHORT + 1) + 1, UINT32_MAX);
        std::unique_ptr<di_sparse, SparseDeleter> sp(new di_sparse());
        sparse_init(*sp, b->device);
        sp->n_terms = n_terms;
        sp->n_post = n;
        sp->n_docs = (uint32_t)b->n_docs;
        sp->nb = nb;
        sp->pdoc.reserve((size_t)std::max<int64_t>(n, 1) * 2);
        sp->pimp.reserve((size_t)std::max<int64_t>(n, 1) * 4);
        sp->term_start.reserve((size_t)std::max<int64_t>(n_terms, 1) * 8);
        sp->blk_off.reserve((size_t)std::max<int64_t>(cells, 1) * 4);
        DevBuf slot, s_doc, s_imp, csum, long_list, ctrl;
        slot.reserve((size_t)std::max<int64_t>(n, 1) * 4);
        s_doc.reserve((size_t)std::max<int64_t>(n, 1) * 2);
        s_imp.reserve((size_t)std::max<int64_t>(n, 1) * 4);
        csum.reserve((size_t)std::max<int64_t>(n_chunks, 1) * 8);
        long_list.reserve((size_t)long_cap * 8);
        ctrl.reserve(sizeof(Ctrl));
        DI_HIP(hipMemsetAsync(ctrl.p, 0, sizeof(Ctrl), s));
        DI_HIP(hipMemsetAsync(sp->blk_off.p, 0, (size_t)std::max<int64_t>(cells, 1) * 4, s));
        if (n_terms == 0) DI_HIP(hipMemsetAsync(sp->term_start.p, 0, 8, s));
        if (n == 0) {  // (the element di_sparse_create pads an empty index with)
            DI_HIP(hipMemsetAsync(sp->pdoc.p, 0, 2, s));
            DI_HIP(hipMemsetAsync(sp->pimp.p, 0, 4, s));
        }
        uint32_t *table = sp->blk_off.as<uint32_t>();
        int64_t *tstart = sp->term_start.as<int64_t>();
        if (n > 0) {
            TimedLaunch tl(sp->timer, timing, "sb_count", s);
            hipLaunchKernelGGL(sb_count_kernel, dim3(grid_for(n, SB_THREADS)), dim3(SB_THREADS),
                               0, s, b->tid.as<uint32_t>(), b->doc.as<uint32_t>(), n, n_terms,
                               stride, table, slot.as<uint32_t>(), ctrl.as<Ctrl>());
            check_launch("sb_count");
        }
        if (n_terms > 0) {
            TimedLaunch tl(sp->timer, timing, "sb_scan", s);
            hipLaunchKernelGGL(sb_rows_kernel, dim3(grid_for(n_terms, SB_WAVES)),
                               dim3(SB_THREADS), 0, s, table, n_terms, nb);
            check_launch("sb_rows");
            hipLaunchKernelGGL(sb_chunk_sum_kernel, dim3((unsigned)n_chunks), dim3(SB_THREADS), 0,
                               s, table, n_terms, nb, csum.as<int64_t>());
            check_launch("sb_chunk_sum");
            hipLaunchKernelGGL(sb_chunk_scan_kernel, dim3(1), dim3(SB_THREADS), 0, s,
                               csum.as<int64_t>(), n_chunks);
            check_launch("sb_chunk_scan");
            hipLaunchKernelGGL(sb_term_start_kernel, dim3((unsigned)n_chunks), dim3(SB_THREADS),
                               0, s, table, n_terms, nb, csum.as<int64_t>(), tstart);
            check_launch("sb_term_start");
        }
        if (n > 0 && n_terms > 0) {
            {
                TimedLaunch tl(sp->timer, timing, "sb_scatter", s);
                hipLaunchKernelGGL(sb_scatter_kernel, dim3(grid_for(n, SB_THREADS)),
                                   dim3(SB_THREADS), 0, s, b->tid.as<uint32_t>(),
                                   b->doc.as<uint32_t>(), b->imp.as<float>(),
                                   slot.as<uint32_t>(), n, n_terms, stride, table, tstart,
                                   s_doc.as<uint16_t>(), s_imp.as<float>());
                check_launch("sb_scatter");
            }
            TimedLaunch tl(sp->timer, timing, "sb_order", s);
            hipLaunchKernelGGL(sb_order_short_kernel, dim3(grid_for(n_terms * nb, SB_WAVES)),
                               dim3(SB_THREADS), 0, s, table, tstart, n_terms, nb, n,
                               s_doc.as<uint16_t>(), s_imp.as<float>(),
                               sp->pdoc.as<uint16_t>(), sp->pimp.as<float>(),
                               long_list.as<int64_t>(), (uint32_t)long_cap, ctrl.as<Ctrl>());
            check_launch("sb_order_short");
            hipLaunchKernelGGL(sb_order_long_kernel, dim3(grid_for(long_cap, 1)),
                               dim3(SB_THREADS), 0, s, table, tstart, nb, s_doc.as<uint16_t>(),
                               s_imp.as<float>(), sp->pdoc.as<uint16_t>(), sp->pimp.as<float>(),
                               long_list.as<int64_t>(), (uint32_t)long_cap, ctrl.as<Ctrl>());
            check_launch("sb_order_long");
        }
        Ctrl h{};
        read_back(h, ctrl.p, s, &sp->timer);
        DI_REQUIRE(!(h.err & SB_ERR_TERM), DI_EINVAL, "a term id is not below n_terms = %lld",
                   (long long)n_terms);
        DI_REQUIRE(!(h.err & SB_ERR_DUP), DI_EINVAL, "a document holds the same term id twice");
        DI_REQUIRE(!(h.err & SB_ERR_SIZE), DI_ERANGE, "a (term, block) count overflowed");
        for (const auto &kv : b->timer.acc) {  // the appends' regions, beside finish's
            auto &e = sp->timer.acc[kv.first];
            e.first += kv.second.first;
            e.second += kv.second.second;
        }
        *out = sp.release();
    });
}

int di_sparse_builder_destroy(di_sparse_builder *b) {
    return guard([&] {
        if (!b) return;
        DeviceScope ds(b->device);
        delete b;
    });
}

int di_sparse_export(const di_sparse *sp, int64_t *term_start, uint32_t *blk_off, uint16_t *pdoc,
                     float *pimp) {
    return guard([&] {
        DI_REQUIRE(sp, DI_EINVAL, "null handle");
        DeviceScope ds(sp->device);
        DI_HIP(hipStreamSynchronize(sp->stream));
        const size_t cells = (size_t)sp->n_terms * (size_t)(sp->nb + 1);
        if (term_start && sp->n_terms)
            DI_HIP(hipMemcpy(term_start, sp->term_start.p, (size_t)sp->n_terms * 8,
                             hipMemcpyDeviceToHost));
        if (blk_off && cells)
            DI_HIP(hipMemcpy(blk_off, sp->blk_off.p, cells * 4, hipMemcpyDeviceToHost));
        if (pdoc && sp->n_post)
            DI_HIP(hipMemcpy(pdoc, sp->pdoc.p, (size_t)sp->n_post * 2, hipMemcpyDeviceToHost));
        if (pimp && sp->n_post)
            DI_HIP(hipMemcpy(pimp, sp->pimp.p, (size_t)sp->n_post * 4, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
