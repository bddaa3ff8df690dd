// ib_sort.h -- the device passes the index builders share (index_build.hip,
// index_layout.hip): an exclusive scan of 32-bit counts into 64-bit offsets, and one pass
// of the stable least-significant-digit radix sort of 16-byte records with 8-bit digits
// (per tile a digit histogram, one scan over (digit, tile), a scatter whose places are
// sums of counts of the records that precede in input order: ballot ranks plus LDS
// counters, no atomic hands out a position).  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>

#include "di_common.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int IB_THREADS = 256, IB_WAVES = IB_THREADS / 64;
constexpr int IB_TILE = DI_INDEX_BUILD_TILE, IB_ROUNDS = IB_TILE / IB_THREADS;
constexpr int IB_MAX_GRID = 1 << 16;  // blocks of a grid-stride launch
constexpr int IB_SCAN_ITEMS = 8, IB_SCAN_CHUNK = IB_THREADS * IB_SCAN_ITEMS;
static_assert(IB_TILE % IB_THREADS == 0, "whole rounds");

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
    for (int w = 0; w < IB_WAVES; ++w) {
        if (w < wave_id()) before += wtot[w];
        all += wtot[w];
    }
    *total = all;
    return v + before;
}

// csum[c] = the sum of cnt[c * IB_SCAN_CHUNK, (c + 1) * IB_SCAN_CHUNK)
__global__ void __launch_bounds__(IB_THREADS)
ib_scan_sum_kernel(const uint32_t *__restrict__ cnt, int64_t len, int64_t *__restrict__ csum) {
    __shared__ int64_t wtot[IB_WAVES];
    const int64_t i0 = (int64_t)blockIdx.x * IB_SCAN_CHUNK + (int64_t)threadIdx.x * IB_SCAN_ITEMS;
    int64_t v = 0;
    for (int j = 0; j < IB_SCAN_ITEMS; ++j)
        if (i0 + j < len) v += cnt[i0 + j];
    int64_t total;
    block_incl_scan64(v, wtot, &total);
    if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

// One workgroup: csum[0, n_chunks) -> its exclusive scan in place, the total in csum[n_chunks].
__global__ void __launch_bounds__(IB_THREADS)
ib_scan_chunks_kernel(int64_t *__restrict__ csum, int64_t n_chunks) {
    __shared__ int64_t wtot[IB_WAVES];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += IB_THREADS) {
        const int64_t c = c0 + threadIdx.x;
        const int64_t v = c < n_chunks ? csum[c] : 0;
        int64_t total;
        const int64_t inc = block_incl_scan64(v, wtot, &total);
        if (c < n_chunks) csum[c] = carry + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) csum[n_chunks] = carry;
}

__global__ void __launch_bounds__(IB_THREADS)
ib_scan_apply_kernel(const uint32_t *__restrict__ cnt, int64_t len,
                     const int64_t *__restrict__ csum, int64_t *__restrict__ off) {
    __shared__ int64_t wtot[IB_WAVES];
    const int64_t i0 = (int64_t)blockIdx.x * IB_SCAN_CHUNK + (int64_t)threadIdx.x * IB_SCAN_ITEMS;
    uint32_t c[IB_SCAN_ITEMS];
    int64_t v = 0;
#pragma unroll
    for (int j = 0; j < IB_SCAN_ITEMS; ++j) {
        c[j] = i0 + j < len ? cnt[i0 + j] : 0u;
        v += c[j];
    }
    int64_t total;
    int64_t at = csum[blockIdx.x] + block_incl_scan64(v, wtot, &total) - v;
#pragma unroll
    for (int j = 0; j < IB_SCAN_ITEMS; ++j) {
        if (i0 + j < len) off[i0 + j] = at;
        at += c[j];
    }
}

// The digit of a record from bit `shift` on: of .y (on_y: the row of a kept posting, the
// first id of a pair record) or of .z (255 - val at shift 0; a pair record's second id).
__device__ __forceinline__ uint32_t ib_digit(const uint4 &r, bool on_y, int shift) {
    return ((on_y ? r.y : r.z) >> shift) & 255u;
}

__global__ void __launch_bounds__(IB_THREADS)
ib_hist_kernel(const uint4 *__restrict__ src, int64_t n, int64_t n_tiles, bool on_y, int shift,
               uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    static_assert(IB_THREADS == 256, "one thread a digit");
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        h[threadIdx.x] = 0;
        __syncthreads();
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i = tile * IB_TILE + (int64_t)r * IB_THREADS + threadIdx.x;
            if (i < n) atomicAdd(&h[ib_digit(src[i], on_y, shift)], 1u);  // (a count)
        }
        __syncthreads();
        hist[(int64_t)threadIdx.x * n_tiles + tile] = h[threadIdx.x];
        __syncthreads();  // h is free again
    }
}

__global__ void __launch_bounds__(IB_THREADS)
ib_scatter_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int64_t n,
                  int64_t n_tiles, bool on_y, int shift, const int64_t *__restrict__ off,
                  const int32_t *__restrict__ term_row, int64_t n_terms) {
    __shared__ int64_t run[256];                // where the next record of a digit goes
    __shared__ uint32_t wcnt[IB_WAVES][256];    // this round's records of a digit, per wave
    const int lane = lane_id(), wave = wave_id();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        run[threadIdx.x] = off[(int64_t)threadIdx.x * n_tiles + tile];
        for (int w = 0; w < IB_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
        __syncthreads();
        for (int r = 0; r < IB_ROUNDS; ++r) {
            const int64_t i0 = tile * IB_TILE + (int64_t)r * IB_THREADS;
            if (i0 >= n) break;  // (the same for the whole workgroup)
            const int64_t i = i0 + threadIdx.x;
            const bool valid = i < n;
            uint4 rec = make_uint4(0, 0, 0, 0);
            if (valid) rec = src[i];
            const uint32_t d = ib_digit(rec, on_y, shift);
            uint64_t same = __ballot(valid);  // the valid lanes of this wave with digit d
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const uint64_t m = __ballot(valid && ((d >> b) & 1u));
                same &= ((d >> b) & 1u) ? m : ~m;
            }
            const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
            if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
            __syncthreads();
            if (valid) {
                uint32_t before = 0;
                for (int w = 0; w < wave; ++w) before += wcnt[w][d];
                const int64_t pos = run[d] + before + rank;
                if (term_row) rec.y = rec.y < n_terms ? (uint32_t)term_row[rec.y] : 0u;
                if (pos >= 0 && pos < n) dst[pos] = rec;  // (always: the counts add up to n)
            }
            __syncthreads();
            uint32_t all = 0;
            for (int w = 0; w < IB_WAVES; ++w) {
                all += wcnt[w][threadIdx.x];
                wcnt[w][threadIdx.x] = 0;
            }
            run[threadIdx.x] += all;
            __syncthreads();
        }
        __syncthreads();  // run and wcnt are free again
    }
}

inline int grid_for(int64_t items, int per_block) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block,
                                                       IB_MAX_GRID));
}

inline size_t at_least_one(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

}  // namespace
}  // namespace di
