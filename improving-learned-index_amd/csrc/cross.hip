// cross.hip -- cross-encoder reranking on the DeeperImpact encoder: (passage, query)
// sequences assembled on the device from two token stores, scored by the existing
// forward with token 0 of every sequence as its only kept row, and ranked per query.
//
// Replaces, for a batch of (query, passage) pairs, the reference's
//   process_cross_encoder_documents_and_query   src/deep_impact/models/cross_encoder.py:39-51
//   DeepImpactCrossEncoder.forward              src/deep_impact/models/cross_encoder.py:9-23
//   sorted(zip(pids, scores), ...)              src/deep_impact/evaluation/cross_encoder_reranker.py:62
// The reference tokenizes f'{document} [SEP] {query}' once per pair; here every unique
// passage and query is tokenized once and only the pair indices reach the device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "di_common.h"
#include "enc_handle.h"
#include "topk_common.h"

namespace di {
namespace {

constexpr int SCAN_THREADS = 1024;  // 16 waves: one workgroup scans every pair
constexpr int COPY_THREADS = 256;   // one wave per sequence
constexpr int SORT_THREADS = 512;

constexpr int PK_BAD_INDEX = 1;  // a pair index outside its store (or offsets not monotone)
constexpr int PK_TOO_LONG = 2;   // 2^31 packed tokens or more

struct PairArgs {
    const int32_t *doc_tok;
    const int64_t *doc_off;
    const int32_t *qry_tok;
    const int64_t *qry_off;
    const int32_t *pair_doc;
    const int32_t *pair_qry;
    int32_t n_docs, n_q, n_pairs;
};

// Lengths + exclusive scan of every sequence, one workgroup walking the pairs in chunks of
// SCAN_THREADS with a running carry: cu[p + 1] = sum of len[0..p], len = n_prefix +
// min(|doc| + |qry|, budget) + n_suffix.  info = (n_tokens, max_len, PK_* bits).  With
// tt / cut: the kept rows of di_encode_pairs, token 0 of each sequence (tt[p] = 0,
// cut = 0..n_pairs).
__global__ __launch_bounds__(SCAN_THREADS) void pairs_scan_kernel(PairArgs a, int n_fixed,
                                                                  int budget,
                                                                  int32_t *__restrict__ cu,
                                                                  int32_t *__restrict__ tt,
                                                                  int32_t *__restrict__ cut,
                                                                  int64_t *__restrict__ info) {
    __shared__ uint32_t wsum[SCAN_THREADS / 64];
    __shared__ uint32_t wmax[SCAN_THREADS / 64];
    const int tid = threadIdx.x, wave = wave_id(), lane = lane_id();
    int64_t carry = 0;
    uint32_t mx = 0;
    int bad = 0;
    if (tid == 0) {
        cu[0] = 0;
        if (cut) cut[0] = 0;
    }
    for (int base = 0; base < a.n_pairs; base += SCAN_THREADS) {
        const int p = base + tid;
        uint32_t len = 0;
        if (p < a.n_pairs) {
            const int32_t d = a.pair_doc[p], q = a.pair_qry[p];
            if ((uint32_t)d >= (uint32_t)a.n_docs || (uint32_t)q >= (uint32_t)a.n_q) {
                bad = PK_BAD_INDEX;
            } else {
                const int64_t dl = a.doc_off[d + 1] - a.doc_off[d];
                const int64_t ql = a.qry_off[q + 1] - a.qry_off[q];
                if (dl < 0 || ql < 0)
                    bad = PK_BAD_INDEX;
                else
                    len = (uint32_t)n_fixed + (uint32_t)min(dl + ql, (int64_t)budget);
            }
        }
        const uint32_t inc = wave_prefix_sum(len);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            const uint32_t v = wsum[w];
            woff += w < wave ? v : 0u;
            tot += v;
        }
        if (p < a.n_pairs) {
            cu[p + 1] = (int32_t)(carry + woff + inc);
            if (tt) {
                tt[p] = 0;
                cut[p + 1] = p + 1;
            }
        }
        carry += tot;
        mx = max(mx, len);
        __syncthreads();  // wsum is rewritten by the next chunk
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    if (lane == 0) wmax[wave] = mx;
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        for (int w = 0; w < SCAN_THREADS / 64; ++w) mx = max(mx, wmax[w]);
        info[0] = carry;
        info[1] = mx;
        info[2] = bad | (carry >= (1ll << 31) ? PK_TOO_LONG : 0);
    }
}

// Sequence p = prefix ++ first (len - n_prefix - n_suffix) tokens of (doc ++ qry) ++ suffix,
// len from cu (pairs_scan_kernel).  One wave per sequence, lanes along its tokens.
__global__ __launch_bounds__(COPY_THREADS) void pairs_copy_kernel(PairArgs a, di_pair_format f,
                                                                  const int32_t *__restrict__ cu,
                                                                  int32_t *__restrict__ ids) {
    const int p = blockIdx.x * (COPY_THREADS / 64) + wave_id();
    if (p >= a.n_pairs) return;
    const int32_t d = a.pair_doc[p], q = a.pair_qry[p];
    if ((uint32_t)d >= (uint32_t)a.n_docs || (uint32_t)q >= (uint32_t)a.n_q) return;
    const int32_t o = cu[p], len = cu[p + 1] - o;
    const int content = len - f.n_prefix - f.n_suffix;
    const int64_t d0 = a.doc_off[d], dl = a.doc_off[d + 1] - d0, q0 = a.qry_off[q];
    for (int t = lane_id(); t < len; t += 64) {
        const int j = t - f.n_prefix;
        int32_t v;
        if (j < 0)
            v = f.prefix[t];
        else if (j >= content)
            v = f.suffix[j - content];
        else if (j < dl)
            v = a.doc_tok[d0 + j];
        else
            v = a.qry_tok[q0 + (j - dl)];
        ids[o + t] = v;
    }
}

// Positions of one segment's scores in the order of Python's
// sorted(zip(pids, scores), key=lambda x: x[1], reverse=True): score descending, equal
// scores (-0.0 == +0.0) in input order.  64-bit keys: order-preserving score bits |
// ~position; padding keys are 0 (below every real key).  One workgroup per segment.
__global__ __launch_bounds__(SORT_THREADS) void segment_order_kernel(
    const float *__restrict__ scores, const int32_t *__restrict__ cu_seg,
    int32_t *__restrict__ out_pos, int32_t *__restrict__ err) {
    __shared__ uint64_t keys[DI_MAX_TOPK];
    const int32_t o = cu_seg[blockIdx.x], n = cu_seg[blockIdx.x + 1] - o;
    if (n <= 0) {
        if (n < 0 && threadIdx.x == 0) err[0] = 1;
        return;
    }
    if (n > DI_MAX_TOPK) {
        for (int i = threadIdx.x; i < n; i += SORT_THREADS) out_pos[o + i] = -1;
        if (threadIdx.x == 0) err[1] = 1;
        return;
    }
    int n2 = 2;
    while (n2 < n) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += SORT_THREADS) {
        uint64_t k = 0;
        if (i < n) {
            uint32_t u = __float_as_uint(scores[o + i]);
            if ((u << 1) == 0) u = 0;  // -0.0 == +0.0 (on the bits: denormals stay apart)
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            k = ((uint64_t)u << 32) | (uint32_t)~(uint32_t)i;
        }
        keys[i] = k;
    }
    __syncthreads();
    bitonic_sort_desc<SORT_THREADS>(keys, n2);
    for (int i = threadIdx.x; i < n; i += SORT_THREADS)
        out_pos[o + i] = (int32_t)~(uint32_t)keys[i];
}

int check_format(const di_pair_format *f) {  // -> the content budget of a sequence
    DI_REQUIRE(f, DI_EINVAL, "null format");
    DI_REQUIRE(f->n_prefix >= 0 && f->n_prefix <= DI_MAX_PAIR_SPECIALS && f->n_suffix >= 0 &&
                   f->n_suffix <= DI_MAX_PAIR_SPECIALS,
               DI_EINVAL, "at most %d prefix and %d suffix ids", DI_MAX_PAIR_SPECIALS,
               DI_MAX_PAIR_SPECIALS);
    DI_REQUIRE(f->max_length >= f->n_prefix + f->n_suffix && f->max_length <= (1 << 16),
               DI_EINVAL, "max_length %d: at least the %d special tokens, at most 65536",
               f->max_length, f->n_prefix + f->n_suffix);
    return f->max_length - f->n_prefix - f->n_suffix;
}

// The two token stores and the pair indices on the device (staged when they are host arrays).
struct StagedPairs {
    DevBuf dt, dof, qt, qof, pd, pq;
    PairArgs a{};
    void stage(const int32_t *doc_tok, const int64_t *doc_off, int32_t n_docs,
               const int32_t *qry_tok, const int64_t *qry_off, int32_t n_q,
               const int32_t *pair_doc, const int32_t *pair_qry, int32_t n_pairs, bool dev,
               hipStream_t s) {
        DI_REQUIRE(doc_off && qry_off && n_docs >= 0 && n_q >= 0 && n_pairs >= 0 &&
                       (n_pairs == 0 || (pair_doc && pair_qry)),
                   DI_EINVAL, "bad argument");
        size_t nd = 0, nq = 0;
        if (!dev) {
            DI_REQUIRE(doc_off[0] == 0 && qry_off[0] == 0 && doc_off[n_docs] >= 0 &&
                           qry_off[n_q] >= 0,
                       DI_EINVAL, "token store offsets must start at 0");
            nd = (size_t)doc_off[n_docs];
            nq = (size_t)qry_off[n_q];
            DI_REQUIRE((nd == 0 || doc_tok) && (nq == 0 || qry_tok), DI_EINVAL,
                       "null token store");
        }
        a.doc_tok = stage_in(doc_tok, nd, dev, dt, s);
        a.doc_off = stage_in(doc_off, (size_t)n_docs + 1, dev, dof, s);
        a.qry_tok = stage_in(qry_tok, nq, dev, qt, s);
        a.qry_off = stage_in(qry_off, (size_t)n_q + 1, dev, qof, s);
        a.pair_doc = stage_in(pair_doc, (size_t)n_pairs, dev, pd, s);
        a.pair_qry = stage_in(pair_qry, (size_t)n_pairs, dev, pq, s);
        a.n_docs = n_docs;
        a.n_q = n_q;
        a.n_pairs = n_pairs;
    }
};

void launch_scan(const PairArgs &a, const di_pair_format &f, int budget, int32_t *d_cu,
                 int32_t *d_tt, int32_t *d_cut, int64_t *d_info, hipStream_t s) {
    hipLaunchKernelGGL(pairs_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a,
                       f.n_prefix + f.n_suffix, budget, d_cu, d_tt, d_cut, d_info);
    check_launch("pairs_scan");
}

// The size read-back: the one synchronisation of a pack.
void read_info(const int64_t *d_info, hipStream_t s, int64_t *n_tokens, int32_t *max_len) {
    int64_t info[3] = {0, 0, 0};
    read_back(info, d_info, s);
    DI_REQUIRE(!(info[2] & PK_BAD_INDEX), DI_EINVAL,
               "a pair index is outside its token store (or the store's offsets decrease)");
    DI_REQUIRE(!(info[2] & PK_TOO_LONG), DI_ERANGE, "the packed batch has %lld tokens >= 2^31",
               (long long)info[0]);
    *n_tokens = info[0];
    *max_len = (int32_t)info[1];
}

void launch_copy(const PairArgs &a, const di_pair_format &f, const int32_t *d_cu, int32_t *d_ids,
                 hipStream_t s) {
    if (a.n_pairs == 0) return;
    const int per = COPY_THREADS / 64;
    hipLaunchKernelGGL(pairs_copy_kernel, dim3((a.n_pairs + per - 1) / per), dim3(COPY_THREADS),
                       0, s, a, f, d_cu, d_ids);
    check_launch("pairs_copy");
}

}  // namespace
}  // namespace di

using namespace di;

extern "C" {

int di_pairs_pack(const int32_t *doc_tok, const int64_t *doc_off, int32_t n_docs,
                  const int32_t *qry_tok, const int64_t *qry_off, int32_t n_q,
                  const int32_t *pair_doc, const int32_t *pair_qry, int32_t n_pairs,
                  const di_pair_format *fmt, int32_t *tok_ids, int64_t tok_cap,
                  int32_t *cu_seqlens, int64_t *n_tokens, int32_t *max_len, int device,
                  void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(cu_seqlens && n_tokens && max_len && tok_cap >= 0 && (tok_cap == 0 || tok_ids),
                   DI_EINVAL, "bad argument");
        const int budget = check_format(fmt);
        check_device(device);
        DeviceScope ds(device);
        const bool dev = flags & DI_F_DEVICE_PTRS;
        hipStream_t s = (hipStream_t)hip_stream;
        StagedPairs sp;
        sp.stage(doc_tok, doc_off, n_docs, qry_tok, qry_off, n_q, pair_doc, pair_qry, n_pairs,
                 dev, s);
        DevBuf info, b_cu, b_ids;
        info.reserve(24);
        StagedOut<int32_t> cu(cu_seqlens, (size_t)n_pairs + 1, dev, b_cu), ids(tok_ids, dev, b_ids);
        launch_scan(sp.a, *fmt, budget, cu.d, nullptr, nullptr, info.as<int64_t>(), s);
        read_info(info.as<int64_t>(), s, n_tokens, max_len);
        DI_REQUIRE(*n_tokens <= tok_cap, DI_ERANGE, "tok_ids holds %lld tokens, %lld needed",
                   (long long)tok_cap, (long long)*n_tokens);
        launch_copy(sp.a, *fmt, cu.d, ids.size((size_t)*n_tokens), s);
        cu.copy_back(s);
        ids.copy_back(s);
        // (host pointers, or staged temporaries that die with this call: wait)
        if (!dev || !(flags & DI_F_ASYNC)) DI_HIP(hipStreamSynchronize(s));
    });
}

int di_encode_pairs(di_encoder *e, const int32_t *doc_tok, const int64_t *doc_off, int32_t n_docs,
                    const int32_t *qry_tok, const int64_t *qry_off, int32_t n_q,
                    const int32_t *pair_doc, const int32_t *pair_qry, int32_t n_pairs,
                    const di_pair_format *fmt, float *out_scores, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(e && (n_pairs == 0 || out_scores), DI_EINVAL, "bad argument");
        DI_REQUIRE(!(flags & (DI_F_TOKEN_IMPACTS | DI_F_ROUND3)), DI_EINVAL,
                   "di_encode_pairs takes DI_F_DEVICE_PTRS, DI_F_ASYNC and DI_F_TIMING");
        const int budget = check_format(fmt);
        DI_REQUIRE(fmt->max_length <= e->cfg.max_positions, DI_ERANGE,
                   "max_length %d > max_positions %d", fmt->max_length, e->cfg.max_positions);
        DeviceScope ds(e->device);
        const bool dev = flags & DI_F_DEVICE_PTRS;
        const bool timing = flags & DI_F_TIMING;
        hipStream_t s = e->stream;
        StagedPairs sp;
        sp.stage(doc_tok, doc_off, n_docs, qry_tok, qry_off, n_q, pair_doc, pair_qry, n_pairs,
                 dev, s);
        if (n_pairs == 0) {
            DI_HIP(hipStreamSynchronize(s));
            return;
        }
        // sequence offsets and kept rows into the encoder's own staging buffers, where
        // di_encode reads them as device arrays
        ensure_workspace(e, 0, n_pairs, n_pairs);
        e->pinfo.reserve(24);
        int64_t n_tokens = 0;
        int32_t max_len = 0;
        {
            TimedLaunch tl(e->timer, timing, "pairs_scan", s);
            launch_scan(sp.a, *fmt, budget, e->cu.as<int32_t>(), e->tt.as<int32_t>(),
                        e->cut.as<int32_t>(), e->pinfo.as<int64_t>(), s);
        }
        read_info(e->pinfo.as<int64_t>(), s, &n_tokens, &max_len);
        ensure_workspace(e, n_tokens, n_pairs, n_pairs);
        {
            TimedLaunch tl(e->timer, timing, "pairs_copy", s);
            launch_copy(sp.a, *fmt, e->cu.as<int32_t>(), e->ids.as<int32_t>(), s);
        }
        DevBuf tmp;
        StagedOut<float> out(out_scores, (size_t)n_pairs, dev, tmp);
        // the staged stores are temporaries of this call: a host-pointer call waits
        const uint32_t f2 = DI_F_DEVICE_PTRS | (timing ? DI_F_TIMING : 0u) |
                            (dev && (flags & DI_F_ASYNC) ? DI_F_ASYNC : 0u);
        const int rc = di_encode(e, e->ids.as<int32_t>(), e->cu.as<int32_t>(), n_pairs, n_tokens,
                                 max_len, e->tt.as<int32_t>(), e->cut.as<int32_t>(), n_pairs,
                                 out.d, f2);
        if (rc != DI_OK) throw Error{rc};  // (di_last_error holds di_encode's message)
        out.copy_back(s);
        if (!dev) DI_HIP(hipStreamSynchronize(s));
    });
}

int di_segment_order(const float *scores, const int32_t *cu_seg, int32_t n_seg, int32_t *out_pos,
                     int device, void *hip_stream, uint32_t flags) {
    return guard([&] {
        DI_REQUIRE(cu_seg && n_seg >= 0, DI_EINVAL, "bad argument");
        check_device(device);
        DeviceScope ds(device);
        const bool dev = flags & DI_F_DEVICE_PTRS;
        hipStream_t s = (hipStream_t)hip_stream;
        if (n_seg == 0) return;
        int64_t n = 0;
        if (!dev) {
            n = check_cu(cu_seg, n_seg, "cu_seg", DI_MAX_TOPK);
            if (n == 0) return;
        }
        DI_REQUIRE(scores && out_pos, DI_EINVAL, "null argument");
        DevBuf sc, cu, b_pos, err;
        err.reserve(8);
        DI_HIP(hipMemsetAsync(err.p, 0, 8, s));
        const float *d_sc = stage_in(scores, (size_t)n, dev, sc, s);
        const int32_t *d_cu = stage_in(cu_seg, (size_t)n_seg + 1, dev, cu, s);
        StagedOut<int32_t> pos(out_pos, (size_t)n, dev, b_pos);
        hipLaunchKernelGGL(segment_order_kernel, dim3(n_seg), dim3(SORT_THREADS), 0, s, d_sc,
                           d_cu, pos.d, err.as<int32_t>());
        check_launch("segment_order");
        pos.copy_back(s);
        // (the error words are a temporary of this call: it always waits for them)
        int32_t h[2] = {0, 0};
        read_back(h, err.p, s);
        DI_REQUIRE(!h[0], DI_EINVAL, "cu_seg is not monotone");
        DI_REQUIRE(!h[1], DI_ERANGE, "a segment has more than %d scores", DI_MAX_TOPK);
    });
}

}  // extern "C"
