// enc_attn_v3.hip -- the persistent, double-buffered bf16 attention (attention_v3_kernel:
// documents of up to 512 tokens, head dim 64), gfx950.  What it computes: enc_attn.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "di_common.h"
#include "enc_attn.h"
#include "enc_launch.h"

namespace di {

// One 32-key step of the online softmax for 16 queries (lane holds 8 raw scores of
// its query), in three parts so that attention_v3_kernel's key loop can test every
// query tile of a step with one branch and keep the common path of both tiles in one
// basic block.  Lazy rescale: the reference max m only moves when a score exceeds it
// by THR (2^8 in p) -- one compare per score and one ballot in the common case; the
// full max / rescale path runs on the first chunk and rarely after.
// p = exp2(s * sc - m * sc) by the raw v_exp_f32 (inputs <= 8; underflow to 0 is
// what softmax wants).
// lim = m + 8 / sc (kept by the caller, moved only with m)
__device__ __forceinline__ bool softmax_need(const f32x4 (&s)[2], float lim) {
    bool need = false;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) need |= s[t][r] > lim;
    return need;
}
__device__ __forceinline__ void softmax_rescale(const f32x4 (&s)[2], float lim, float &m,
                                                float &msc, f32x4 (&o)[4], f32x4 &l) {
    constexpr float sc = ATT_SC;
    const float cmax =
        lane_group_max(fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                             fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3]))));
    // per query: only a row with a score of its own above its limit moves its reference
    // (alpha = 1 exactly for the others), so that a row's arithmetic does not depend on
    // which queries share its tile -- the pruned last layer regroups them
    const float m_new = cmax > lim ? fmaxf(m, cmax) : m;
    const float alpha = exp2f((m - m_new) * sc);  // 0 on the first chunk
    m = m_new;
    msc = m_new * sc;
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
}
__device__ __forceinline__ void softmax_p(const f32x4 (&s)[2], float msc, bf16x8 &pb) {
    constexpr float sc = ATT_SC;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pb[r] = (bf16)__builtin_amdgcn_exp2f(fmaf(s[0][r], sc, -msc));
        pb[4 + r] = (bf16)__builtin_amdgcn_exp2f(fmaf(s[1][r], sc, -msc));
    }
}

// ---------------------------------------------------------------------------
// Persistent, double-buffered form (bf16, max_len <= 320): the QKV projection is
// written row-major [M][3H] (Q | K | V, no V^T scatter), and one 512-thread
// workgroup per CU walks the (doc, head) pairs.  For each pair the K and V rows
// (128 B per key and head) are copied into LDS by LDS-DMA (global_load_lds,
// 16-byte XOR swizzle on the source), the NEXT pair's copy is issued before the
// current pair is computed, so the copy latency hides behind the MFMA/softmax
// work (the compute loop issues no global loads: Q fragments are loaded before
// the prefetch is issued).
//   K image: row r = 128 B, chunk q at slot q ^ (r & 7); S^T fragment row c of
//            tile t = key 8(c>>2) + 4t + (c&3) (lane group g then holds the
//            consecutive keys 8g..8g+7 of P^T).
//   V image: same row format; the O^T A operand (V^T rows) is read with
//            ds_read_b64_tr_b16: per 16-lane group, lane 4q+p addresses key row
//            q of a 4-row block, columns 4p..4p+3; lane i receives column i.
// Eight waves, 32 queries (two 16-query tiles) per wave-block, blocks round robin.
// DB = true : two buffers of 320 K + 320 V rows (80 KiB each, 160 KiB: the whole
//             CU), next pair prefetched during the current one; n <= 320.
// DB = false: one buffer of 512 + 512 rows (128 KiB), no prefetch; n <= 512.
constexpr int ATT3_WAVES = 8;
template <bool DB>
struct Att3 {
    static constexpr int ROWS = DB ? 320 : 512;  // K and V image rows each
    static constexpr int BUF = 2 * ROWS * 128;
    static constexpr int LDS = DB ? 2 * BUF : BUF;
};

// K / V image swizzle: the 16-byte slot j of key row r is stored at slot
// j ^ att3_swz(r).  Bit 2 folds in row bit 3 so that the fragment reads are
// conflict-free: a ds_read_b128 lane group (16 lanes, rows 8 (c >> 2) + (c & 3) + 4 t
// of two lane groups g) and a ds_read_b64_tr_b16 lane group (32 lanes, rows
// 8 g + 4 h2 + q of two g) each see every bank once.  Bits 0-4 of a fragment row
// never depend on the 32-key chunk, so per lane every read address is a per-pair base
// plus key0 * 128 plus an immediate (see kb / vb below).
__device__ __forceinline__ int att3_swz(int r) { return (r & 7) ^ ((r >> 1) & 4); }

// f(integral_constant<K>) for K = K0, K0 + 1, .. < N until f returns true
template <int K, int N, class F>
__device__ __forceinline__ void att3_chunks(F &f) {
    if constexpr (K < N) {
        if (f(std::integral_constant<int, K>{})) return;
        att3_chunks<K + 1, N>(f);
    }
}

// The key loop is instantiated per tile count (1 or 2) and runs both tiles' S^T
// products, one shared rescale test (a branch only into the rare path) and both
// tiles' exp / O^T products as one basic block, so that one tile's softmax VALU
// overlaps the other tile's MFMAs (-2.5% attention time against a per-tile loop,
// bit-identical).
template <bool DB>
__global__ void __launch_bounds__(64 * ATT3_WAVES, 1)
attention_v3_kernel(const bf16 *__restrict__ qkv, const int32_t *__restrict__ cu_seqlens, int H,
                    int n_heads, int n_pairs, bf16 *__restrict__ ctx,
                    const int32_t *__restrict__ qsel, const int32_t *__restrict__ cu_qsel) {
    // qsel (optional): only the query rows qsel[cu_qsel[d] ..) (doc-local token
    // indices) of document d are computed, into ctx rows cu_qsel[d] + i (the encoder's
    // last layer: only the rows the term gather reads); keys are always every token.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    typedef __attribute__((address_space(3))) void lds_void;
    constexpr int QTB = 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
    const int ld = 3 * H;
    const uint32_t lds_base =
        (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char *)lds);

    // pair -> (doc, head): p / n_heads by a multiply-high (exact for p < 2^32 / n_heads);
    // one head: the magic number would be 2^32, the pair is the document
    const uint32_t heads_magic = 0xFFFFFFFFu / (uint32_t)n_heads + 1u;
    auto doc_of = [&](int pp) {
        return n_heads == 1 ? pp : (int)__umulhi((uint32_t)pp, heads_magic);
    };

    // LDS-DMA of pair p's K and V rows < round32(n) into buffer b, through a buffer
    // resource spanning the document's rows only: rows past n read zeros (their scores
    // are masked, their probabilities 0).  Slot j of row r lands at j ^ att3_swz(r); a
    // wave's pieces are all of one parity (pieces wave, wave + 8, ..; n8 is even), so
    // the swizzle is a per-lane constant: r_in ^ ((wave & 1) << 2).
    auto stage = [&](int p, int b) {
        const int doc = doc_of(p), h = p - doc * n_heads;
        const int tok0 = cu_seqlens[doc], n = cu_seqlens[doc + 1] - tok0;
        const int n8 = ((n + 31) & ~31) >> 3;  // 8-row pieces of K, and of V
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
            (void *)(qkv + (int64_t)tok0 * ld), (short)0, n * ld * 2, 0x00020000);
        const int r_in = lane >> 3;  // row within a piece
        const uint32_t voff = r_in * ld * 2 + (H + h * ATT_D) * 2 +
                              (((lane & 7) ^ r_in ^ ((wave & 1) << 2)) << 4);
        unsigned char *buf = lds + b * Att3<DB>::BUF;
        for (int pc = wave; pc < 2 * n8; pc += ATT3_WAVES) {
            const bool is_k = pc < n8;
            const int piece = is_k ? pc : pc - n8;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsrc, (lds_void *)(buf + (is_k ? 0 : Att3<DB>::ROWS * 128) + piece * 1024), 16,
                voff + piece * 8 * ld * 2 + (is_k ? 0 : H * 2), 0, 0, 0);
        }
    };

    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16)1.0f;
    // Per-lane fragment offsets within an image (key0 = 0; see att3_swz).
    // K, S^T tile t, head-dim chunk ch: row krel + 4 t, slot 4 ch + g, stored at
    // (g ^ (c & 3)) | ((ch ^ t ^ b3) << 2)  ->  koff[ch ^ t] + 512 t.
    uint32_t koff[2];
    {
        const int krel = 8 * (c >> 2) + (c & 3), b3 = (c >> 2) & 1;
#pragma unroll
        for (int x = 0; x < 2; ++x) koff[x] = krel * 128 + ((g ^ (c & 3)) << 4) + ((x ^ b3) << 6);
    }
    // V^T by ds_read_b64_tr_b16, lane 4 q + p of a 16-lane group: row 8 g + 4 h2 + q,
    // columns 16 dt + 4 p..+3 = slot 2 dt + (p >> 1), half p & 1, stored at slot
    // u0 | ((u1 ^ dt0) << 1) | ((dt1 ^ h2 ^ g0) << 2) with u = (p >> 1) ^ q
    //   ->  voff[dt & 1][(dt >> 1) ^ h2] + 512 h2.
    uint32_t voff[2][2];
    {
        const int tq = c >> 2, tp = c & 3, u = (tp >> 1) ^ tq;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb)
                voff[a][bb] = (8 * g + tq) * 128 + 8 * (tp & 1) +
                              16 * ((u & 1) | (((u >> 1) ^ a) << 1) | ((bb ^ (g & 1)) << 2));
    }

    // Q of pair p comes one pair ahead (inline-asm global loads: the compiler sees no
    // pending load, so it neither waits nor drains the K/V prefetch for them), into the
    // register set not in use; the wait at the top of the pair retires it.  The two
    // sets are used in turn (the loop is unrolled by two: no register copies).
    // Query tiles (16 queries) of a document are dealt to the 8 waves in contiguous
    // runs whose lengths differ by at most one (wave w: tiles [t_first, t_first + t_cnt));
    // a wave takes its run two tiles at a time (K / V fragments shared) and an odd last
    // tile alone, so a pair costs ceil(tiles / 8) tile-steps instead of whole 32-query
    // blocks dealt round robin.
    auto tiles_of = [&](int nn, int &t_first, int &t_cnt) {
        const int n_t = (nn + 15) >> 4, base = n_t / ATT3_WAVES, extra = n_t % ATT3_WAVES;
        t_cnt = base + (wave < extra ? 1 : 0);
        t_first = wave * base + min(wave, extra);
    };
    // Q row addresses of pair pp for this wave's tile group i (tiles t_first + 2 i,
    // + 2 i + 1): [qt][ch]
    auto q_srcs = [&](int pp, int i, const bf16 *(&src)[QTB][2]) {
        const int dd = doc_of(pp), hh = pp - dd * n_heads;
        const int t0 = cu_seqlens[dd], nn = cu_seqlens[dd + 1] - t0;
        const int qs0 = qsel ? cu_qsel[dd] : 0, nq = qsel ? cu_qsel[dd + 1] - qs0 : nn;
        int t_first, t_cnt;
        tiles_of(nq, t_first, t_cnt);
        const int q_base = (t_first + 2 * i) * 16;
#pragma unroll
        for (int qt = 0; qt < QTB; ++qt) {
            const int qi = max(min(q_base + 16 * qt + c, nq - 1), 0);
            const int qloc = qsel ? (nq > 0 ? min(max(qsel[qs0 + qi], 0), max(nn - 1, 0)) : 0)
                                  : qi;
            const int qrow = t0 + qloc;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch)
                src[qt][ch] = qkv + (int64_t)qrow * ld + hh * ATT_D + ch * 32 + 8 * g;
        }
    };
    // DB: tile group 0 of the next pair, one pair ahead
    auto load_q = [&](int pp, uint4 (&qd)[QTB][2]) {
        const bf16 *src[QTB][2];
        q_srcs(pp, 0, src);
#pragma unroll
        for (int qt = 0; qt < QTB; ++qt)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch)
                asm volatile("global_load_dwordx4 %0, %1, off"
                             : "=v"(qd[qt][ch])
                             : "v"(src[qt][ch])
                             : "memory");
    };
    // tile group i of pair pp now, loaded together with the wait for them (one asm
    // statement: the outputs exist only after the wait, so no copy of a register
    // still being loaded can be scheduled above it).  The wait also retires any K / V
    // staging in flight (!DB: this pair's; DB, group 1: the next pair's, by then
    // mostly landed).
    auto load_q_wait = [&](int pp, int i, uint4 (&qd)[QTB][2]) {
        static_assert(QTB == 2, "load_q_wait: 4 loads");
        const bf16 *src[QTB][2];
        q_srcs(pp, i, src);
        asm volatile(
            "global_load_dwordx4 %0, %4, off\n\t"
            "global_load_dwordx4 %1, %5, off\n\t"
            "global_load_dwordx4 %2, %6, off\n\t"
            "global_load_dwordx4 %3, %7, off\n\t"
            "s_waitcnt vmcnt(0)"
            : "=&v"(qd[0][0]), "=&v"(qd[0][1]), "=&v"(qd[1][0]), "=&v"(qd[1][1])
            : "v"(src[0][0]), "v"(src[0][1]), "v"(src[1][0]), "v"(src[1][1])
            : "memory");
    };
    // qn: tile group 0 of pair p (DB: loaded one pair ahead, in flight); qc: the copy
    // the key loops read, made after the wait (so qn can take the next pair's loads)
    auto run_pair = [&](int p, int b, uint4 (&qc)[QTB][2], uint4 (&qn)[QTB][2])
                        __attribute__((always_inline)) {
        if (!DB) {
            stage(p, 0);
            load_q_wait(p, 0, qn);  // (also retires the staging)
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // K/V and Q of this pair
#pragma unroll
        for (int qt = 0; qt < QTB; ++qt)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {  // the loaded values exist from here on
                asm volatile("" : "+v"(qn[qt][ch].x), "+v"(qn[qt][ch].y), "+v"(qn[qt][ch].z),
                             "+v"(qn[qt][ch].w));
                qc[qt][ch] = qn[qt][ch];
            }
        __syncthreads();
        const int doc = doc_of(p), h = p - doc * n_heads;
        const int tok0 = cu_seqlens[doc], n = cu_seqlens[doc + 1] - tok0;
        const int qs0 = qsel ? cu_qsel[doc] : 0, nq = qsel ? cu_qsel[doc + 1] - qs0 : n;
        const int out0 = qsel ? qs0 : tok0;  // ctx row of query 0
        int t_first, t_cnt;
        tiles_of(nq, t_first, t_cnt);
        if (DB && p + (int)gridDim.x < n_pairs) {
            load_q(p + gridDim.x, qn);
            stage(p + gridDim.x, b ^ 1);
        }

        const uint32_t kim = lds_base + b * Att3<DB>::BUF;
        const uint32_t vim = kim + Att3<DB>::ROWS * 128;
        // Per-pair fragment bases (opaque to the compiler, so that it keeps one set
        // live instead of precomputing every buffer / chunk combination).
        uint32_t kb[2], vb[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            kb[x] = kim + koff[x];
            asm volatile("" : "+v"(kb[x]));
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                vb[a][bb] = vim + voff[a][bb];
                asm volatile("" : "+v"(vb[a][bb]));
            }
        // Fragment reads of the 32-key chunk at key0 + SUB: key0 (a multiple of 64, one
        // address add per two chunks) in the address, SUB (compile time) and the row
        // parts in the instruction's immediate.  Inline asm: the compiler must not drain
        // the next pair's LDS-DMA with vmcnt(0) before them.  Issue and wait are
        // separate statements; the wait names every register still being written
        // ("+v"), so nothing touches one earlier (tools/asm_wait_scan.py checks the
        // assembly).
        using C0 = std::integral_constant<int, 0>;
        using C32 = std::integral_constant<int, 32>;
        auto read_k = [&](int key0, auto sub_c, bf16x8 (&kf)[2][2]) {  // [t][ch]
            constexpr int OFF = decltype(sub_c)::value * 128;
            const uint32_t k0 = kb[0] + key0 * 128, k1 = kb[1] + key0 * 128;
            asm volatile(
                "ds_read_b128 %0, %4 offset:%6\n\t"
                "ds_read_b128 %1, %5 offset:%6\n\t"
                "ds_read_b128 %2, %5 offset:%7\n\t"
                "ds_read_b128 %3, %4 offset:%7"
                : "=&v"(kf[0][0]), "=&v"(kf[0][1]), "=&v"(kf[1][0]), "=&v"(kf[1][1])
                : "v"(k0), "v"(k1), "i"(OFF), "i"(OFF + 512)
                : "memory");
        };
        auto read_v = [&](int key0, auto sub_c, uint2 (&hv)[4][2]) {  // [dt][h2]
            constexpr int OFF = decltype(sub_c)::value * 128;
            const uint32_t v00 = vb[0][0] + key0 * 128, v01 = vb[0][1] + key0 * 128,
                           v10 = vb[1][0] + key0 * 128, v11 = vb[1][1] + key0 * 128;
            asm volatile(
                "ds_read_b64_tr_b16 %0, %8 offset:%12\n\t"
                "ds_read_b64_tr_b16 %1, %9 offset:%13\n\t"
                "ds_read_b64_tr_b16 %2, %10 offset:%12\n\t"
                "ds_read_b64_tr_b16 %3, %11 offset:%13\n\t"
                "ds_read_b64_tr_b16 %4, %9 offset:%12\n\t"
                "ds_read_b64_tr_b16 %5, %8 offset:%13\n\t"
                "ds_read_b64_tr_b16 %6, %11 offset:%12\n\t"
                "ds_read_b64_tr_b16 %7, %10 offset:%13"
                : "=&v"(hv[0][0]), "=&v"(hv[0][1]), "=&v"(hv[1][0]), "=&v"(hv[1][1]),
                  "=&v"(hv[2][0]), "=&v"(hv[2][1]), "=&v"(hv[3][0]), "=&v"(hv[3][1])
                : "v"(v00), "v"(v01), "v"(v10), "v"(v11), "i"(OFF), "i"(OFF + 512)
                : "memory");
        };
        // counted waits naming the registers they retire ("+v"): LDS reads complete in
        // issue order, so lgkmcnt(N) retires all but the newest N
        auto wait_k = [&](bf16x8 (&kf)[2][2]) {  // K in flight, then the 8 V reads
            asm volatile("s_waitcnt lgkmcnt(8)"
                         : "+v"(kf[0][0]), "+v"(kf[0][1]), "+v"(kf[1][0]), "+v"(kf[1][1])
                         :
                         : "memory");
        };
        auto wait_v = [&](uint2 (&hv)[4][2], int) {  // V, then the 4 K reads
            asm volatile("s_waitcnt lgkmcnt(4)"
                         : "+v"(hv[0][0]), "+v"(hv[0][1]), "+v"(hv[1][0]), "+v"(hv[1][1]),
                           "+v"(hv[2][0]), "+v"(hv[2][1]), "+v"(hv[3][0]), "+v"(hv[3][1])
                         :
                         : "memory");
        };
        auto wait_all = [&](bf16x8 (&kf)[2][2], uint2 (&hv)[4][2]) {
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(kf[0][0]), "+v"(kf[0][1]), "+v"(kf[1][0]), "+v"(kf[1][1]),
                           "+v"(hv[0][0]), "+v"(hv[0][1]), "+v"(hv[1][0]), "+v"(hv[1][1]),
                           "+v"(hv[2][0]), "+v"(hv[2][1]), "+v"(hv[3][0]), "+v"(hv[3][1])
                         :
                         : "memory");
        };
        // merged key loop over NQ (1 or 2) query tiles starting at q_base, software
        // pipelined one chunk deep: step k issues S^T(k + 1) = K(k + 1) Q^T on the
        // matrix pipe, then computes P(k) (VALU) beside it, then O^T += V^T(k) P^T(k);
        // the LDS reads of K(k + 2) and V(k + 1) are in flight meanwhile.  Every
        // product and every f32 operation is the one of the unpipelined loop, in the
        // same order (bit-identical).
        auto key_loop = [&](auto nq_c, const uint4 (&qf)[QTB][2], int q_base)
                            __attribute__((always_inline)) {
            constexpr int NQ = decltype(nq_c)::value;
            float m[NQ], msc[NQ], lim[NQ];
            f32x4 o[NQ][4], l[NQ];
#pragma unroll
            for (int qt = 0; qt < NQ; ++qt) {
                m[qt] = -INFINITY;
                msc[qt] = -INFINITY;
                lim[qt] = -INFINITY;
                l[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            bf16x8 qv[NQ][2];  // B operands Q^T
#pragma unroll
            for (int qt = 0; qt < NQ; ++qt)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) __builtin_memcpy(&qv[qt][ch], &qf[qt][ch], 16);
            auto qk = [&](const bf16x8 (&kf)[2][2], f32x4 (&s)[NQ][2]) {
#pragma unroll
                for (int qt = 0; qt < NQ; ++qt)
#pragma unroll
                    for (int t = 0; t < 2; ++t) s[qt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ch = 0; ch < 2; ++ch)  // independent chains adjacent
#pragma unroll
                    for (int qt = 0; qt < NQ; ++qt)
#pragma unroll
                        for (int t = 0; t < 2; ++t)
                            s[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[t][ch], qv[qt][ch], s[qt][t], 0, 0, 0);
            };
            auto rescale = [&](f32x4 (&s)[NQ][2]) {
                bool need[NQ], need_any = false;
#pragma unroll
                for (int qt = 0; qt < NQ; ++qt) {
                    need[qt] = softmax_need(s[qt], lim[qt]);
                    need_any |= need[qt];
                }
                if (__any(need_any)) {  // rare after the first chunk
#pragma unroll
                    for (int qt = 0; qt < NQ; ++qt)
                        if (__any(need[qt])) {
                            softmax_rescale(s[qt], lim[qt], m[qt], msc[qt], o[qt], l[qt]);
                            lim[qt] = m[qt] + 8.0f / ATT_SC;
                        }
                }
            };
            auto pv = [&](const f32x4 (&s)[NQ][2], const uint2 (&hv)[4][2]) {
                bf16x8 pb[NQ];
#pragma unroll
                for (int qt = 0; qt < NQ; ++qt) softmax_p(s[qt], msc[qt], pb[qt]);
                bf16x8 vf[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const uint4 v4 = make_uint4(hv[dt][0].x, hv[dt][0].y, hv[dt][1].x, hv[dt][1].y);
                    __builtin_memcpy(&vf[dt], &v4, 16);
                }
#pragma unroll
                for (int qt = 0; qt < NQ; ++qt) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt)
                        o[qt][dt] =
                            __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[dt], pb[qt], o[qt][dt], 0, 0, 0);
                    l[qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pb[qt], l[qt], 0, 0, 0);
                }
            };
            // step at chunk key0 + SUB (not the last chunk): s = S^T(chunk) issued,
            // kn = K(chunk + 32) in flight, reloaded in place with K(chunk + 64) once the
            // S^T products have read it (MFMA A operands are read at issue; one chunk
            // past the end reads stale rows of the image, never used); sn receives
            // S^T(chunk + 32).  V(chunk) is read inside the step (its latency hides
            // behind the S^T products and the softmax).
            auto step = [&](int key0, auto sub_c, f32x4 (&s)[NQ][2], f32x4 (&sn)[NQ][2],
                            bf16x8 (&kn)[2][2]) {
                rescale(s);
                uint2 hv[4][2];
                read_v(key0, sub_c, hv);
                wait_k(kn);
                qk(kn, sn);
                read_k(key0, std::integral_constant<int, decltype(sub_c)::value + 64>{}, kn);
                wait_v(hv, 0);
                pv(s, hv);
            };
            // the last chunk: masked keys; kn (K one chunk past the end) is named by
            // the wait
            auto last = [&](int key0, auto sub_c, f32x4 (&s)[NQ][2], bf16x8 (&kn)[2][2]) {
                const int kc = key0 + decltype(sub_c)::value;
                if (kc + 32 > n) {
#pragma unroll
                    for (int qt = 0; qt < NQ; ++qt)
#pragma unroll
                        for (int t = 0; t < 2; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (kc + 8 * g + 4 * t + r >= n) s[qt][t][r] = -INFINITY;
                }
                rescale(s);
                uint2 hv[4][2];
                read_v(key0, sub_c, hv);
                wait_all(kn, hv);
                pv(s, hv);
            };
            bf16x8 kf[2][2];
            f32x4 sa[NQ][2], sb[NQ][2];
            read_k(0, C0{}, kf);
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(kf[0][0]), "+v"(kf[0][1]), "+v"(kf[1][0]), "+v"(kf[1][1])
                         :
                         : "memory");
            qk(kf, sa);
            read_k(0, C32{}, kf);
            // two steps per iteration: S^T alternates between sa and sb without copies,
            // and the second step's addresses are the first's plus an immediate
            int key0 = 0;
            for (; key0 + 64 < n; key0 += 64) {
                step(key0, C0{}, sa, sb, kf);
                step(key0, C32{}, sb, sa, kf);
            }
            if (key0 + 32 < n) {
                step(key0, C0{}, sa, sb, kf);
                last(key0, C32{}, sb, kf);
            } else {
                last(key0, C0{}, sa, kf);
            }
#pragma unroll
            for (int qt = 0; qt < NQ; ++qt) {
                const float inv = 1.0f / l[qt][0];
                const int q = q_base + 16 * qt + c;
                if (q < nq) {
                    bf16 *out = ctx + (int64_t)(out0 + q) * H + h * ATT_D + 4 * g;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        bf16x4 v;
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = (bf16)(o[qt][dt][r] * inv);
                        *reinterpret_cast<bf16x4 *>(out + dt * 16) = v;
                    }
                }
            }
        };
        // this wave's tiles, two at a time (documents past 8 x 32 queries, x 16 with
        // qsel, take a second group, its Q loaded here)
        for (int i = 0; 2 * i < t_cnt;) {
            if (t_cnt - 2 * i >= 2)
                key_loop(std::integral_constant<int, 2>{}, qc, (t_first + 2 * i) * 16);
            else
                key_loop(std::integral_constant<int, 1>{}, qc, (t_first + 2 * i) * 16);
            if (2 * ++i >= t_cnt) break;
            load_q_wait(p, i, qc);
        }
        // !DB: every wave is done with the buffer before the next pair restages it (DB:
        // the barrier at the top of the next pair orders buffer b's restaging, which
        // is issued after it, behind every wave's reads of this pair)
        if (!DB) __syncthreads();
    };
    uint4 qc[QTB][2], qn[QTB][2];
    int p = blockIdx.x, b = 0;
    if (DB && p < n_pairs) {
        stage(p, 0);
        load_q(p, qn);
    }
    for (; p < n_pairs; p += gridDim.x, b ^= (DB ? 1 : 0)) run_pair(p, b, qc, qn);
}

bool attention_v3_ok(int max_len, int H) { return max_len <= 512 && H % ATT_D == 0; }

void launch_attention_v3(const bf16 *qkv, const int32_t *cu_seqlens, int n_docs, int max_len,
                         int H, bf16 *ctx, hipStream_t s, const int32_t *qsel,
                         const int32_t *cu_qsel) {
    DI_REQUIRE(attention_v3_ok(max_len, H), DI_EINVAL, "attention v3: max_len %d > 512", max_len);
    if (n_docs == 0 || max_len == 0) return;
    const int n_heads = H / ATT_D, n_pairs = n_docs * n_heads;
    // the kernel's pair -> document multiply-high is exact for pairs < 2^32 / n_heads
    DI_REQUIRE((int64_t)n_pairs * n_heads < (1ll << 32), DI_ERANGE, "attention v3: %d pairs", n_pairs);
    const int grid = std::min(n_pairs, n_cu());
    // ([0]: the double-buffered form, documents of up to 320 tokens)
    static std::atomic<uint64_t> set_on[2];
    auto launch = [&](auto kern, int lds_bytes, std::atomic<uint64_t> &on) {
        dynamic_lds_once(on, {{(const void *)kern, lds_bytes}});
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * ATT3_WAVES), lds_bytes, s, qkv, cu_seqlens,
                           H, n_heads, n_pairs, ctx, qsel, cu_qsel);
    };
    if (max_len <= Att3<true>::ROWS)
        launch(attention_v3_kernel<true>, Att3<true>::LDS, set_on[0]);
    else
        launch(attention_v3_kernel<false>, Att3<false>::LDS, set_on[1]);
    check_launch("attention_v3");
}

}  // namespace di
