// enc_attn_x3.hip -- fp32-faithful attention (precision bf16x3, head dim 64), gfx950:
// attention_x3_kernel, the unit order of its launches (attn_order_kernel) and their launchers.
//
// Every product as split bf16 (x = x_hi + x_lo, three 16x16x32 bf16 MFMAs per f32
// product: hi*hi + lo*hi + hi*lo, f32 accumulate, ~2^-17 relative per product) instead
// of f32 MFMA (1/16 of the bf16 rate): S^T = K Q^T from split K and Q, O^T = V^T P^T
// from split V and the split probabilities; softmax and the row sums in f32.  Q | K | V
// arrive as split rows [M][6H] from the QKV GEMM (split_col over the 3H logical
// columns): no V^T scatter.
//
// One persistent 512-thread workgroup per CU walks the (doc, head) pairs; the 8 waves
// own 48 queries each (three 16-query tiles; documents past 384 tokens take a second
// pass), and the keys stream through LDS in 64-key chunks, double-buffered: chunk i+1
// is copied by LDS-DMA (global_load_lds, every wave 1 KiB pieces of K and of V) while
// chunk i is computed, so every K / V byte is read from memory once per pass for the
// workgroup.
//   K and V images (16 KiB each): key row r = the head's 256 B [ch0 hi | ch0 lo | ch1 hi
//   | ch1 lo] (16-byte slots), slot j stored at j ^ ax_swz(r).
//   S^T fragment row c of tile t = key 8 (c >> 2) + 4 t + (c & 3), so lane group g holds
//   the consecutive keys 8 g..8 g + 7 of P^T (as attention_v3_kernel); the O^T A
//   operand (V^T) is read from the V rows with ds_read_b64_tr_b16.
// Fragment reads are inline-asm ds_reads with their lgkmcnt wait in the same statement
// (the compiler would otherwise drain the in-flight prefetch with vmcnt(0) before an
// LDS read it cannot tell apart from the DMA's destination).
//
// The kernel as it ships (the forms that led here -- tiles dealt 2w, 2w + 1, a cross-lane
// max at every sub-chunk, no interleave, two query tiles per wave -- were developer A/B
// variants and are gone; DESIGN.md keeps their measurements):
//   - wave w owns the 16-query tiles w, w + NW and w + 2 NW of a pass, so the tiles of a
//     short pass spread over the four SIMDs (wave w runs on SIMD w % 4), and a tile with
//     no query is skipped: the chunk loop is instantiated per count of non-empty tiles;
//   - lazy max: the softmax's reference max moves only when a score exceeds it by 8 / sc
//     (p <= 2^8): one compare per score and one ballot in the common case instead of the
//     cross-lane max; the scale folds into the exponent's fma;
//   - two or three tiles: tile i + 1's S^T products are interleaved with tile i's
//     exponentials, and the first O^T products with the last tile's (sched_group_barrier),
//     so the softmax issues in the MFMAs' shadow.  One tile: products and softmax in turn.
// Template parameters, the two shipped forms being <8, 64> and <4, 32>:
//   NW: waves per workgroup.  8: one workgroup per CU, 384-query passes.  4: two
//       workgroups per CU (64 KiB of LDS and <= 256 VGPRs each), 192-query passes -- a SIMD
//       idle at one workgroup's short last pass runs the other workgroup's wave.
//   KC: keys per staged chunk (64; 32 halves the K / V buffers for the 4-wave form).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "di_common.h"
#include "enc_attn.h"
#include "enc_handle.h"
#include "enc_launch.h"

namespace di {

constexpr int AX_QTN = 3;  // query tiles per wave and pass
// Image swizzle: slot j of key row r at j ^ ax_swz(r), ax_swz(r) = r0 r1 r3 in bits 1-3.
// A ds_read_b128 lane group (16 lanes: rows c&3 + 8 (c>>2) + 4 t, slot bit 0 = g) and a
// ds_read_b64_tr_b16 lane group (32 lanes: rows q + 8 g + 4 h2, slot bit 0 = p>>1)
// then reach 16 distinct slots (every 256-byte row starts at bank 0): conflict-free
// (r & 15 conflicts 2-way on both).  Row bit 5 (the 32-key sub-chunk) is not used, so
// the sub-chunk stays an immediate offset.
__device__ __forceinline__ int ax_swz(int r) { return ((r & 3) << 1) | (r & 8); }
// LDS: [K image, buffer 0 | K, buffer 1 | V, buffer 0 | V, buffer 1], one image = KC
// key rows of 256 B; every fragment read's (buffer, sub-chunk) offset is an immediate.
// (Measured: 128-key chunks -- half the barriers -- and raised MFMA issue priority
// were both slower, r03 ab_attn.)
// Q through LDS: every wave copies the next unit's query fragments by LDS-DMA into a
// region of its own ([qt][ch][hi, lo] x 1 KiB, lane l's 16 B at l * 16) with the chunk
// staging, and reads them into registers once at the unit's start -- no second set of
// Q registers live across the chunk loop (and none of the moves its conditional load
// cost at every chunk)
constexpr int AX_QTB = 4096;  // Q region bytes per query tile
constexpr int ax_lds(int nw, int kc) { return 4 * kc * 256 + nw * AX_QTN * AX_QTB; }
// Row bit 2 of an image (the K tile t, the V half h2) is not in the swizzle, so those
// halves are the immediate offset 4 * 256 of one address register
constexpr int AX_HALF = 1024;

// The fragment reads of one 32-key sub-chunk, OFF = its (stage buffer, sub-chunk) byte
// offset.  One asm statement for a group's reads and their wait: the outputs exist only
// after it (with a separate wait the compiler copied V^T registers above it --
// tools/asm_wait_scan.py).
// K: kf[t][ch][hi, lo] from the addresses ka[ch][hi, lo]
template <int OFF>
__device__ __forceinline__ void ax_read_k(const uint32_t (&ka)[2][2], uint4 (&kf)[2][2][2]) {
    asm volatile(
        "ds_read_b128 %0, %8 offset:%12"
        "\n\tds_read_b128 %1, %9 offset:%12"
        "\n\tds_read_b128 %2, %10 offset:%12"
        "\n\tds_read_b128 %3, %11 offset:%12"
        "\n\tds_read_b128 %4, %8 offset:%13"
        "\n\tds_read_b128 %5, %9 offset:%13"
        "\n\tds_read_b128 %6, %10 offset:%13"
        "\n\tds_read_b128 %7, %11 offset:%13"
        "\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(kf[0][0][0]), "=&v"(kf[0][0][1]), "=&v"(kf[0][1][0]), "=&v"(kf[0][1][1]),
          "=&v"(kf[1][0][0]), "=&v"(kf[1][0][1]), "=&v"(kf[1][1][0]), "=&v"(kf[1][1][1])
        : "v"(ka[0][0]), "v"(ka[0][1]), "v"(ka[1][0]), "v"(ka[1][1]),
          "i"(OFF), "i"(OFF + AX_HALF)
        : "memory");
}
// V^T: vt2[dt][hi, lo][h2] from the addresses va[dt][hi, lo]
template <int OFF>
__device__ __forceinline__ void ax_read_vt(const uint32_t (&va)[4][2], uint2 (&vt2)[4][2][2]) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %16 offset:%24"
        "\n\tds_read_b64_tr_b16 %1, %16 offset:%25"
        "\n\tds_read_b64_tr_b16 %2, %17 offset:%24"
        "\n\tds_read_b64_tr_b16 %3, %17 offset:%25"
        "\n\tds_read_b64_tr_b16 %4, %18 offset:%24"
        "\n\tds_read_b64_tr_b16 %5, %18 offset:%25"
        "\n\tds_read_b64_tr_b16 %6, %19 offset:%24"
        "\n\tds_read_b64_tr_b16 %7, %19 offset:%25"
        "\n\tds_read_b64_tr_b16 %8, %20 offset:%24"
        "\n\tds_read_b64_tr_b16 %9, %20 offset:%25"
        "\n\tds_read_b64_tr_b16 %10, %21 offset:%24"
        "\n\tds_read_b64_tr_b16 %11, %21 offset:%25"
        "\n\tds_read_b64_tr_b16 %12, %22 offset:%24"
        "\n\tds_read_b64_tr_b16 %13, %22 offset:%25"
        "\n\tds_read_b64_tr_b16 %14, %23 offset:%24"
        "\n\tds_read_b64_tr_b16 %15, %23 offset:%25"
        "\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(vt2[0][0][0]), "=&v"(vt2[0][0][1]), "=&v"(vt2[0][1][0]), "=&v"(vt2[0][1][1]),
          "=&v"(vt2[1][0][0]), "=&v"(vt2[1][0][1]), "=&v"(vt2[1][1][0]), "=&v"(vt2[1][1][1]),
          "=&v"(vt2[2][0][0]), "=&v"(vt2[2][0][1]), "=&v"(vt2[2][1][0]), "=&v"(vt2[2][1][1]),
          "=&v"(vt2[3][0][0]), "=&v"(vt2[3][0][1]), "=&v"(vt2[3][1][0]), "=&v"(vt2[3][1][1])
        : "v"(va[0][0]), "v"(va[0][1]), "v"(va[1][0]), "v"(va[1][1]),
          "v"(va[2][0]), "v"(va[2][1]), "v"(va[3][0]), "v"(va[3][1]),
          "i"(OFF), "i"(OFF + AX_HALF)
        : "memory");
}
// f(integral_constant<OFF>) for stage buffer b (0 or 1 at run time, at b * IMG) and
// sub-chunk u (a constant of the caller's unrolled loop, at u * 32 rows): one branch per
// site -- a switch over the offsets' value range compiled to a chain of compares
template <int KC, class F>
__device__ __forceinline__ void ax_sel(int b, int u, F f) {
    constexpr int IMG = KC * 256, SUB = 32 * 256;
    static_assert(KC == 64 || KC == 32, "one or two sub-chunks per chunk");
    if constexpr (KC == 64) {
        if (b) {
            if (u) f(std::integral_constant<int, IMG + SUB>{});
            else f(std::integral_constant<int, IMG>{});
        } else {
            if (u) f(std::integral_constant<int, SUB>{});
            else f(std::integral_constant<int, 0>{});
        }
    } else {
        if (b) f(std::integral_constant<int, IMG>{});
        else f(std::integral_constant<int, 0>{});
    }
}
// a 12-MFMA region: 1 MFMA : 4 VALU (incl. transcendental) groups.  (A macro: as a
// __forceinline__ function the same barriers left the 4-wave form with 4 more VGPRs and
// both forms with ~20 more instructions -- profiles/attention_refactor_isa.txt.)
#define AX_INTERLEAVE()                                                                            \
    do {                                                                                           \
        _Pragma("unroll") for (int i_ = 0; i_ < 12; ++i_) {                                        \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
            __builtin_amdgcn_sched_group_barrier(0x402, 4, 0);                                     \
        }                                                                                          \
    } while (0)

// The lazy max's rare step for one query tile, after a score passed lim: v = the lane's 8
// raw scores (masked keys -inf), m = the reference max in raw units, lim = m + 8 / sc,
// mneg = -m sc.  Per query: a row whose own scores stay under its limit keeps its
// reference, whatever the tile's other rows do -- its arithmetic must not depend on which
// queries share the tile (the pruned last layer regroups them).
__device__ __forceinline__ void ax_move_max(const float (&v)[8], float &m, float &lim,
                                            float &mneg, float &lsum, f32x4 (&o)[4]) {
    constexpr float sc = ATT_SC;
    const float cmax = lane_group_max(fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])),
                                            fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7]))));
    const float m_new = cmax > lim ? fmaxf(m, cmax) : m;
    if (m_new != m) {  // (per lane; alpha = 0 at a unit's first sub-chunk)
        const float alpha = __builtin_amdgcn_exp2f((m - m_new) * sc);
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    }
    m = m_new;
    lim = m_new + 8.0f / sc;
    mneg = -m_new * sc;
}

#ifdef DI_ATTN_STAMP
// Diagnostic build only (never the product's): every workgroup's first and last clock
// reading (100 MHz) of one launch, in a buffer of their own that no kernel reads;
// ax_stamp_report prints the spread of the finish times (DI_ATTN_STAMP_FROM / _COUNT:
// which launches of the process)
__device__ unsigned long long ax_stamp[2][1024];
#endif

template <int NW, int KC>
__global__ void __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(2)))
attention_x3_kernel(const bf16 *__restrict__ qkv, const int32_t *__restrict__ cu_seqlens, int H,
                    int n_heads, int n_pairs, bf16 *__restrict__ ctx_split,
                    const int32_t *__restrict__ qsel, const int32_t *__restrict__ cu_qsel,
                    const int32_t *__restrict__ q_order, const int32_t *__restrict__ q_range,
                    int abl) {
    // abl (developer timing ablations, wrong results; 1, 2 and 4 act on a wave's one-tile
    // loop only): 1 no softmax arithmetic, 2 no S^T products, 4 no O^T products, 16 no
    // second pass
    // qsel (optional, the pruned last layer): only the query rows qsel[cu_qsel[d] ..)
    // (doc-local token indices) of document d are computed, into ctx rows cu_qsel[d] + i;
    // keys and values are every token of the document either way.
    constexpr int QTN = AX_QTN;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;
#ifdef DI_ATTN_STAMP
    if (lane == 0)
        atomicMin(&ax_stamp[0][blockIdx.x], (unsigned long long)__builtin_amdgcn_s_memrealtime());
    __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
    const int64_t ld = 6 * (int64_t)H;  // split row: 3H logical columns
    const uint32_t lds_base =
        (uint32_t)(uintptr_t)((__attribute__((address_space(3))) unsigned char *)lds);
    const float sc = ATT_SC;
    constexpr int PASS_Q = NW * QTN * 16;         // queries per pass (384 or 192)
    constexpr int IMG = KC * 256, KVL = 4 * IMG;  // one K or V image; the four of them

    // Work units: (pair, pass) (persistent); the next unit's Q and first K / V chunk load
    // while the current unit's last chunk computes.  In round r this workgroup takes pair
    // r * gridDim.x + blockIdx.x.  With a unit order (q_order: the documents longest first;
    // q_range: the [lo, hi) of that list this launch computes) the pairs are counted along
    // the list and odd rounds deal backwards, blockIdx.x gridDim.x - 1 first: a round's
    // pairs cost nearly the same and what differences there are cancel from round to round,
    // so every workgroup ends at nearly the same time, whatever the documents' lengths.
    // Every quantity here is the same in all of a workgroup's waves (the barriers of the
    // chunk loop depend on them).
    struct Unit {
        int r, pass, tok0, n, h, q0, nq;  // q0: ctx row of query 0; nq: queries
    };
    const int q_lo = q_order ? q_range[0] : 0;
    const int n_units = q_order ? (q_range[1] - q_lo) * n_heads : n_pairs;
    // round r's unit (pass 0), or false past the last pair
    auto make_unit = [&](int r, Unit &u) {
        const int gs = (int)gridDim.x, bx = (int)blockIdx.x;
        const int64_t i = (int64_t)r * gs + ((q_order && (r & 1)) ? gs - 1 - bx : bx);
        if (i >= n_units) return false;
        const int di = (int)i / n_heads;
        const int doc = q_order ? q_order[q_lo + di] : di;
        u.r = r;
        u.pass = 0;
        u.h = (int)i - di * n_heads;
        u.tok0 = cu_seqlens[doc];
        u.n = cu_seqlens[doc + 1] - u.tok0;
        u.q0 = qsel ? cu_qsel[doc] : u.tok0;
        u.nq = qsel ? cu_qsel[doc + 1] - u.q0 : u.n;
        return true;
    };
    // the unit after `u` with at least one token and one query, or false
    auto next_unit = [&](const Unit &u, Unit &nu) {
        if ((u.pass + 1) * PASS_Q < u.nq && !(abl & 16)) {
            nu = u;
            nu.pass = u.pass + 1;
            return true;
        }
        for (int r = u.r + 1; make_unit(r, nu); ++r)
            if (nu.n > 0 && nu.nq > 0) return true;
        return false;
    };
    // chunk ci of unit u -> stage buffer b: key rows RPW wave..+RPW-1 of K and of V
    // (RPW / 4 pieces of 1 KiB each), 16 B per lane, source slots permuted by the
    // swizzle (piece pc: key rows RPW wave + 4 pc + lane >> 4)
    constexpr int RPW = KC / NW;  // key rows per wave and image (8 or 16)
    const int sr = RPW * wave + (lane >> 4);
    auto stage = [&](const Unit &u, int ci, int b) {
        const bf16 *kg = qkv + split_col(H + u.h * ATT_D);      // + key row * ld: 256 B
        const bf16 *vg = qkv + split_col(2 * H + u.h * ATT_D);
#pragma unroll
        for (int pc = 0; pc < RPW / 4; ++pc) {
            const int rl = sr + 4 * pc;
            const int row = u.tok0 + min(ci * KC + rl, u.n - 1);
            const int j = (lane & 15) ^ ax_swz(rl);
            const int dst = b * IMG + (RPW * wave + 4 * pc) * 256;
            __builtin_amdgcn_global_load_lds((const void *)(kg + row * ld + j * 8),
                                             (lds_void *)(lds + dst), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void *)(vg + row * ld + j * 8),
                                             (lds_void *)(lds + 2 * IMG + dst), 16, 0, 0);
        }
    };
    // first query (within its pass) of this wave's tile qt
    auto qtile = [&](int qt) { return 16 * (wave + NW * qt); };
    // unit u's query fragments of this wave -> its Q region (LDS-DMA, 8 x 1 KiB)
    auto dma_q = [&](const Unit &u) {
        const bf16 *qbase = qkv + split_col(u.h * ATT_D) + 8 * g;
#pragma unroll
        for (int qt = 0; qt < QTN; ++qt) {
            const int qi = min(u.pass * PASS_Q + qtile(qt) + c, u.nq - 1);
            const int qloc = qsel ? min(max(qsel[u.q0 + qi], 0), u.n - 1) : qi;
            const int qrow = u.tok0 + qloc;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const bf16 *src = qbase + qrow * ld + ch * 64;
                const int dst = KVL + wave * (QTN * AX_QTB) + (qt * 2 + ch) * 2048;
                __builtin_amdgcn_global_load_lds((const void *)src, (lds_void *)(lds + dst), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const void *)(src + 32),
                                                 (lds_void *)(lds + dst + 1024), 16, 0, 0);
            }
        }
    };
    // fragment addresses (buffer 0; buffer 1 is the immediate offset IMG; the K tile t and
    // the V half h2 the immediate offset AX_HALF: 12 VGPRs instead of 24)
    uint32_t ka[2][2];  // [ch][hi, lo]: key row 8 (c >> 2) + (c & 3) (+ 4 t: + AX_HALF)
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int r = 8 * (c >> 2) + (c & 3), j = ch * 8 + pt * 4 + g;
            ka[ch][pt] = lds_base + r * 256 + ((j ^ ax_swz(r)) << 4);
        }
    // [dt][hi, lo]: ds_read_b64_tr_b16 roles -- lane 4 q + p of a 16-lane group addresses
    // key row 8 g + 4 h2 + q (h2: + AX_HALF), columns 16 dt + 4 p..+3 (one 8-byte half
    // slot); lane i then holds column d = 16 dt + i for keys 8 g + 4 h2 + 0..3
    uint32_t va[4][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int q = c >> 2, pp = c & 3;
            const int r = 8 * g + q;
            const int j = (dt >> 1) * 8 + pt * 4 + 2 * (dt & 1) + (pp >> 1);
            va[dt][pt] = lds_base + 2 * IMG + r * 256 + ((j ^ ax_swz(r)) << 4) + 8 * (pp & 1);
        }

    Unit cu;
    for (int r = 0;; ++r) {
        if (!make_unit(r, cu)) return;  // (no unit, or none with a token and a query)
        if (cu.n > 0 && cu.nq > 0) break;
    }
    bf16x8 qh[QTN][2], ql[QTN][2];
    const uint32_t qa = lds_base + KVL + wave * (QTN * AX_QTB) + lane * 16;
    // this wave's Q region -> qh / ql (landed: the caller waited vmcnt(0))
    auto read_q = [&]() {
        uint4 q4[8];
        asm volatile(
            "ds_read_b128 %0, %8 offset:0"
            "\n\tds_read_b128 %1, %8 offset:1024"
            "\n\tds_read_b128 %2, %8 offset:2048"
            "\n\tds_read_b128 %3, %8 offset:3072"
            "\n\tds_read_b128 %4, %8 offset:4096"
            "\n\tds_read_b128 %5, %8 offset:5120"
            "\n\tds_read_b128 %6, %8 offset:6144"
            "\n\tds_read_b128 %7, %8 offset:7168"
            "\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(q4[0]), "=&v"(q4[1]), "=&v"(q4[2]), "=&v"(q4[3]), "=&v"(q4[4]),
              "=&v"(q4[5]), "=&v"(q4[6]), "=&v"(q4[7])
            : "v"(qa)
            : "memory");
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                __builtin_memcpy(&qh[qt][ch], &q4[(qt * 2 + ch) * 2], 16);
                __builtin_memcpy(&ql[qt][ch], &q4[(qt * 2 + ch) * 2 + 1], 16);
            }
        uint4 q5[4];  // tile 2
        asm volatile(
            "ds_read_b128 %0, %4 offset:8192"
            "\n\tds_read_b128 %1, %4 offset:9216"
            "\n\tds_read_b128 %2, %4 offset:10240"
            "\n\tds_read_b128 %3, %4 offset:11264"
            "\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(q5[0]), "=&v"(q5[1]), "=&v"(q5[2]), "=&v"(q5[3])
            : "v"(qa)
            : "memory");
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            __builtin_memcpy(&qh[2][ch], &q5[ch * 2], 16);
            __builtin_memcpy(&ql[2][ch], &q5[ch * 2 + 1], 16);
        }
    };
    stage(cu, 0, 0);
    dma_q(cu);
    int b = 0;  // stage buffer of the next chunk to compute
    for (;;) {
        const int n = cu.n, h = cu.h, q0 = cu.q0, nq = cu.nq;
        const int q_pass = cu.pass * PASS_Q;
        // (uniform) this wave's tile 0 / 1 / 2 has queries
        const bool has_q = q_pass + qtile(0) < nq;
        const bool two = q_pass + qtile(1) < nq;
        const bool three = q_pass + qtile(2) < nq;
        const int n_chunks = (n + KC - 1) / KC;
        Unit nu;
        const bool more = next_unit(cu, nu);
        float m[QTN], lsum[QTN], lim[QTN], mneg[QTN];
        f32x4 o[QTN][4];
#pragma unroll
        for (int qt = 0; qt < QTN; ++qt) {
            m[qt] = -INFINITY;
            lim[qt] = -INFINITY;
            mneg[qt] = 0.f;
            lsum[qt] = 0.f;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // The chunk loop for a unit whose wave has NQT (1, 2 or 3) query tiles -- one loop per
        // count, not a choice per chunk: with the choice inside, the two bodies left the
        // O accumulators in different registers and the loop's back edge moved them
        // (16 v_mov_b64 + 12 v_mov per chunk in the ISA)
        // (and the unit's whole 64-key chunks in a loop of their own, the partial last chunk
        // after it: a sub-chunk loop that may stop after its first sub-chunk also left them
        // in different registers, moved at the top and the bottom of every chunk)
        // (and a wave with no query in the unit runs the staging alone: a body that may
        // skip its products also moved the accumulators)
        auto stage_next = [&](const int ci) {
            if (ci + 1 < n_chunks) {
                stage(cu, ci + 1, b ^ 1);
            } else if (more) {  // the next unit's first chunk and Q
                stage(nu, 0, b ^ 1);
                dma_q(nu);
            }
        };
        // chunk ci > 0 (chunk 0's wait is the unit's start, below)
        auto stage_step = [&](const int ci) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of chunk ci
            __syncthreads();  // every piece landed; buffer b ^ 1 no longer read
            stage_next(ci);
        };
        // unit start: chunk 0 and this wave's Q landed; Q into registers before the next
        // unit's Q copy can be issued (stage_next(0) issues it for a one-chunk unit)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        read_q();
        stage_next(0);
        // the unit's chunks for a wave with NQT non-empty query tiles
        auto chunk_loop = [&](auto nqt_c) {
            constexpr int NQT = decltype(nqt_c)::value;
            // chunk ci; WHOLE: all of its KC keys are the document's
            auto one_chunk = [&](const int ci, auto whole_c) {
                constexpr bool WHOLE = decltype(whole_c)::value;
                if (ci > 0) stage_step(ci);
                // the chunk's 32-key sub-chunks.  (A lambda of its own: written into
                // one_chunk the compiler shares one scalar test between two sub-chunks of
                // the 8-wave form's one-tile loop, and the kernel is no longer the measured
                // one instruction for instruction.)
                auto sub_chunks = [&]() {
#pragma unroll
                    for (int u = 0; u < KC / 32; ++u) {
                        const int key0 = ci * KC + 32 * u;
                        if (!WHOLE && key0 >= n) break;
                        uint4 kf[2][2][2];
                        uint2 vt2[4][2][2];
                        auto read_k = [&](auto off) __attribute__((always_inline)) {
                            ax_read_k<decltype(off)::value>(ka, kf);
                        };
                        auto read_vt = [&](auto off) __attribute__((always_inline)) {
                            ax_read_vt<decltype(off)::value>(va, vt2);
                        };
                        ax_sel<KC>(b, u, read_k);
                        __builtin_amdgcn_sched_barrier(0);
                        bf16x8 kfr[2][2][2];  // [t][ch][hi, lo]
#pragma unroll
                        for (int t = 0; t < 2; ++t)
#pragma unroll
                            for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                                for (int pt = 0; pt < 2; ++pt)
                                    __builtin_memcpy(&kfr[t][ch][pt], &kf[t][ch][pt], 16);
                        bf16x8 vfr[4][2];  // [dt][hi, lo], from vt2 once its read has waited
                        auto take_vt = [&]() {
#pragma unroll
                            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                                for (int pt = 0; pt < 2; ++pt) {
                                    const uint4 v4 = make_uint4(vt2[dt][pt][0].x, vt2[dt][pt][0].y,
                                                                vt2[dt][pt][1].x, vt2[dt][pt][1].y);
                                    __builtin_memcpy(&vfr[dt][pt], &v4, 16);
                                }
                        };
                        if constexpr (NQT >= 2) {
                            // (uniform) no masked key in this sub-chunk
                            const bool full = WHOLE || key0 + 32 <= n;
                            f32x4 s[QTN][2];
                            float v[QTN][8];
                            bf16x8 ph[QTN], pl[QTN];
                            // S^T of tile qt (12 MFMAs; the two accumulators' chains interleaved)
                            auto s_mfma = [&](int qt) {
                                s[qt][0] = s[qt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                                    for (int p = 0; p < 3; ++p)
#pragma unroll
                                        for (int t = 0; t < 2; ++t)
                                            s[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                                kfr[t][ch][p == 1], p == 2 ? ql[qt][ch] : qh[qt][ch],
                                                s[qt][t], 0, 0, 0);
                            };
                            // softmax part A of tile qt: masked raw scores, the lazy max test and
                            // the rare rescale (a branch: outside the interleaved regions)
                            auto soft_a = [&](int qt) {
                                // (a uniform branch: the common full sub-chunk takes the scores
                                // as they are, without 8 compares and selects per tile)
                                if (full) {
#pragma unroll
                                    for (int e = 0; e < 8; ++e) v[qt][e] = s[qt][e >> 2][e & 3];
                                } else {
                                    // (key 8 g + e of the sub-chunk is valid iff e < n - key0 -
                                    // 8 g: one value per lane against constants, not 8 hoisted
                                    // key offsets)
                                    const int kv = n - key0 - 8 * g;
#pragma unroll
                                    for (int e = 0; e < 8; ++e)
                                        v[qt][e] = e < kv ? s[qt][e >> 2][e & 3] : -INFINITY;
                                }
                                // (the test by compares: the max, with its NaN-canonicalising
                                // operand maxes, only on the rare path)
                                bool up = false;
#pragma unroll
                                for (int e = 0; e < 8; ++e) up |= v[qt][e] > lim[qt];
                                if (__any(up))
                                    ax_move_max(v[qt], m[qt], lim[qt], mneg[qt], lsum[qt], o[qt]);
                            };
                            // softmax part B: the exponentials, row sums and split probabilities
                            auto soft_b = [&](int qt) {
#pragma unroll
                                for (int e = 0; e < 8; ++e) {
                                    const float pr =
                                        __builtin_amdgcn_exp2f(fmaf(v[qt][e], sc, mneg[qt]));
                                    lsum[qt] += pr;
                                    ph[qt][e] = split_hi(pr);
                                    pl[qt][e] = split_lo(pr);
                                }
                            };
                            auto o_mfma = [&](int qt) {
#pragma unroll
                                for (int p = 0; p < 3; ++p)
#pragma unroll
                                    for (int dt = 0; dt < 4; ++dt)
                                        o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                            vfr[dt][p == 1], p == 2 ? pl[qt] : ph[qt], o[qt][dt], 0,
                                            0, 0);
                            };
                            s_mfma(0);
                            __builtin_amdgcn_sched_barrier(0);
                            ax_sel<KC>(b, u, read_vt);  // (their wait overlaps tile 0's products)
                            __builtin_amdgcn_sched_barrier(0);
                            take_vt();
                            soft_a(0);
                            __builtin_amdgcn_sched_barrier(0);
                            s_mfma(1);
                            soft_b(0);
                            AX_INTERLEAVE();
                            __builtin_amdgcn_sched_barrier(0);
                            soft_a(1);
                            __builtin_amdgcn_sched_barrier(0);
                            if constexpr (NQT == 3) {  // tile 2's products in tile 1's shadow
                                s_mfma(2);
                                soft_b(1);
                                AX_INTERLEAVE();
                                __builtin_amdgcn_sched_barrier(0);
                                soft_a(2);
                                __builtin_amdgcn_sched_barrier(0);
                                o_mfma(0);
                                soft_b(2);
                                AX_INTERLEAVE();
                                __builtin_amdgcn_sched_barrier(0);
                                o_mfma(1);
                                o_mfma(2);
                            } else {
                                o_mfma(0);
                                soft_b(1);
                                AX_INTERLEAVE();
                                __builtin_amdgcn_sched_barrier(0);
                                o_mfma(1);
                            }
                        } else {
                            // one tile (NQT = 1: the loops over qt run once; written for
                            // qt = 0 alone the softmax below is scheduled differently, see
                            // profiles/attention_refactor_isa.txt): S^T, each product stage over
                            // the 2 independent accumulators before the next (one accumulator's
                            // 3 products are a chain)
                            f32x4 s[QTN][2];
#pragma unroll
                            for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                                for (int t = 0; t < 2; ++t) s[qt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                            if (!(abl & 2))
#pragma unroll
                                for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                                    for (int p = 0; p < 3; ++p)
#pragma unroll
                                        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                                            for (int t = 0; t < 2; ++t)
                                                s[qt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                                    kfr[t][ch][p == 1],
                                                    p == 2 ? ql[qt][ch] : qh[qt][ch], s[qt][t], 0, 0,
                                                    0);
                            __builtin_amdgcn_sched_barrier(0);
                            ax_sel<KC>(b, u, read_vt);
                            __builtin_amdgcn_sched_barrier(0);
                            const bool full = WHOLE || key0 + 32 <= n;  // (as above)
                            bf16x8 ph[QTN], pl[QTN];
                            if (abl & 1) {
#pragma unroll
                                for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                                    for (int e = 0; e < 8; ++e) {
                                        ph[qt][e] = (bf16)s[qt][e >> 2][e & 3];
                                        pl[qt][e] = ph[qt][e];
                                    }
                            } else {
#pragma unroll
                                for (int qt = 0; qt < NQT; ++qt) {
                                    // raw scores (masked keys -inf); the reference max m is in raw units
                                    float v[8];
                                    const int kv = n - key0 - 8 * g;  // key 8 g + e valid iff e < kv
#pragma unroll
                                    for (int e = 0; e < 8; ++e)  // (t = e >> 2, r = e & 3)
                                        v[e] = (full || e < kv) ? s[qt][e >> 2][e & 3] : -INFINITY;
                                    bool up = false;  // (by compares, as soft_a)
#pragma unroll
                                    for (int e = 0; e < 8; ++e) up |= v[e] > lim[qt];
                                    // (always at a unit's first sub-chunk: lim = -inf, key 0 is valid)
                                    if (__any(up))
                                        ax_move_max(v, m[qt], lim[qt], mneg[qt], lsum[qt], o[qt]);
#pragma unroll
                                    for (int e = 0; e < 8; ++e) {
                                        const float pr = __builtin_amdgcn_exp2f(fmaf(v[e], sc, mneg[qt]));
                                        lsum[qt] += pr;
                                        ph[qt][e] = split_hi(pr);
                                        pl[qt][e] = split_lo(pr);
                                    }
                                }
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            take_vt();
                            if (!(abl & 4))
#pragma unroll
                                for (int p = 0; p < 3; ++p)
#pragma unroll
                                    for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                                        for (int dt = 0; dt < 4; ++dt)
                                            o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                                vfr[dt][p == 1], p == 2 ? pl[qt] : ph[qt], o[qt][dt],
                                                0, 0, 0);
                        }
                    }
                };
                sub_chunks();
            };
            const int n_whole = n / KC;
            int ci = 0;
            for (; ci < n_whole; ++ci, b ^= 1) one_chunk(ci, std::true_type{});
            if (ci < n_chunks) {
                one_chunk(ci, std::false_type{});
                b ^= 1;
            }
        };
        if (!has_q) {
            for (int ci = 0; ci < n_chunks; ++ci, b ^= 1)
                if (ci > 0) stage_step(ci);
        } else if (three) {
            chunk_loop(std::integral_constant<int, 3>{});
        } else if (two) {
            chunk_loop(std::integral_constant<int, 2>{});
        } else {
            chunk_loop(std::integral_constant<int, 1>{});
        }
        if (has_q) {
#pragma unroll
            for (int qt = 0; qt < QTN; ++qt) {
                float l = lsum[qt];
                l += __shfl_xor(l, 16, 64);
                l += __shfl_xor(l, 32, 64);
                const float inv = 1.0f / l;
                const int q = q_pass + qtile(qt) + c;
                if (q < nq) {
                    bf16 *out = ctx_split + (int64_t)(q0 + q) * 2 * H;
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        bf16x4 hv, lv;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float y = o[qt][dt][r] * inv;
                            hv[r] = split_hi(y);
                            lv[r] = split_lo(y);
                        }
                        const int64_t sc0 = split_col(h * ATT_D + dt * 16 + 4 * g);
                        *reinterpret_cast<bf16x4 *>(out + sc0) = hv;
                        *reinterpret_cast<bf16x4 *>(out + sc0 + 32) = lv;
                    }
                }
            }
        }
        if (!more) break;
        cu = nu;
    }
#ifdef DI_ATTN_STAMP
    if (lane == 0)
        atomicMax(&ax_stamp[1][blockIdx.x], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
}

// The unit order of one encode call: order[0 .. n_docs) = the documents by token count,
// longest first, ties to the lower document (a counting sort over the lengths 0 ..
// max_len, lengths outside clamped: whatever cu_seqlens holds, order is a permutation);
// ctl = {0, n_long, n_docs, 0, n_docs}, n_long = documents of more than long_len tokens.
// One workgroup: a histogram, its running sum from the longest length down, then thread b
// places the documents of length b in document order, reading the lengths from LDS tiles.
constexpr int AQ_THREADS = 1024, AQ_TILE = 4096;
__global__ void __launch_bounds__(AQ_THREADS)
attn_order_kernel(const int32_t *__restrict__ cu_seqlens, int n_docs, int max_len, int long_len,
                  int32_t *__restrict__ order, int32_t *__restrict__ ctl) {
    extern __shared__ int32_t aq_lds[];  // start[max_len + 1] | tile[AQ_TILE]
    int32_t *start = aq_lds, *tile = aq_lds + (max_len + 1);
    const int tid = threadIdx.x;
    auto len_of = [&](int d) {
        return min(max(cu_seqlens[d + 1] - cu_seqlens[d], 0), max_len);
    };
    for (int b = tid; b <= max_len; b += AQ_THREADS) start[b] = 0;
    __syncthreads();
    for (int d = tid; d < n_docs; d += AQ_THREADS) atomicAdd(&start[len_of(d)], 1);
    __syncthreads();
    if (tid == 0) {
        int acc = 0, n_long = 0;
        for (int b = max_len; b >= 0; --b) {
            const int cnt = start[b];
            start[b] = acc;
            acc += cnt;
            if (b == long_len + 1) n_long = acc;
        }
        ctl[0] = 0;
        ctl[1] = n_long;
        ctl[2] = n_docs;
        ctl[3] = 0;
        ctl[4] = n_docs;
    }
    __syncthreads();
    for (int t0 = 0; t0 < n_docs; t0 += AQ_TILE) {
        const int nt = min(AQ_TILE, n_docs - t0);
        for (int i = tid; i < nt; i += AQ_THREADS) tile[i] = len_of(t0 + i);
        __syncthreads();
        for (int b = tid; b <= max_len; b += AQ_THREADS) {
            int pos = start[b];  // (< n_docs: the histogram counted every document once)
            for (int i = 0; i < nt; ++i)
                if (tile[i] == b) order[pos++] = t0 + i;
            start[b] = pos;
        }
        __syncthreads();
    }
}

bool attn_order_ok(int max_positions) {
    return max_positions >= 0 && (size_t)(max_positions + 1 + AQ_TILE) * 4 <= 64 * 1024;
}

void launch_attn_order(const int32_t *cu_seqlens, int n_docs, int max_positions, int32_t *order,
                       int32_t *ctl, hipStream_t s) {
    DI_REQUIRE(attn_order_ok(max_positions), DI_ERANGE, "attention order: max_positions %d",
               max_positions);
    hipLaunchKernelGGL(attn_order_kernel, dim3(1), dim3(AQ_THREADS),
                       (size_t)(max_positions + 1 + AQ_TILE) * 4, s, cu_seqlens, n_docs,
                       max_positions, AQ_LONG_LEN, order, ctl);
    check_launch("attn_order");
}

int attn_queue_mode() {
    static const int mode = [] {
        const char *e = getenv("DI_ATTN_X3_QUEUE");
        return e ? atoi(e) : 2;
    }();
    return mode;
}

namespace {

// LDS of one CU and the most one workgroup may take (current device)
void ax_lds_limits(int &per_cu, int &per_wg) {
    int dev = 0, cu = 0, wg = 0;
    DI_HIP(hipGetDevice(&dev));
    DI_HIP(hipDeviceGetAttribute(&wg, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev);
    per_wg = wg;
    per_cu = std::max(cu, wg);
}

struct AxArgs {
    const bf16 *qkv;
    const int32_t *cu_seqlens;
    int H, n_heads;
    int64_t n_pairs;
    bf16 *ctx_split;
    const int32_t *qsel, *cu_qsel, *q_order, *q_range;
    int abl;
    hipStream_t s;
};

#ifdef DI_ATTN_STAMP
unsigned long long *ax_stamp_reset(hipStream_t s) {
    unsigned long long *st = nullptr;
    DI_HIP(hipGetSymbolAddress((void **)&st, HIP_SYMBOL(ax_stamp)));
    DI_HIP(hipMemsetAsync(st, 0xFF, 1024 * 8, s));
    DI_HIP(hipMemsetAsync(st + 1024, 0, 1024 * 8, s));
    return st;
}

// after the launch: the spread of its workgroups' finish times, to stderr
void ax_stamp_report(const unsigned long long *st, const AxArgs &a, int nw, int grid) {
    static int n_launch = 0;
    static const int from = getenv("DI_ATTN_STAMP_FROM") ? atoi(getenv("DI_ATTN_STAMP_FROM")) : 0;
    static const int cnt = getenv("DI_ATTN_STAMP_COUNT") ? atoi(getenv("DI_ATTN_STAMP_COUNT")) : 0;
    if (n_launch >= from && n_launch < from + cnt && grid <= 1024) {
        static unsigned long long h[2][1024];
        DI_HIP(hipStreamSynchronize(a.s));
        DI_HIP(hipMemcpy(h, st, sizeof h, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0;
        double sum = 0;
        int nb = 0;
        std::vector<unsigned long long> ends;
        for (int i = 0; i < grid; ++i)
            if (h[1][i]) {
                t0 = std::min(t0, h[0][i]);
                t1 = std::max(t1, h[1][i]);
                ends.push_back(h[1][i]);
                ++nb;
            }
        if (nb) {
            std::sort(ends.begin(), ends.end());
            for (auto e : ends) sum += (double)(e - t0);
            const double span = (double)(t1 - t0), mean = sum / nb;
            fprintf(stderr,
                    "ax_stamp launch %d NW=%d qsel=%d list=%d grid=%d busy=%d span_us=%.1f "
                    "mean_end=%.4f first_end=%.4f median_end=%.4f p90_end=%.4f tail=%.4f\n",
                    n_launch, nw, a.qsel != nullptr, a.q_order != nullptr, grid, nb, span * 0.01,
                    mean / span, (ends.front() - t0) / span, (ends[nb / 2] - t0) / span,
                    (ends[nb * 9 / 10] - t0) / span, 1.0 - mean / span);
        }
    }
    ++n_launch;
}
#endif

template <int NW, int KC>
void ax_launch(const AxArgs &a) {
    constexpr int LDS = ax_lds(NW, KC);
    const auto kern = attention_x3_kernel<NW, KC>;
    int per_cu = 0, per_wg = 0;
    ax_lds_limits(per_cu, per_wg);
    DI_REQUIRE(LDS <= per_wg, DI_ERANGE, "attention_x3: %d bytes of LDS, the device gives %d",
               LDS, per_wg);
    static std::atomic<uint64_t> set_on{0};
    dynamic_lds_once(set_on, {{(const void *)kern, LDS}});
    const int grid = (int)std::min<int64_t>(a.n_pairs, (int64_t)n_cu() * (per_cu / LDS));
#ifdef DI_ATTN_STAMP
    const unsigned long long *st = ax_stamp_reset(a.s);
#endif
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), LDS, a.s, a.qkv, a.cu_seqlens, a.H,
                       a.n_heads, (int)a.n_pairs, a.ctx_split, a.qsel, a.cu_qsel, a.q_order,
                       a.q_range, a.abl);
    check_launch("attention_x3");
#ifdef DI_ATTN_STAMP
    ax_stamp_report(st, a, NW, grid);
#endif
}

}  // namespace

void launch_attention_x3(const bf16 *qkv, const int32_t *cu_seqlens, int n_docs, int H,
                         bf16 *ctx_split, hipStream_t s, const int32_t *qsel,
                         const int32_t *cu_qsel, const AttnQueue *q) {
    DI_REQUIRE(H % ATT_D == 0, DI_EINVAL, "hidden %d is not a multiple of the head dim 64", H);
    if (n_docs == 0) return;
    const int n_heads = H / ATT_D;
    const int64_t n_pairs = (int64_t)n_docs * n_heads;
    DI_REQUIRE(n_pairs < (1ll << 31), DI_ERANGE, "attention grid too large");
    static const int abl = [] {
        const char *e = getenv("DI_ATTN_X3_ABLATE");
        return e ? atoi(e) : 0;
    }();
    // q (optional, launch_attn_order's list of this call): the launch walks a slice of the
    // documents longest first (attention_x3_kernel); without it, the documents as they come
    if (q && !q->order) q = nullptr;
    AxArgs a{qkv, cu_seqlens, H, n_heads, n_pairs, ctx_split, qsel, cu_qsel,
             q ? q->order : nullptr, q ? q->ctl + AQ_ALL : nullptr, abl, s};
    // persistent: one 8-wave workgroup per CU (64-key chunks) or two 4-wave ones (32-key)
    if (qsel) {
        // The pruned last layer (qsel: the terms' rows, ~1/5 of the queries): the 4-wave
        // form, so that a document's few query tiles keep a workgroup's waves busy
        ax_launch<4, 32>(a);
    } else if (q && q->two_forms) {
        // Full layers with a list, two forms: the documents past one 192-query pass of the
        // 4-wave form in the 8-wave kernel, the others in the 4-wave form (two workgroups
        // per CU: a SIMD that one of them leaves idle runs the other's wave); each launch
        // reads its slice from ctl and a workgroup without a unit ends at once
        a.q_range = q->ctl + AQ_LONG;
        ax_launch<8, 64>(a);
        a.q_range = q->ctl + AQ_SHORT;
        ax_launch<4, 32>(a);
    } else {
        ax_launch<8, 64>(a);
    }
}

}  // namespace di
