// enc_pairwise.hip -- the pairwise impact head of DeepPairwiseImpact on the encoder's
// workspace, gfx950.
//
// Replaces, for a packed batch, the reference's
//   get_pairwise_impact_scores    src/deep_impact/models/pairwise_impact.py:44-95
// with pairwise_indices = combinations(sorted(map_.values()), 2) per document (the
// commented block of src/deep_impact/indexing/indexer.py:49-54).  For the pair of term
// rows (a, b), a < b in token order:
//   attn(a,b)  = max over layers of max(mean_h P[h,a,b], mean_h P[h,b,a])   (:62-68)
//   score(a,b) = relu(w[0] attn + w[1:H+1] h_a + w[H+1:2H+1] h_b + bias)    (:72-87)
// The attention kernels never write the probabilities P; pair_attn_kernel computes them
// again for the query rows of the kept terms only, from the Q and K the layer's QKV
// projection left in the workspace: a T x n score panel per (document, layer, head),
// its row maximum and sum, and the T x T block at the terms' columns.  The mean over
// heads is folded into a per-document running maximum Mx[a][b] over the layers (each
// direction on its own: direction and layer maxima commute, pair_score_kernel takes
// max(Mx[a][b], Mx[b][a])).  The two halves of the head's dot product are per-row
// values u = LN(x) w[1:H+1], v = LN(x) w[H+1:2H+1] (pair_uv_kernel), so a pair costs
// two loads and three adds.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "di_common.h"
#include "enc_common.h"
#include "enc_launch.h"

namespace di {

namespace {

constexpr int PA_WAVES = 4, PA_THREADS = 64 * PA_WAVES;
constexpr int PA_ROWS = 16;  // term rows of one workgroup (one MFMA tile)
constexpr int PA_D = 64;     // head dim

// error bits of the encoder's err word (1, 2: di_encode's)
constexpr int ERR_TERMS = 4, ERR_PAIRS = 8;

// row stride of the score panel: n rounded up to the 16-key tile, plus 4 so that the four
// rows 4g + r a wave stores at once fall on different banks
__host__ __device__ __forceinline__ int pa_ld(int n) { return ((n + 15) & ~15) + 4; }
__host__ __device__ __forceinline__ size_t pa_lds_floats(int n, int T) {
    return (size_t)PA_ROWS * pa_ld(n) + (size_t)PA_ROWS * T + (size_t)T;
}

// Operand loaders: 4 consecutive logical columns of a Q or K row as f32.
struct LoadF32 {  // the fp32 forward: qk [M][2H], Q | K row-major
    const float *p;
    int H;
    __device__ __forceinline__ f32x4 q(int64_t row, int col) const {
        return *reinterpret_cast<const f32x4 *>(p + row * 2 * H + col);
    }
    __device__ __forceinline__ f32x4 k(int64_t row, int col) const {
        return *reinterpret_cast<const f32x4 *>(p + row * 2 * H + H + col);
    }
};
struct LoadSplit {  // bf16x3 forwards: split rows [M][6H], hi + lo exact in f32
    const bf16 *p;
    int H;
    __device__ __forceinline__ f32x4 at(int64_t row, int col) const {
        const bf16 *x = p + row * 6 * H + split_col(col);
        const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(x);
        const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(x + 32);
        return f32x4{(float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1],
                     (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]};
    }
    __device__ __forceinline__ f32x4 q(int64_t row, int col) const { return at(row, col); }
    __device__ __forceinline__ f32x4 k(int64_t row, int col) const { return at(row, H + col); }
};

// Checks the term and pair arrays and lays out Mx: cu_sq[d] = sum of T^2 of the documents
// before d.  One workgroup; thread t owns a contiguous run of documents.  A violation
// sets an error bit, and the pair kernels then do nothing.
__global__ void __launch_bounds__(256)
pair_prep_kernel(const int32_t *__restrict__ cu_seq, const int32_t *__restrict__ cu_terms,
                 const int32_t *__restrict__ term_tok, const int64_t *__restrict__ cu_pairs,
                 int n_docs, int64_t n_terms, int64_t n_pairs, int max_len,
                 int64_t *__restrict__ cu_sq, int32_t *__restrict__ err) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int d0 = (int)((int64_t)n_docs * t / 256), d1 = (int)((int64_t)n_docs * (t + 1) / 256);
    int bad = 0;
    if (t == 0) {
        if (cu_terms[0] != 0 || cu_terms[n_docs] != n_terms) bad |= ERR_TERMS;
        if (cu_pairs[0] != 0 || cu_pairs[n_docs] != n_pairs) bad |= ERR_PAIRS;
    }
    int64_t sum = 0;
    for (int d = d0; d < d1; ++d) {
        const int a = cu_terms[d], b = cu_terms[d + 1];
        const int len = cu_seq[d + 1] - cu_seq[d];
        const int64_t T = (int64_t)b - a;
        if (a < 0 || T < 0 || T > len || len > max_len || b > n_terms) {
            bad |= ERR_TERMS;
            continue;
        }
        int prev = -1;
        for (int i = a; i < b; ++i) {  // strictly ascending, inside the document
            const int tok = term_tok[i];
            if (tok <= prev || tok >= len) bad |= ERR_TERMS;
            prev = tok;
        }
        if (cu_pairs[d + 1] - cu_pairs[d] != T * (T - 1) / 2) bad |= ERR_PAIRS;
        sum += T * T;
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        cu_sq[n_docs] = run;
    }
    __syncthreads();
    int64_t run = part[t];
    for (int d = d0; d < d1; ++d) {
        cu_sq[d] = run;
        const int64_t T = (int64_t)cu_terms[d + 1] - cu_terms[d];
        const int len = cu_seq[d + 1] - cu_seq[d];
        if (T >= 0 && T <= len && len <= max_len) run += T * T;
    }
    if (bad) atomicOr(err, bad);
}

// One workgroup per (document, 16-row tile of its term rows); the heads in order.
//   1. S = Q_R K^T over all n keys (v_mfma_f32_16x16x4_f32; A = the term rows' Q, B = K
//      rows: lane (g, c) holds S[4g + r][16 kt + c]), scaled by log2(e) / 8, into LDS
//   2. row maximum m and sum l of 2^(S - m): 16 lanes per row (raw v_exp_f32: the
//      arguments are <= 0, and a probability below 2^-126 is 0)
//   3. P at the T term columns, 2^(S - m) / l, added to the head sum in LDS
// and after the last head Mx = max(Mx, sum / heads).  The workgroup owns its rows of Mx,
// so the read-max-write across the layers (launches in stream order) needs no atomics.
// Every sum runs in a fixed order that depends on the document alone.
template <class LD>
__global__ void __launch_bounds__(PA_THREADS)
pair_attn_kernel(LD ld, const int32_t *__restrict__ cu_seq, const int32_t *__restrict__ cu_terms,
                 const int32_t *__restrict__ term_tok, const int64_t *__restrict__ cu_sq,
                 int n_docs, int n_tiles, int n_heads, int max_len, float *__restrict__ Mx,
                 const int32_t *__restrict__ err) {
    extern __shared__ float lds[];
    if (*err & (ERR_TERMS | ERR_PAIRS)) return;
    // 1-D grid, XCD-grouped (speed only, as attention_kernel): the tiles of one document
    // are ids j * 8 + x for one run of j -- all on XCD x under round-robin dispatch and
    // next to each other in time -- so they share the document's K through that L2
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int doc = (j / n_tiles) * 8 + x, tile = j % n_tiles;
    if (doc >= n_docs) return;
    const int t0 = cu_terms[doc], T = cu_terms[doc + 1] - t0;
    if (tile * PA_ROWS >= T) return;
    const int tok0 = cu_seq[doc], n = cu_seq[doc + 1] - tok0;
    if (n > max_len) return;  // (the LDS panel is sized for max_len keys)
    const int ldS = pa_ld(n);
    float *S = lds;                                        // [16][ldS]
    float *acc = S + PA_ROWS * ldS;                        // [16][T] head sums
    int *tcol = reinterpret_cast<int *>(acc + PA_ROWS * T);  // [T] the terms' token index
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    for (int i = tid; i < PA_ROWS * T; i += PA_THREADS) acc[i] = 0.f;
    for (int i = tid; i < T; i += PA_THREADS) tcol[i] = min(max(term_tok[t0 + i], 0), n - 1);
    // this lane's query row of the A operand (rows past T repeat the last term)
    const int64_t qrow = tok0 + min(max(term_tok[t0 + min(tile * PA_ROWS + c, T - 1)], 0), n - 1);
    const float sc = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e)
    const int n_kt = (n + 15) >> 4;
    const int row = tid >> 4, sub = tid & 15;  // softmax phase: 16 lanes per row
    __syncthreads();
    for (int h = 0; h < n_heads; ++h) {
        f32x4 qf[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) qf[ch] = ld.q(qrow, h * PA_D + ch * 16 + 4 * g);
        for (int kt = wave; kt < n_kt; kt += PA_WAVES) {
            const int key = kt * 16 + c;
            const int64_t krow = tok0 + min(key, n - 1);
            f32x4 kf[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) kf[ch] = ld.k(krow, h * PA_D + ch * 16 + 4 * g);
            // two independent accumulation chains over the head dim (0..31, 32..63)
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[ch][i], kf[ch][i], s, 0, 0, 0);
                    s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[ch + 2][i], kf[ch + 2][i], s1, 0,
                                                              0, 0);
                }
            s += s1;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                S[(4 * g + r) * ldS + key] = key < n ? s[r] * sc : -INFINITY;
        }
        __syncthreads();
        const float *Sr = S + row * ldS;
        float m = -INFINITY;
        for (int k = sub; k < n; k += 16) m = fmaxf(m, Sr[k]);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float l = 0.f;
        for (int k = sub; k < n; k += 16) l += __builtin_amdgcn_exp2f(Sr[k] - m);
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) l += __shfl_xor(l, o, 64);
        const float inv = 1.0f / l;
        for (int b = sub; b < T; b += 16)
            acc[row * T + b] += __builtin_amdgcn_exp2f(Sr[tcol[b]] - m) * inv;
        __syncthreads();
    }
    const int a = tile * PA_ROWS + row;
    if (a < T) {
        float *mx = Mx + cu_sq[doc] + (int64_t)a * T;
        const float inv_h = 1.0f / (float)n_heads;
        for (int b = sub; b < T; b += 16) mx[b] = fmaxf(mx[b], acc[row * T + b] * inv_h);
    }
}

__device__ __forceinline__ int find_seg32(const int32_t *cu, int n, int64_t i) {
    int lo = 0, hi = n;  // last d with cu[d] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int find_seg64(const int64_t *cu, int n, int64_t i) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// One wave per kept term row: the last LayerNorm of its pre-LayerNorm row in f32 (two
// passes: mean, then the centred sum of squares) and the two dot products with the pair
// head's halves.  src_mode 0: f32 rows at the terms' token rows (fp32 forward); 1: f32
// rows packed in term order (bf16x3, unfolded); 2: split rows packed in term order,
// x = hi + lo (bf16x3, folded: the pruned last layer's FFN output).
__global__ void __launch_bounds__(256)
pair_uv_kernel(const void *__restrict__ src, int src_mode, const int32_t *__restrict__ cu_seq,
               const int32_t *__restrict__ cu_terms, const int32_t *__restrict__ term_tok,
               int n_docs, int64_t n_terms, int H, const float *__restrict__ gamma,
               const float *__restrict__ beta, float eps, const float *__restrict__ w,
               float2 *__restrict__ uv, const int32_t *__restrict__ err) {
    if (*err & (ERR_TERMS | ERR_PAIRS)) return;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_terms) return;
    int64_t r = i;
    if (src_mode == 0) r = cu_seq[find_seg32(cu_terms, n_docs, i)] + term_tok[i];
    float x[16];  // H <= 1024
    const int nk = H / 64;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        x[j] = 0.f;
        if (j < nk) {
            const int k = j * 64 + lane;
            if (src_mode == 2) {
                const bf16 *p = static_cast<const bf16 *>(src) + r * 2 * H + split_col(k);
                x[j] = (float)p[0] + (float)p[32];
            } else {
                x[j] = static_cast<const float *>(src)[r * H + k];
            }
            sum += x[j];
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum / (float)H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < nk) sq += (x[j] - mean) * (x[j] - mean);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sq += __shfl_xor(sq, o, 64);
    const float rstd = 1.0f / sqrtf(sq / (float)H + eps);
    float u = 0.f, v = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < nk) {
            const int k = j * 64 + lane;
            const float y = (x[j] - mean) * rstd * gamma[k] + beta[k];
            u += y * w[1 + k];
            v += y * w[1 + H + k];
        }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u += __shfl_xor(u, o, 64);
        v += __shfl_xor(v, o, 64);
    }
    if (lane == 0) uv[i] = make_float2(u, v);
}

// numpy's round(np.float32, 3), as enc_misc.hip's gather
__device__ __forceinline__ float pair_round3(float x) {
    return __fdiv_rn(rintf(__fmul_rn(x, 1000.0f)), 1000.0f);
}

// One thread per pair: j = a (2T - a - 1) / 2 + (b - a - 1) within its document.
__global__ void __launch_bounds__(256)
pair_score_kernel(const int32_t *__restrict__ cu_terms, const int64_t *__restrict__ cu_pairs,
                  const int64_t *__restrict__ cu_sq, int n_docs, int64_t n_pairs,
                  const float *__restrict__ Mx, const float2 *__restrict__ uv, float w0,
                  float bias, int do_round, float *__restrict__ out_pair,
                  float *__restrict__ out_attn, const int32_t *__restrict__ err) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    if (*err & (ERR_TERMS | ERR_PAIRS)) {
        out_pair[p] = 0.f;
        if (out_attn) out_attn[p] = 0.f;
        return;
    }
    const int d = find_seg64(cu_pairs, n_docs, p);
    const int64_t j = p - cu_pairs[d];
    const int t0 = cu_terms[d];
    const int64_t T = cu_terms[d + 1] - t0;
    auto first = [&](int64_t a) { return a * (2 * T - a - 1) / 2; };  // index of pair (a, a+1)
    const double s = (double)(2 * T - 1);
    int64_t a = (int64_t)((s - sqrt(s * s - 8.0 * (double)j)) * 0.5);
    a = min(max(a, (int64_t)0), T - 2);
    while (a > 0 && first(a) > j) --a;
    while (a < T - 2 && first(a + 1) <= j) ++a;
    const int64_t b = a + 1 + (j - first(a));
    const float *mx = Mx + cu_sq[d];
    const float attn = fmaxf(mx[a * T + b], mx[b * T + a]);
    const float z = ((w0 * attn + uv[t0 + a].x) + uv[t0 + b].y) + bias;
    const float y = fmaxf(z, 0.f);
    out_pair[p] = do_round ? pair_round3(y) : y;
    if (out_attn) out_attn[p] = attn;
}

}  // namespace

// LDS bytes of pair_attn_kernel for documents of up to max_len tokens (T <= n)
size_t pair_attn_lds_bytes(int max_len) { return pa_lds_floats(max_len, max_len) * 4; }

void launch_pair_prep(const int32_t *cu_seq, const int32_t *cu_terms, const int32_t *term_tok,
                      const int64_t *cu_pairs, int n_docs, int64_t n_terms, int64_t n_pairs,
                      int max_len, int64_t *cu_sq, int32_t *err, hipStream_t s) {
    hipLaunchKernelGGL(pair_prep_kernel, dim3(1), dim3(256), 0, s, cu_seq, cu_terms, term_tok,
                       cu_pairs, n_docs, n_terms, n_pairs, max_len, cu_sq, err);
    check_launch("pair_prep");
}

// qk: the layer's Q | K (| V) rows -- f32 [M][2H] (split = false) or split rows [M][6H]
void launch_pair_attn(const void *qk, bool split, const int32_t *cu_seq, const int32_t *cu_terms,
                      const int32_t *term_tok, const int64_t *cu_sq, int n_docs, int max_len,
                      int H, float *Mx, const int32_t *err, hipStream_t s) {
    if (n_docs <= 0 || max_len <= 0) return;
    const size_t lds = pair_attn_lds_bytes(max_len);
    const int n_tiles = (max_len + PA_ROWS - 1) / PA_ROWS;  // (tiles past a document's T exit)
    const dim3 grid((unsigned)((n_docs + 7) / 8 * 8 * n_tiles));
    if (split) {
        auto k = pair_attn_kernel<LoadSplit>;
        DI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, grid, dim3(PA_THREADS), lds, s,
                           LoadSplit{static_cast<const bf16 *>(qk), H}, cu_seq, cu_terms, term_tok,
                           cu_sq, n_docs, n_tiles, H / PA_D, max_len, Mx, err);
    } else {
        auto k = pair_attn_kernel<LoadF32>;
        DI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, grid, dim3(PA_THREADS), lds, s,
                           LoadF32{static_cast<const float *>(qk), H}, cu_seq, cu_terms, term_tok,
                           cu_sq, n_docs, n_tiles, H / PA_D, max_len, Mx, err);
    }
    check_launch("pair_attn");
}

void launch_pair_score(const void *src, int src_mode, const int32_t *cu_seq,
                       const int32_t *cu_terms, const int32_t *term_tok,
                       const int64_t *cu_pairs, const int64_t *cu_sq, int n_docs,
                       int64_t n_terms, int64_t n_pairs, int H, const float *gamma,
                       const float *beta, float eps, const float *w, float w0, float bias,
                       const float *Mx, float2 *uv, int do_round, float *out_pair,
                       float *out_attn, const int32_t *err, hipStream_t s) {
    if (n_pairs <= 0) return;
    hipLaunchKernelGGL(pair_uv_kernel, dim3((unsigned)((n_terms + 3) / 4)), dim3(256), 0, s, src,
                       src_mode, cu_seq, cu_terms, term_tok, n_docs, n_terms, H, gamma, beta, eps,
                       w, uv, err);
    check_launch("pair_uv");
    hipLaunchKernelGGL(pair_score_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s,
                       cu_terms, cu_pairs, cu_sq, n_docs, n_pairs, Mx, uv, w0, bias, do_round,
                       out_pair, out_attn, err);
    check_launch("pair_score");
}

}  // namespace di
