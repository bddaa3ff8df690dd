// enc_launch.h -- the encoder kernels' launchers and their predicates, declared once: the
// files that define them (enc_gemm*.hip, enc_attn*.hip, enc_misc.hip, enc_pairwise.hip) and
// the files that run a forward (encoder.hip) include it.
#pragma once

#include <hip/hip_runtime.h>

#include "enc_common.h"

namespace di {

struct AttnQueue;  // enc_handle.h

// enc_gemm.hip, enc_gemm256.hip
template <typename T>
void launch_gemm(int epi, const GemmArgs &g, hipStream_t s);
bool gemm256_ok(int epi, const GemmArgs &g);
void launch_gemm256(int epi, const GemmArgs &g, hipStream_t s);
int gemm_stats_cols();

// enc_attn.hip
template <typename T>
void launch_attention(const T *qk, const T *vt, const int32_t *cu_seqlens, int n_docs,
                      int max_len, int H, int ld_v, T *ctx, hipStream_t s,
                      bf16 *ctx_split = nullptr);
void launch_vt_cols(const int32_t *cu, int n_docs, int M, int32_t *vcol, hipStream_t s);
int vt_ld(int64_t M, int n_docs);

// enc_attn_v3.hip
bool attention_v3_ok(int max_len, int H);
void launch_attention_v3(const bf16 *qkv, const int32_t *cu_seqlens, int n_docs, int max_len,
                         int H, bf16 *ctx, hipStream_t s, const int32_t *qsel = nullptr,
                         const int32_t *cu_qsel = nullptr);

// enc_attn_x3.hip
void launch_attention_x3(const bf16 *qkv, const int32_t *cu_seqlens, int n_docs, int H,
                         bf16 *ctx_split, hipStream_t s, const int32_t *qsel = nullptr,
                         const int32_t *cu_qsel = nullptr, const AttnQueue *q = nullptr);
// the knob DI_ATTN_X3_QUEUE (developer A/B): 0 no list, 1 one launch per layer, 2 two forms
int attn_queue_mode();
bool attn_order_ok(int max_positions);
void launch_attn_order(const int32_t *cu_seqlens, int n_docs, int max_positions, int32_t *order,
                       int32_t *ctl, hipStream_t s);

// enc_misc.hip
void launch_scatter_term_rows(const bf16 *Xg, const int32_t *cu_seq, const int32_t *cu_terms,
                              const int32_t *term_tok, int n_docs, int W, int64_t ld, bf16 *X,
                              hipStream_t s);
void launch_gather_term_rows(const bf16 *X, const float2 *rl, const int32_t *cu_seq,
                             const int32_t *cu_terms, const int32_t *term_tok, int n_docs, int H,
                             bf16 *Xg, float2 *rlg, hipStream_t s);
void launch_gather_terms(const float *impact, const int32_t *cu_seq, const int32_t *cu_terms,
                         int n_docs, const int32_t *term_tok, int n_terms, int do_round,
                         float *out, int32_t *err, hipStream_t s);
void launch_embed_ln_split(const int32_t *ids, const int32_t *cu, int n_docs, int M, int H,
                           const float *word, const float *pos, const float *type0,
                           const float *gamma, const float *beta, float eps, int pos_offset,
                           int vocab, int max_pos, bf16 *out, int32_t *err, hipStream_t s);
void launch_ln_split(const float *pre, int M, int H, const float *gamma, const float *beta,
                     float eps, bf16 *out, const float *head_w, float head_b, int act,
                     float *impact, hipStream_t s);
template <typename T>
void launch_embed_ln(const int32_t *ids, const int32_t *cu, int n_docs, int M, int H,
                     const T *word, const T *pos, const T *type0, const float *gamma,
                     const float *beta, float eps, int pos_offset, int vocab, int max_pos, T *out,
                     int32_t *err, hipStream_t s);
template <typename T>
void launch_ln(const T *pre, int M, int H, const float *gamma, const float *beta, float eps,
               T *out, const float *head_w, float head_b, int act, float *impact, hipStream_t s);
void launch_head_from_stats(const float4 *st, int ld, int n_part, int M, int H, float eps,
                            float sw, float cw, int act, float *impact, hipStream_t s);
void launch_row_ln(const float4 *st, int ld, int n_part, int M, int H, float eps, float2 *out,
                   hipStream_t s);

// enc_pairwise.hip
size_t pair_attn_lds_bytes(int max_len);
void launch_pair_prep(const int32_t *cu_seq, const int32_t *cu_terms, const int32_t *term_tok,
                      const int64_t *cu_pairs, int n_docs, int64_t n_terms, int64_t n_pairs,
                      int max_len, int64_t *cu_sq, int32_t *err, hipStream_t s);
void launch_pair_attn(const void *qk, bool split, const int32_t *cu_seq, const int32_t *cu_terms,
                      const int32_t *term_tok, const int64_t *cu_sq, int n_docs, int max_len,
                      int H, float *Mx, const int32_t *err, hipStream_t s);
void launch_pair_score(const void *src, int src_mode, const int32_t *cu_seq,
                       const int32_t *cu_terms, const int32_t *term_tok,
                       const int64_t *cu_pairs, const int64_t *cu_sq, int n_docs,
                       int64_t n_terms, int64_t n_pairs, int H, const float *gamma,
                       const float *beta, float eps, const float *w, float w0, float bias,
                       const float *Mx, float2 *uv, int do_round, float *out_pair,
                       float *out_attn, const int32_t *err, hipStream_t s);

}  // namespace di
