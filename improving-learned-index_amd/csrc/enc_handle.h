// enc_handle.h -- the encoder handle (weights + workspace of one device), shared by the
// files that run a forward on it: encoder.hip (di_encode) and cross.hip (di_encode_pairs).
#pragma once

#include <memory>
#include <vector>

#include "di_common.h"
#include "pair_order.h"

namespace di {

struct Layer {
    DevBuf w_qkv, b_qkv, w_o, b_o, ln1_g, ln1_b, w_i, b_i, w_out, b_out, ln2_g, ln2_b;
    DevBuf s_qkv, c_qkv, s_i, c_i;  // LN folding: per-column s = W' 1, c = b + W beta
};

// One di_encode_pairwise call in flight: what the forwards hand to pair_attn_kernel after
// each layer's QKV projection (di_encoder::pair_run, null outside such a call).
struct PairRun {
    const int32_t *tt, *ct;  // term_tok, cu_terms (device)
    const int64_t *cu_sq;    // Mx offset of every document
    int max_len;
};

// The attention's unit order of one encode call (launch_attn_order): the documents sorted
// by token count, longest first, and the slices of that list its launches walk.  ctl =
// {0, n_long, n_docs, 0, n_docs}: documents [0, n_long) are longer than AQ_LONG_LEN tokens.
// order == nullptr: no list, the launches walk the documents as they come.
struct AttnQueue {
    const int32_t *order = nullptr;  // [n_docs] (device)
    const int32_t *ctl = nullptr;    // [AQ_CTL] (device)
    bool two_forms = false;          // full layers: long and short documents in two launches
};
constexpr int AQ_CTL = 5, AQ_LONG = 0, AQ_SHORT = 1, AQ_ALL = 3;  // ctl index of a slice's [lo, hi)
constexpr int AQ_LONG_LEN = 192;  // one pass of the 4-wave form

}  // namespace di

struct di_encoder {
    di_encoder_cfg cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    size_t esz = 2;  // bytes per activation/weight element (bf16 or f32)
    // fp32-faithful split-bf16 mode (DI_PREC_BF16X3): esz = 4 sizes the workspace (a
    // split row of 2H bf16 = an f32 row), f32 tables, GEMM weights [N][3K] bf16
    bool split = false;
    di::DevBuf word, pos, type0, emb_g, emb_b, head_w;
    float head_b = 0.f;
    std::vector<std::unique_ptr<di::Layer>> layers;
    // workspace
    di::DevBuf X, qk, vt, vcol, ctx, pre, X1, Hff, impact, ids, cu, tt, cut, err;
    // LayerNorm folding (bf16): the GEMM consuming LN(x) reads x and folds LN in
    bool folded = false;
    di::DevBuf stats1, stats2, head_wg;  // row-statistics partials; w * gamma_last
    di::DevBuf rln1, rln2;               // per-row (rstd, -rstd mean) of P1 / P2
    float head_sw = 0.f, head_cw = 0.f;
    int64_t cap_tokens = 0;
    int64_t cap_rows = 0;  // allocated rows of the GEMM A operands (>= cap_tokens)
    int cap_docs = 0;
    int ld_v = 0;
    // pairwise head (pairwise_impact_score_encoder, optional): w [2H+1] f32 on the device,
    // w[0] and the bias on the host; Mx = running maximum of the head-mean probabilities,
    // T x T per document; uv = the head's two dot products per kept row
    bool has_pair = false;
    di::DevBuf pair_w, Mx, uv, cu_sq, cup;
    float pair_w0 = 0.f, pair_b = 0.f;
    const di::PairRun *pair_run = nullptr;
    // di_encode_pairwise_entries: the unrounded singles and pairs, single_pos, and the
    // ordering's scratch
    di::DevBuf ent_single, ent_pair, ent_pos;
    di::PairOrderWs order;
    di::DevBuf aq_order, aq_ctl;  // bf16x3: the attention's unit order of the call in flight
    di::AttnQueue aq;
    di::DevBuf pinfo;  // di_encode_pairs: (n_tokens, max_len, error bits) of the pack
    di::Timer timer;
};

namespace di {

// Grows the workspace to M tokens / n_docs documents / n_terms kept rows (never shrinks).
void ensure_workspace(di_encoder *e, int64_t M, int n_docs, int64_t n_terms);

}  // namespace di
