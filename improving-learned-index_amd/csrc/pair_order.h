// pair_order.h -- the device ordering of DeepPairwiseImpact's entries (pair_order.hip),
// shared by di_pairwise_order and di_encode_pairwise_entries (encoder.hip).
#pragma once

#include "di_common.h"

namespace di {

// Scratch of one ordering call (the standalone call's own, or the encoder's workspace).
struct PairOrderWs {
    DevBuf cnt;         // entries per document (int32)
    DevBuf info;        // PO_INFO totals of the scan (int64)
    DevBuf ldoc, loff;  // the large-route documents and their key / run / tile offsets
    DevBuf keyA, keyB;  // the large route's ping-pong key buffers
    DevBuf err;
    DevBuf o_cu, o_first, o_second, o_score;  // device side of host outputs
    void reserve_docs(int n_docs);
};

// single / pair / cu_terms / cu_pairs / single_pos (may be null): device pointers.
// out_*: device pointers when out_dev, else host pointers (copied before returning).
// Waits for the stream (once for the sizes, once at the end).  timer may be null.
void pairwise_order_run(PairOrderWs &ws, Timer *timer, bool timing, const float *single,
                        const float *pair, const int32_t *cu_terms, const int64_t *cu_pairs,
                        const int32_t *single_pos, int n_docs, int64_t n_terms, int64_t n_pairs,
                        int64_t *out_cu, int32_t *out_first, int32_t *out_second,
                        float *out_score, int64_t out_cap, int64_t *n_out, bool out_dev,
                        bool round3, hipStream_t s);

}  // namespace di
