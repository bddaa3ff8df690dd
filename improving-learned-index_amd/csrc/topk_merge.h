// topk_merge.h -- the top-k merge of per-list candidates by 64-bit key (topk_merge.hip),
// launched by the quantized index (index.hip), the float index (sparse.hip) and
// di_topk_merge.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace di {

// What the merge writes besides the keys: doc and score decoded from a quantized key
// (wide keys for the queries of more than DI_SHORT_QUERY_TERMS terms, by cu_q), from a
// float-index key, or nothing.
enum DecodeMode : int { DECODE_QUANT = 0, DECODE_SPARSE = 1, DECODE_NONE = 2 };

// Per query, the k largest of n_lists lists of up to k_in keys each; list l of query q at
// keys[(q * n_lists + l) * k_in] with its length at counts[q * n_lists + l], or with
// lists_major at keys[(l * n_q + q) * k_in] / counts[l * n_q + q].  Sets the kernels'
// dynamic-LDS limits itself, once per process and device.
void launch_merge(const uint64_t *keys, const int32_t *counts, int n_q, int n_lists, int k_in,
                  int k, uint64_t *out_key, uint32_t *out_doc, uint32_t *out_score,
                  int32_t *out_n, int mode, hipStream_t s, bool lists_major = false,
                  const int32_t *cu_q = nullptr);

}  // namespace di
