// enc_attn.h -- what the three attention kernels share (device side): enc_attn.hip
// (generic), enc_attn_v3.hip (persistent bf16), enc_attn_x3.hip (split bf16).
#pragma once

#include <hip/hip_runtime.h>

#include "enc_common.h"

namespace di {

constexpr int ATT_D = 64;  // head dim
// scores -> exponent of 2: 1/sqrt(64) * log2(e)
constexpr float ATT_SC = 0.125f * 1.4426950408889634f;

// doc d's first V^T column: 32-aligned (one split chunk; 16 B loads for bf16 / f32),
// at most 31 gap columns per document
__host__ __device__ __forceinline__ int vt_base(int doc, int tok0) { return 32 * (doc + (tok0 >> 5)); }

// max of x over the 4 lane groups (lanes l, l ^ 16, l ^ 32, l ^ 48): two permlane swaps
__device__ __forceinline__ float lane_group_max(float x) {
    const auto p16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x),
                                                      false, false);
    x = fmaxf(__uint_as_float(p16[0]), __uint_as_float(p16[1]));
    const auto p32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x),
                                                      false, false);
    return fmaxf(__uint_as_float(p32[0]), __uint_as_float(p32[1]));
}

}  // namespace di
