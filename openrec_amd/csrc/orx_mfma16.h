// What the bf16 matrix-core kernels share (kernels_fullsoftmax16.hip, kernels_inbatch16.hip, kernels_topk16.hip, kernels_tower16.hip): the vector types of
// v_mfma_f32_16x16x32_bf16's operands and the rounding of eight fp32 values to its 16-byte fragment.
//
// The instruction's fragments, lane = 16 q + ln:  A: row ln, k = 8 q .. 8 q + 7;  B: k = 8 q .. 8 q + 7, column ln;
// C / D: rows 4 q .. 4 q + 3 (one per register), column ln.
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight fp32 -> eight bf16, round to nearest even (v_cvt_pk_bf16_f32), as 16 bytes
__device__ __forceinline__ u32x4 fs16_pack(f32x4 lo, f32x4 hi) {
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = (__bf16)lo[j]; v[4 + j] = (__bf16)hi[j]; }
    return __builtin_bit_cast(u32x4, v);
}
