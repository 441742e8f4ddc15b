// What the tower's fp32 and bf16 kernels share on the device (kernels_tower.hip, kernels_tower16.hip)
#pragma once

// round(round(a b) + c): the l2 term as fs_finish_kernel's fmaf(scale, s, l2 x) rounds it at scale 1 -- the product once, then the sum
__device__ __forceinline__ float tw_l2_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return c + p;
}
