// yolo355 -- vector stores of one lane's NT consecutive output channels (bf16 / int8), shared by the
// implicit-GEMM convolutions (convg.hip, convgeom.hip).
#pragma once
#include <hip/hip_runtime.h>

template <int NT>
__device__ __forceinline__ void store_bf16(char *dst, const float (&v)[NT]) {
    unsigned short h[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) h[t] = __builtin_bit_cast(unsigned short, (__bf16)v[t]);
    if constexpr (NT == 1) {
        *(unsigned short *)dst = h[0];
    } else if constexpr (NT == 2) {
        *(unsigned int *)dst = (unsigned int)h[0] | ((unsigned int)h[1] << 16);
    } else if constexpr (NT == 4) {
        uint2 u;
        u.x = (unsigned int)h[0] | ((unsigned int)h[1] << 16);
        u.y = (unsigned int)h[2] | ((unsigned int)h[3] << 16);
        *(uint2 *)dst = u;
    } else {
        static_assert(NT == 8, "NT");
        uint4 u;
        u.x = (unsigned int)h[0] | ((unsigned int)h[1] << 16);
        u.y = (unsigned int)h[2] | ((unsigned int)h[3] << 16);
        u.z = (unsigned int)h[4] | ((unsigned int)h[5] << 16);
        u.w = (unsigned int)h[6] | ((unsigned int)h[7] << 16);
        *(uint4 *)dst = u;
    }
}

template <int NT>
__device__ __forceinline__ void store_i8(char *dst, const int (&q)[NT]) {
#pragma unroll
    for (int t0 = 0; t0 < NT; t0 += 4) {
        if constexpr (NT >= 4) {
            *(unsigned int *)(dst + t0) = (unsigned int)((q[t0] & 0xff) | ((q[t0 + 1] & 0xff) << 8) |
                                                         ((q[t0 + 2] & 0xff) << 16) | ((unsigned)(q[t0 + 3] & 0xff) << 24));
        }
    }
    if constexpr (NT == 2) *(unsigned short *)dst = (unsigned short)((q[0] & 0xff) | ((q[1] & 0xff) << 8));
    if constexpr (NT == 1) *dst = (char)q[0];
}
