// yolo355 -- device primitives the hand-scheduled convolution kernels share (gfx950 only): the LDS-DMA wrapper, the counted
// s_waitcnt vmcnt forms, bare max / min instructions, the SDWA max-into-byte, the byte and bf16 packs.  One copy each; the
// kernels pull them in with `using namespace y355dev`.
#pragma once
#include "y355_common.h"

namespace y355dev {
// fp32 epilogue on exact integers: 1.5 * 2^23 and the clamp bounds MAGIC -+ 127 around it
constexpr float MAGIC = 12582912.0f;
constexpr float QLO = 12582785.0f, QHI = 12583039.0f;

// LDS-DMA: 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4), counted by vmcnt
__device__ __forceinline__ void glds16(const void *g, void *lds) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                     (__attribute__((address_space(3))) void *)lds, 16, 0, 0);
}

// s_waitcnt vmcnt(N), N a compile-time constant (the counter has six bits)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0, "vmcnt");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N > 63 ? 63 : N) : "memory");
}
// s_waitcnt needs an immediate: a table of the waits 0 .. MAX for a wave-uniform n; anything outside it (the -1 that
// convpx / convpxb pass on purpose included) waits for everything.  The table size is the caller's: it bounds the switch
// the compiler emits where n is not a constant.
template <int MAX>
__device__ __forceinline__ void wait_vmcnt_upto(int n) {
    static_assert(MAX >= 0 && MAX <= 63, "vmcnt has six bits");
#define Y355_W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n < 0 || n > MAX ? -1 : n) {
        Y355_W(0) Y355_W(1) Y355_W(2) Y355_W(3) Y355_W(4) Y355_W(5) Y355_W(6) Y355_W(7)
        Y355_W(8) Y355_W(9) Y355_W(10) Y355_W(11) Y355_W(12) Y355_W(13) Y355_W(14) Y355_W(15)
        Y355_W(16) Y355_W(17) Y355_W(18) Y355_W(19) Y355_W(20) Y355_W(21) Y355_W(22) Y355_W(23)
        Y355_W(24) Y355_W(25) Y355_W(26) Y355_W(27) Y355_W(28) Y355_W(29) Y355_W(30) Y355_W(31)
        Y355_W(32) Y355_W(33) Y355_W(34) Y355_W(35) Y355_W(36) Y355_W(37) Y355_W(38) Y355_W(39)
        Y355_W(40) Y355_W(41) Y355_W(42) Y355_W(43) Y355_W(44) Y355_W(45) Y355_W(46) Y355_W(47)
        Y355_W(48) Y355_W(49) Y355_W(50) Y355_W(51) Y355_W(52) Y355_W(53) Y355_W(54) Y355_W(55)
        Y355_W(56) Y355_W(57) Y355_W(58) Y355_W(59) Y355_W(60) Y355_W(61) Y355_W(62) Y355_W(63)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
#undef Y355_W
}
// the ring kernels' form: n clamped into 0 .. 63; their callers pass values that are constants after unrolling, so the table
// folds to one instruction
__device__ __forceinline__ void wait_vmcnt_clamped(int n) { wait_vmcnt_upto<63>(n < 0 ? 0 : (n > 63 ? 63 : n)); }

// LDS reads and writes retired, then the workgroup barrier
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// bare instructions: hipcc canonicalises (quiets) both operands of fmaxf / fminf chains and turns `m >= 0 ? m : m * s` into
// a compare + select (v_cndmask on vcc: 22 cycles back to back, profiles/r04_notes.md section 9)
__device__ __forceinline__ float vmax(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float d;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// byte B of w = bits [7:0] of max(a, b), the other bytes kept (B = 0: zeroed): the LeakyReLU's max and the int8 pack in one
// SDWA instruction per output (the same issue cost as the plain v_max_f32)
template <int B>
__device__ __forceinline__ void max_to_byte(unsigned int &w, float a, float b) {
    if constexpr (B == 0)
        asm("v_max_f32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:DWORD" : "=v"(w) : "v"(a), "v"(b));
    else if constexpr (B == 1)
        asm("v_max_f32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(w) : "v"(a), "v"(b));
    else if constexpr (B == 2)
        asm("v_max_f32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(w) : "v"(a), "v"(b));
    else
        asm("v_max_f32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(w) : "v"(a), "v"(b));
}
// bytes 0 of four registers (floats MAGIC + q) -> one dword
__device__ __forceinline__ unsigned int pack4(float a, float b, float c, float d) {
    const unsigned int ab = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x0c0c0400u);
    const unsigned int cd = __builtin_amdgcn_perm(__float_as_uint(d), __float_as_uint(c), 0x04000c0cu);
    return ab | cd;
}
// (a, b) -> two bf16 (RNE), a in the low half
__device__ __forceinline__ unsigned int pk_bf16(float a, float b) {
    typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
    const v2bf v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned int, v);
}
// lane i of each row of 16 lanes receives lane i + 1's value (lane 15: zero)
__device__ __forceinline__ unsigned int row_next(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x101 /* row_shl:1 */, 0xf, 0xf, true);
}

// Slab pieces the ring kernels (conv3x3_ring.hip, convr.hip) issue in steps lo..hi: step u issues one when
// 1 <= (u mod 9) <= ppw; negative steps are the previous tile's (none before the first tile: its slab went out whole in the
// prologue).  Their counted waits are sums of this.
constexpr int ring_sp(int lo, int hi, int ppw, bool prev) {
    int n = 0;
    for (int u = lo; u <= hi; ++u) {
        if (u < 0 && !prev) continue;
        const int t = ((u % 9) + 9) % 9;
        if (t >= 1 && t <= ppw) ++n;
    }
    return n;
}
}  // namespace y355dev
