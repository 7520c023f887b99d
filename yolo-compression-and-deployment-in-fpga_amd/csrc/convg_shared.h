// yolo355 -- what the generic implicit-GEMM convolutions (convg.hip: 4 and 8 waves; convgeom.hip) share, device and host: the
// tile geometry of convg.hip, the MFMA step on 16-byte fragments, the vector stores of one lane's NT consecutive output channels
// (bf16 / int8), and the host-side B-fragment packer.
#pragma once
#include "y355_common.h"
#include <cstring>
#include <type_traits>

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

// ---- MFMA on 16-byte fragments: byte-wise the A/B fragments of the bf16 and int8 shapes are identical (lane (g, j) holds 16
// bytes of row/column j at k-offset 16 g), so one k-step serves both
template <bool BF>
using MmaAcc = typename std::conditional<BF, v4f, v4i>::type;
template <bool BF>
__device__ __forceinline__ void mma_step(MmaAcc<BF> &acc, const v4i &a, const v4i &b) {
    if constexpr (BF) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a), __builtin_bit_cast(v8bf, b), acc, 0, 0, 0);
    else acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
}

// ---- tile geometry of convg.hip, derived once for both kernels and the launcher: a TH x TW output tile (2x2 pooling windows
// in adjacent GEMM rows when POOL), BN output channels, WM x WN waves, stride S, the input patch staged in chunks of CHB bytes
// per pixel
template <int CHB, int BN, int TH, int TW, bool POOL, int WM, int WN, int S>
struct ConvGTile {
    static constexpr bool THIN = (CHB == 32);           // 32 B per pixel: a k-step covers two taps
    // input patch of a TH x TW output tile: S*(T-1)+3 pixels a side (stride S, 3x3, pad 1)
    static constexpr int PW = S * (TW - 1) + 3, PH = S * (TH - 1) + 3, NPIX = PH * PW;
    static constexpr int STRIDE = CHB + 16;             // 16-byte pad: conflict-free ds_read_b128 across pixels
    static constexpr int CPP = CHB / 16;
    static constexpr int SUB = THIN ? 1 : CHB / 64;     // k-steps per tap and chunk
    static constexpr int BM = TH * TW;
    static constexpr int MT = ((BM + 15) / 16 + WM - 1) / WM;
    static constexpr int NT = BN / 16 / WN;
    static constexpr int SLAB = (NPIX * STRIDE + 15) / 16 * 16;     // LDS bytes of one staged chunk
    static_assert(S == 1 || (S == 2 && !POOL && !THIN), "stride 2: plain 64-byte-chunk tiles only");
    static_assert(!POOL || (TH % 2 == 0 && TW % 2 == 0), "pooled tiles are even");
};

// The k-steps of one staged chunk of tile T, in B-fragment order: kstep(ko) with the slab byte offset of the step's tap and
// 64-byte sub-chunk -- THIN: five steps of two taps (the lane's kofs); else per sub-chunk the nine taps, or the centre tap alone
// (1x1).  USUB: unroll count of the loop over sub-chunks.  A macro, not a function that takes the k-step as a callable: through
// one the kernels' instructions change (cross-compiled: the 8-wave pooled 26x26 tiles double their scratch)
#define CONVG_PRAGMA(x) _Pragma(#x)
#define CONVG_WALK_CHUNK(T, USUB, taps, kofs, kstep)                                                                    \
    if constexpr (T::THIN) {                                                                                            \
        CONVG_PRAGMA(unroll)                                                                                            \
        for (int ks = 0; ks < 5; ++ks) kstep(kofs[ks]);                                                                 \
    } else {                                                                                                            \
        CONVG_PRAGMA(unroll USUB)                                                                                       \
        for (int sub = 0; sub < T::SUB; ++sub) {                                                                        \
            if (taps == 9) {                                                                                            \
                CONVG_PRAGMA(unroll)                                                                                    \
                for (int tap = 0; tap < 9; ++tap) kstep(((tap / 3) * T::PW + tap % 3) * T::STRIDE + sub * 64);          \
            } else {                                                                                                    \
                kstep((T::PW + 1) * T::STRIDE + sub * 64);                                                              \
            }                                                                                                           \
        }                                                                                                               \
    }

// ---- host: B fragments.  frag(nb, ks, wn, t), lane (g, j) holds the 16 bytes at k-offset 16 g of output channel
// n = nb*BN + wn*NT*16 + j*NT + t.  rule(ks, k, tap, ci): the tap and input channel of element k (of 64 int8 or 32 bf16) of
// k-step ks.  `w` is [cout][cin][taps], fp32 (bf16 nets: rounded to nearest-even here) or int8; what lies outside it is zero
template <class Rule>
void y355_pack_bfrags(bool bf, int KS, int BN, int WN, int NT, const float *w_f, const int8_t *w_q, int cout, int cin, int taps,
                      int cout_pad, char *dst, Rule rule) {
    const int es = bf ? 2 : 1, epg = 16 / es;          // element size, elements per lane
    for (int nb = 0; nb < cout_pad / BN; ++nb)
        for (int ks = 0; ks < KS; ++ks)
            for (int wn = 0; wn < WN; ++wn)
                for (int t = 0; t < NT; ++t) {
                    char *f = dst + ((((size_t)nb * KS + ks) * WN + wn) * NT + t) * 1024;
                    for (int l = 0; l < 64; ++l) {
                        const int g = l >> 4, j = l & 15;
                        const int n = nb * BN + wn * NT * 16 + j * NT + t;
                        for (int e = 0; e < epg; ++e) {
                            int tap, ci;
                            rule(ks, g * epg + e, tap, ci);
                            const bool ok = tap < taps && n < cout && ci < cin;
                            const size_t wi = ((size_t)n * cin + ci) * taps + tap;
                            if (bf) {
                                const unsigned short h = y355_bf16_rne(ok ? w_f[wi] : 0.f);
                                memcpy(f + l * 16 + e * 2, &h, 2);
                            } else {
                                f[l * 16 + e] = ok ? (char)w_q[wi] : 0;
                            }
                        }
                    }
                }
}
