// yolo355 -- the fp32 form of the int8 epilogue for a lane's four outputs: front.hip and both roles of
// pxpair.hip.  convpx.hip takes only epi_word_hot and keeps its own copy of the constants, the pair arithmetic and the
// clamped, counting word in its `finish` (the shared forms changed its register allocation): A CHANGE TO epi_scales, epi_ops,
// epi_pair OR epi_word_clamped MUST BE MADE THERE TOO.  (conv3x3_ring.hip's FPE path builds its scales from exponent bits,
// has neg = pos / 8 and keeps its own arithmetic on y355_dev.h's primitives.)
//
// With t = (acc << shl) + bias exact in fp32 (|t| < 2^24: y355_fp32_exact, y355_common.h) and M = MAGIC = 1.5 * 2^23,
//     q = low byte of med3(max(fma(t, s_pos, M), fma(t, s_neg, M)), M - 127, M + 127),   s_pos = 2^(lk - sh), s_neg = neg_mul * 2^-sh
// is RNE(t' * 2^-sh) clamped, bit for bit the integer pipeline of DESIGN.md section 2: the fma rounds the exact product
// once, to the integer grid of [2^23, 2^24), ties to even.
//   * The two fma are the two branches of the LeakyReLU, each M + rne(t * scale), and y = max(pos, neg): RNE is monotone, so
//     round(max) = max(round).
//   * 0 <= s_neg <= s_pos (y355_fp32_slope_ok): t >= 0 -> pos >= neg >= M, t < 0 -> pos <= neg <= M, so
//     y > M + 127 <=> pos > M + 127  and  y < M - 127 <=> neg < M - 127.  The hot passes therefore do not clamp: they take the
//     low bytes of the unclamped maxima (one SDWA max per output) and track the branches' extremes ymx / ymn, two
//     instructions per four outputs each; when those leave [QLO, QHI] (rare) the caller redoes the wave's share with the
//     clamped word, which also counts.
//   * FOLD (y355_fp32_fold) says where the bias and the conversion happen:
//       0  accumulator shift != 0: v_cvt, then fma(acc, 2^shl, bias);
//       1  shift 0: the bias rides in as the MFMAs' C operand, one v_cvt;
//       2  shift 0, |t| < 2^22, sh <= 22, sh - lk >= -8: the C operand is bias + 0x4B400000, so the int32 accumulator IS the
//          bit pattern of the float M + t (no v_cvt), and M + t * s = fma(M + t, s, M * (1 - s)) exactly (M * (1 - s) is
//          representable for 2^-22 <= s <= 2^8).
//   * The scales and addends are VGPR operands on purpose: an SGPR source takes a vector instruction off the fast issue path
//     (scratch/ubench/valu_rates.hip: v_fma_f32 3.0 cycles per SIMD with VGPR sources, 4.6 with one SGPR source).
// Host rules (y355_common.h, next to Requant; each launcher adds its own mode, guard and geometry conditions):
// y355_fp32_slope_ok, y355_fp32_exact and y355_fp32_fold are the three conditions named above.
#pragma once
#include "y355_dev.h"

namespace y355dev {
// wave-uniform: the scales can wait in SGPRs between the phases that use them
struct EpiScales {
    float s_pos, s_neg;      // 2^(lk - sh), neg_mul * 2^-sh
    float scl;               // FOLD 0: 2^shl
};
__device__ __forceinline__ EpiScales epi_scales(const Requant &rq) {
    EpiScales r;
    r.s_pos = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ldexpf(1.0f, rq.lk - rq.sh))));
    r.s_neg = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)rq.neg_mul * ldexpf(1.0f, -rq.sh))));
    r.scl = ldexpf(1.0f, rq.shl);
    return r;
}
// the fma operands, pinned into VGPRs
struct EpiOps {
    float sp, sn, cp, cn;    // the scales; the addends: FOLD 2 M * (1 - s), else M
};
template <int FOLD>
__device__ __forceinline__ EpiOps epi_ops(const EpiScales &r) {
    EpiOps v = {r.s_pos, r.s_neg, FOLD == 2 ? MAGIC - MAGIC * r.s_pos : MAGIC, FOLD == 2 ? MAGIC - MAGIC * r.s_neg : MAGIC};
    asm volatile("" : "+v"(v.sp), "+v"(v.sn), "+v"(v.cp), "+v"(v.cn));
    return v;
}
// (pooled) accumulator -> the two branches, unclamped
template <int FOLD>
__device__ __forceinline__ void epi_pair(int m, float biasf, const EpiScales &r, const EpiOps &v, float &pos, float &neg) {
    const float tf = FOLD == 2 ? __int_as_float(m) : FOLD == 1 ? (float)m : fmaf((float)m, r.scl, biasf);   // (float)m exact: |t| < 2^24
    pos = fmaf(tf, v.sp, v.cp);
    neg = fmaf(tf, v.sn, v.cn);
}
// hot: the unclamped low bytes of four outputs; ymx / ymn track the branches that can leave [-127, 127]
// NEGSAFE (Requant::negsafe: no accumulator the weights allow drives the negative branch below -127): ymn is not tracked
template <bool NEGSAFE>
__device__ __forceinline__ unsigned int epi_word_hot(const float (&pos)[4], const float (&neg)[4], float &ymx, float &ymn) {
    unsigned int w;
    ymx = vmax3(vmax3(ymx, pos[0], pos[1]), pos[2], pos[3]);
    if constexpr (!NEGSAFE) ymn = vmin3(vmin3(ymn, neg[0], neg[1]), neg[2], neg[3]);
    max_to_byte<0>(w, pos[0], neg[0]);
    max_to_byte<1>(w, pos[1], neg[1]);
    max_to_byte<2>(w, pos[2], neg[2]);
    max_to_byte<3>(w, pos[3], neg[3]);
    return w;
}
// cold: the clamped bytes; nbad += outputs that were clamped, where `own` (a lane that holds a real output)
__device__ __forceinline__ unsigned int epi_word_clamped(const float (&pos)[4], const float (&neg)[4], bool own, unsigned int &nbad) {
    float yc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float y = vmax(pos[q], neg[q]);
        yc[q] = __builtin_amdgcn_fmed3f(y, QLO, QHI);
        nbad += (own && y != yc[q]) ? 1u : 0u;
    }
    return pack4(yc[0], yc[1], yc[2], yc[3]);
}
// four (pooled) accumulators of one lane -> packed int8 word, hot (CLAMP = false) or cold
template <int FOLD, bool CLAMP, bool NEGSAFE>
__device__ __forceinline__ unsigned int epi_word(const int (&m)[4], const float (&biasf)[4], const EpiScales &r, const EpiOps &v, bool own,
                                                 float &ymx, float &ymn, unsigned int &nbad) {
    float pos[4], neg[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) epi_pair<FOLD>(m[q], biasf[q], r, v, pos[q], neg[q]);
    if constexpr (!CLAMP) return epi_word_hot<NEGSAFE>(pos, neg, ymx, ymn);
    else return epi_word_clamped(pos, neg, own, nbad);
}
}  // namespace y355dev
