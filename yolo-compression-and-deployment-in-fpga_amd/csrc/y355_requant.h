// yolo355 -- the host half of the int8 fixed-point epilogue: the kernel-argument structs (Requant, RequantG, ResQ) and the ONE
// derivation of their contents from a layer's exponents, biases and weights.  Plain C++17, no HIP and no handle: g++ compiles
// it, and tests/requant_host_check.cpp walks it under the sanitizers.  The device half is y355_common.h's helpers
// (y355_requant_fast, y355_requant_gen32, y355_pc_word) and y355_fp32epi.h.
//
// "Why may this layer run the 32-bit / fp32 epilogue" is answered here:
//   y355_rq_fixed      everything in front of the output exponent: F, the accumulator shifts, the pre-shifted biases, and the
//                      two bounds on |t| (tw: worst-case weights, tb: the layer's own)
//   y355_rq_engine     conv3x3.hip / conv3x3_ring.hip / convpx.hip / pxpair.hip / front.hip of the SlimYOLOv2 engine and the
//                      operator layer (ops.hip): wide (64-bit kernels), tmax_log2 and negsafe (fp32 on exact integers:
//                      y355_fp32_exact, y355_fp32_fold), the branch-free 32-bit constants, the head-room guard
//   y355_rq_net        convg.hip / convr.hip / the pointwise kernel of the y355_net families: narrow (32-bit instantiation) by
//                      y355_rq_fits32 on tb, else split (the negative branch's product in two halves)
//   y355_rq_first      conv1.hip as y355_net's first layer: gen32 by y355_rq_fits32 on tw
//   y355_rq_front      front.hip under y355_net: tmax_log2, negsafe, wide
//   y355_rq_res        residual layers of convg.hip: the 64-bit proof and the 32-bit form
//   y355_rq_stat       the statistics pass of y355_net_calibrate: no requantisation, t' (residual: the sum u) in 64 bits
// Bounds are long doubles holding integers times powers of two below 2^64: exact (tests/int8_tile_cases.py restates the net's
// rule in rationals).  A refusal is a value (Y355RqErr: the code and a static message); the callers hand it to y355_fail.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// Fixed-point epilogue of one fused layer (DESIGN.md "requantisation"):
//   t  = (acc << shl) + bias_t[c]        bias_t = q_b << (F - e_b),  F = max(sa_in + e_w, e_b)
//   t' = leaky ? max(t, 8 t) : t         LeakyReLU(0.125) scaled by 8, F' = F + 3
//   q  = clamp(RNE(t' * 2^-sh), +-127)   sh = F' - sa_out
// Restates models/slim_yolo_v2.py:220-231 + :33-38 exactly in integers;
// shift composition as programmed by c_embedding/yolo_forward.c:233-257.
struct Requant {
    int shl;
    int sh;
    int leaky;
    int guard_log2;   // guard trips when |t'| >= 2^guard_log2 ( >= 63: never )
    int wide;         // 1: worst-case |t'| does not fit 30 bits -> 64-bit epilogue kernels
    // branch-free form of the same pipeline (32-bit path), filled by the host:
    //   t' = max(t, t << lk)                       lk = leaky ? 3 : 0
    //   q  = ((t' << sh_l) + hm1 + bfe(t', sh_r, bw)) >> sh_r
    // with sh_r = max(sh,0), sh_l = max(-sh,0), hm1 = sh>0 ? 2^(sh-1)-1 : 0, bw = sh>0 ? 1 : 0
    int lk, sh_l, sh_r, hm1, bw;
    // general LeakyReLU slope neg_mul / 2^lk (1 / 2^3 = the reference's 0.125); only the 64-bit
    // epilogues (y355_pre) honour neg_mul != 1
    int neg_mul;
    // 1: the general slope fits 32 bits (host-checked: |t| * max(2^max(0, lk - sh), neg_mul * 2^max(0, -sh)) < 2^31):
    //   q = t >= 0 ? rne(t * 2^(lk - sh)) : rne(t * neg_mul * 2^-sh)          (y355_requant_gen32; first layer of y355_net)
    int gen32;
    // |t| = |(acc << shl) + bias_t| < 2^tmax_log2 for worst-case operands (<= 24: t is exact in fp32, y355_fp32_exact)
    int tmax_log2;
    // gen32 only: 1 = the negative branch's product t * neg_mul does not fit 32 bits but t does; it is taken in two halves
    // (y355_requant_gen32): needs sh >= 9 and (|t| / 256 + 1) * neg_mul + 256 < 2^31 (host-checked)
    int split;
    // 1: the LeakyReLU's negative branch cannot leave [-127, 127]: |t| * neg_mul * 2^-sh <= 127 for the worst-case |t| of these weights
    // (host-checked on the exact bound, not on 2^tmax_log2): the hot passes of y355_fp32epi.h's NEGSAFE form (front.hip) then do not track that branch's minimum
    int negsafe;
};
// Host rules of the fp32 epilogue on exact integers (y355_fp32epi.h has their reasons): slope in [0, 1]; t exact; the FOLD class
inline bool y355_fp32_slope_ok(const Requant &rq) { return rq.neg_mul >= 0 && rq.neg_mul <= (1 << rq.lk); }
inline bool y355_fp32_exact(const Requant &rq) { return !rq.wide && rq.tmax_log2 <= 24; }
inline int y355_fp32_fold(const Requant &rq) { return rq.shl != 0 ? 0 : (rq.tmax_log2 <= 22 && rq.sh <= 22 && rq.sh - rq.lk >= -8) ? 2 : 1; }

// ---- generic chunked conv (convg.hip): bf16 nets and the int8 layers conv3x3.hip cannot hold --
struct RequantG {
    int shl;       // t = acc * 2^shl + bias (the kernels read it per output channel: bias_w / shl_w of ConvGParams)
    int sh;        // q = clamp(RNE(t' * 2^-sh))
    int lk;        // t' = t >= 0 ? t * 2^lk : t * neg_mul     (LeakyReLU slope neg_mul / 2^lk)
    int neg_mul;
    int narrow;    // 1: the whole epilogue fits 32 bits (host-checked bound): the 8-wave kernels take their 32-bit instantiation
    int split;     // narrow only: Requant::split (the negative branch's product in two halves)
};

// int8 residual (backbone/darknet.py:36 `x + block(x)`), one rounding after the add (DESIGN.md "int8 DarkNet"):
//   E = F + lk (exponent of t'), s_r the residual's, G = max(E, s_r)
//   u = t' * 2^(G - E) + q_r * 2^(G - s_r);  q = clamp(RNE(u * 2^(s_out - G)))
// 64-bit form: t_sh = G - E, r_sh = G - s_r, sh = G - s_out.  32-bit form (RequantG::narrow), the same rational per branch
// over a common power of two 2^d: X = t * 2^(lk - sh' + d) + q_r * 2^(s_out - s_r + d) (t >= 0, sh' = E - s_out) or
// X = t * neg_mul * 2^(d - sh') + q_r * 2^(s_out - s_r + d) (t < 0); q = clamp(RNE(X * 2^-d)) -- host-checked to fit 31 bits
struct ResQ {
    int t_sh, r_sh, sh;       // 64-bit form
    int p_t, p_r, p_d;        // 32-bit form, t >= 0
    int n_t, n_r, n_d;        // 32-bit form, t < 0
};

// ---- the derivation ----------------------------------------------------------------------------------------------------------
constexpr int Y355_RQ_ERANGE = -4;                  // Y355_ERANGE of include/yolo355.h (engine.hip asserts that they agree)
struct Y355RqErr { int code; const char *msg; };    // code 0: none
constexpr Y355RqErr Y355_RQ_OK{0, ""};
constexpr Y355RqErr Y355_RQ_GAP{Y355_RQ_ERANGE, "exponent gap too large for the fixed-point epilogue"};
constexpr Y355RqErr Y355_RQ_62{Y355_RQ_ERANGE, "fixed-point epilogue exceeds 62 bits"};
inline long double y355_rq_pow2(int n) { return std::ldexp(1.0L, n); }

// largest accumulator shift a caller accepts (y355_rq_fixed's shl_max).  Engine and operator layer: conv3x3.hip forms
// t = acc << shl in 32 bits (y355_requant_fast).  y355_net: the limit include/yolo355.h documents for convg.hip's per-channel
// shifts ("shl[c] > 24 is Y355_ERANGE"); why it is lower than the engine's is not recorded
constexpr int Y355_RQ_SHL_MAX_ENGINE = 30, Y355_RQ_SHL_MAX_NET = 24;

// The fixed-point epilogue of an int8 convolution up to t', for the exponents in front of the layer -- none of this depends on
// the output's exponent:  t = acc * 2^shc[c] + bw[c] at exponent F = max(sa_i + e_w, e_b),
// t' = t >= 0 ? t * 2^lk : t * nm at exponent E = F + lk
struct Y355RqFixed {
    int sa_i, F, shl, bshl, lk, nm, E;      // shl: of the channels with the largest weight exponent, the smallest of shc
    std::vector<long long> bw;              // [cout_pad] q_b << bshl
    std::vector<int> shc;                   // [cout_pad] every output channel's own accumulator shift
    long double bmax;                       // max |bw|
    long double tw, tb;                     // bounds on |t|: worst-case weights / the layer's own (|acc| <= 127 sum |q_w|)
    long double slope() const { return std::max(y355_rq_pow2(lk), (long double)nm); }      // |t'| <= |t| * slope()
};
// e_w [nch], wabs [nch] (sum |q_w| per channel, or null: unknown; all zero counts as unknown): nch = cout, or 1 for a per-tensor
// layer that knows only its largest sum.  K = taps * cin, the products of one accumulator.  LeakyReLU slope neg_mul / 2^lk.
// tw is 127 * 127 per product in the channel with the largest shift; a layer whose exponents differ takes its own weights
// there too (the worst-case weight in the channel with the largest shift is a bound nobody needs)
inline Y355RqErr y355_rq_fixed(int sa_in, const int *e_w, const long long *wabs, int nch, int e_b, const int32_t *q_b, int cout,
                               int cout_pad, int lk, int neg_mul, long long K, int shl_max, Y355RqFixed *cf) {
    const int e_hi = *std::max_element(e_w, e_w + nch), e_lo = *std::min_element(e_w, e_w + nch);
    cf->sa_i = sa_in;
    cf->F = std::max(sa_in + e_hi, e_b);
    cf->shl = cf->F - sa_in - e_hi;
    cf->bshl = cf->F - e_b;
    cf->lk = lk;
    cf->nm = neg_mul;
    cf->E = cf->F + lk;
    if (cf->F - sa_in - e_lo > shl_max || cf->bshl > 40) return Y355_RQ_GAP;
    cf->bw.assign(cout_pad, 0);
    cf->shc.assign(cout_pad, 0);
    cf->bmax = 0;
    long double own = 0;
    for (int c = 0; c < cout; ++c) {
        cf->bw[c] = (long long)((unsigned long long)(long long)q_b[c] << cf->bshl);     // q_b * 2^bshl (a product past 64 bits wraps)
        cf->shc[c] = cf->F - sa_in - e_w[nch == 1 ? 0 : c];
        cf->bmax = std::max(cf->bmax, std::fabs((long double)q_b[c]) * y355_rq_pow2(cf->bshl));
        if (wabs) own = std::max(own, (long double)127 * wabs[nch == 1 ? 0 : c] * y355_rq_pow2(cf->shc[c]));
    }
    const bool known = wabs && *std::max_element(wabs, wabs + nch) > 0;
    const long double generic = (long double)127 * 127 * K * y355_rq_pow2(cf->F - sa_in - e_lo);
    cf->tw = (known && e_lo != e_hi ? own : generic) + cf->bmax;
    cf->tb = (known ? own : generic) + cf->bmax;
    return Y355_RQ_OK;
}

// ---- what every consumer's rule is made of
// the general-slope epilogue fits 32 bits (y355_requant_gen32) for |t| <= t:
//   |t| * max(2^max(0, lk - sh), nm * 2^max(0, -sh)) + rounding < 2^31
inline bool y355_rq_fits32(const Y355RqFixed &cf, long double t, int sh) {
    const long double fpos = y355_rq_pow2(std::max(0, cf.lk - sh)), fneg = (long double)cf.nm * y355_rq_pow2(std::max(0, -sh));
    return t * std::max(fpos, fneg) + y355_rq_pow2(std::max(sh, 0)) < y355_rq_pow2(31) && cf.bmax < y355_rq_pow2(31);
}
// the constants every Requant carries: never guarded; each rule adds what its kernel reads beyond these
inline Requant y355_rq_base(const Y355RqFixed &cf, int sh) {
    Requant r{};
    r.shl = cf.shl; r.sh = sh; r.leaky = (cf.lk || cf.nm != 1) ? 1 : 0; r.lk = cf.lk; r.neg_mul = cf.nm; r.guard_log2 = 63;
    return r;
}
// Requant::tmax_log2: the smallest n (<= 62) with |t| < 2^n on the layer's own weights
inline int y355_rq_tmax_log2(const Y355RqFixed &cf) {
    int n = 0;
    while (n < 62 && y355_rq_pow2(n) <= cf.tb) ++n;
    return n;
}
// Requant::negsafe: the negative branch cannot leave [-127, 127] on the layer's own weights
inline int y355_rq_negsafe(const Y355RqFixed &cf, int sh) { return std::ldexp(cf.tb * cf.nm, -sh) <= 127.0L ? 1 : 0; }
// the 32-bit copy of the pre-shifted biases (meaningful only where a 32-bit or fp32 epilogue was selected)
inline std::vector<int32_t> y355_rq_bias32(const Y355RqFixed &cf) {
    std::vector<int32_t> b(cf.bw.size());
    for (size_t c = 0; c < b.size(); ++c) b[c] = (int32_t)cf.bw[c];
    return b;
}

// ---- the SlimYOLOv2 engine and the operator layer
// act: 0 none (prediction layer), 1 LeakyReLU(0.125) (t' = t >= 0 ? 8 t : t, F' = F + 3), 2 ReLU (utils/modules.py:26 with
// leakyReLU=False: t' = max(t, 0), F' = F; runs on the generic kernels, whose epilogue honours neg_mul = 0)
inline void y355_rq_act(int act, int *lk, int *neg_mul) {
    *lk = act == 1 ? 3 : 0;
    *neg_mul = act == 2 ? 0 : 1;
}
// Requantisation to sa_out when have_out, else none (sh = 0: t' is the result).  `wide` keeps the operand-independent bound tw;
// only tmax_log2 and negsafe, the gates of the fp32-exact epilogues, use the layer's own.  *frac_bits = F', the exponent of t'
inline Y355RqErr y355_rq_engine(const Y355RqFixed &cf, int sa_out, bool have_out, int retune, Requant *rq, int *frac_bits) {
    int sh = have_out ? cf.E - sa_out : 0;
    if (sh > 62) sh = 62;                                                   // (everything is rounded away from there on)
    if (sh < -30) return Y355RqErr{Y355_RQ_ERANGE, "output exponent too large"};      // conv3x3.hip shifts t' left in 32 bits
    // worst-case magnitude through the rounding add / left shift
    const long double tmax = cf.tw * cf.slope();
    const long double lim = sh > 0 ? tmax + y355_rq_pow2(sh - 1) : sh < 0 ? std::ldexp(tmax, -sh) : tmax;
    if (lim >= y355_rq_pow2(62)) return Y355_RQ_62;
    const int wide = lim >= y355_rq_pow2(30) ? 1 : 0;
    if (!wide && sh > 31) sh = 31;                  // (the 32-bit kernels' shift count; never taken: sh > 31 puts 2^31 into lim)
    Requant r = y355_rq_base(cf, sh);
    r.wide = wide;
    r.tmax_log2 = y355_rq_tmax_log2(cf);
    r.negsafe = y355_rq_negsafe(cf, sh);
    r.sh_l = sh < 0 ? -sh : 0;
    r.sh_r = sh > 0 ? sh : 0;
    r.hm1 = sh > 0 ? (int)((1ll << (sh - 1)) - 1) : 0;
    r.bw = sh > 0 ? 1 : 0;
    const int g = 15 + cf.E - retune;               // yolo_forward.c:35: the reference's 2^15 head room, moved by the layer's retune
    r.guard_log2 = g < 0 ? 0 : (g > 63 ? 63 : g);
    *rq = r;
    *frac_bits = cf.E;
    return Y355_RQ_OK;
}
// one stand-alone 3x3 / general-geometry layer from its plain numbers: y355_rq_fixed (per-tensor, wabs = the largest sum |q_w|
// of an output channel or 0: unknown), then y355_rq_engine; the biases [cout_pad] in both widths.  A refusal leaves *out alone
struct Y355RqLayer {
    Requant rq{};
    int frac_bits = 0;
    std::vector<int32_t> bias_t;
    std::vector<long long> bias_w;
};
inline Y355RqErr y355_rq_layer(int cin, int taps, int sa_in, int e_w, int e_b, int sa_out, bool have_out, int act, int retune,
                               const int32_t *q_b, int cout, int cout_pad, long long wabs, Y355RqLayer *out) {
    Y355RqFixed cf;
    int lk, nm;
    y355_rq_act(act, &lk, &nm);
    Y355RqErr e = y355_rq_fixed(sa_in, &e_w, &wabs, 1, e_b, q_b, cout, cout_pad, lk, nm, (long long)taps * cin, Y355_RQ_SHL_MAX_ENGINE, &cf);
    if (!e.code) e = y355_rq_engine(cf, sa_out, have_out, retune, &out->rq, &out->frac_bits);
    if (e.code) return e;
    out->bias_t = y355_rq_bias32(cf);
    out->bias_w = std::move(cf.bw);
    return Y355_RQ_OK;
}

// ---- the y355_net families
// convg.hip / convr.hip / pointwise: the 64-bit proof on tw, then the 32-bit epilogue on the layer's own weights (a tighter
// bound than 127 per weight)
inline Y355RqErr y355_rq_net(const Y355RqFixed &cf, int sa_out, RequantG *rq) {
    const int lk = cf.lk, nm = cf.nm, sh = cf.E - sa_out;
    if (sh > 62 || sh < -20) return Y355_RQ_GAP;      // convg.hip: refused, where the engine clamps at 62 and goes down to -30 (no reason recorded)
    // worst case |t'| (through the slope and a left shift / the rounding add) must stay below 2^62; the rounding add counts as
    // 2^sh here and as 2^(sh - 1) in y355_rq_engine (both kept as they were)
    long double lim = cf.tw * cf.slope();
    lim = sh < 0 ? lim * y355_rq_pow2(-sh) : lim + y355_rq_pow2(sh);
    if (lim >= y355_rq_pow2(62)) return Y355_RQ_62;
    *rq = RequantG{cf.shl, sh, lk, nm, y355_rq_fits32(cf, cf.tb, sh) ? 1 : 0, 0};
    if (!rq->narrow && sh >= 9 && sh <= 31 && nm >= 1 && nm < 4096) {
        // t itself and the positive branch fit 32 bits, only t * neg_mul does not: the negative branch goes in two halves
        const long double pos = cf.tb * y355_rq_pow2(std::max(0, lk - sh)) + y355_rq_pow2(std::max(sh - lk, 0));
        const long double neg = (cf.tb / 256 + 1) * nm + 256 + y355_rq_pow2(sh - 9);
        if (cf.tb < y355_rq_pow2(30) && pos < y355_rq_pow2(31) && neg < y355_rq_pow2(31) && cf.bmax < y355_rq_pow2(31))
            rq->narrow = rq->split = 1;
    }
    return Y355_RQ_OK;
}
// conv1.hip as the first layer: its fast kernel when the epilogue fits 32 bits for worst-case weights, else the 64-bit one
inline Requant y355_rq_first(const Y355RqFixed &cf, int sh) {
    Requant r = y355_rq_base(cf, sh);
    r.wide = 1;
    r.gen32 = y355_rq_fits32(cf, cf.tw, sh) ? 1 : 0;
    return r;
}
// front.hip: t = acc * 2^shl + bias below 2^24 (exact in fp32) on the layer's own weights
inline Requant y355_rq_front(const Y355RqFixed &cf, int sh) {
    Requant r = y355_rq_base(cf, sh);
    r.tmax_log2 = y355_rq_tmax_log2(cf);
    r.negsafe = y355_rq_negsafe(cf, sh);
    // the magic-number rounding needs |t * slope| < 2^22 only where it does not saturate, and |sh| moderate
    r.wide = (r.tmax_log2 > 24 || cf.bmax >= y355_rq_pow2(24) || sh > 30 || sh - cf.lk < -8 || cf.nm < 1 || cf.nm > (1 << cf.lk)) ? 1 : 0;
    return r;
}
// exponents of a residual layer's epilogue (ResQ) and whether its 32-bit form holds for these weights (*narrow; no split
// form).  Refuses when no bound proves the 64-bit sum u = t' 2^(G-E) + q_r 2^(G-s_r) (and its rounding) below 2^62.
inline Y355RqErr y355_rq_res(const Y355RqFixed &cf, int sa_o, int s_r, ResQ *rr, int *narrow) {
    const Y355RqErr refused{Y355_RQ_ERANGE, "residual epilogue exceeds 62 bits"};
    const int lk = cf.lk, nm = cf.nm, E = cf.E, G = std::max(E, s_r);
    *rr = ResQ{};
    rr->t_sh = G - E;
    rr->r_sh = G - s_r;
    rr->sh = G - sa_o;
    *narrow = 0;
    if (rr->t_sh > 62 || rr->r_sh > 62 || rr->sh > 62 || rr->sh < -62) return refused;
    long double u = cf.tw * cf.slope() * y355_rq_pow2(rr->t_sh) + 127.0L * y355_rq_pow2(rr->r_sh);
    u = rr->sh < 0 ? u * y355_rq_pow2(-rr->sh) : u + y355_rq_pow2(rr->sh);
    if (u >= y355_rq_pow2(62)) return refused;
    // 32-bit form: both branches over their common power of two, on the layer's own weights
    const int shp = E - sa_o;
    const int dp = std::max({shp - lk, s_r - sa_o, 0}), dn = std::max({shp, s_r - sa_o, 0});
    rr->p_t = lk - shp + dp; rr->p_r = sa_o - s_r + dp; rr->p_d = dp;
    rr->n_t = dn - shp; rr->n_r = sa_o - s_r + dn; rr->n_d = dn;
    const long double tb = cf.tb, lim = y355_rq_pow2(31);
    if (dp <= 30 && dn <= 30 && rr->p_t <= 30 && rr->p_r <= 30 && rr->n_t <= 30 && rr->n_r <= 30 && tb < lim && cf.bmax < lim &&
        tb * y355_rq_pow2(rr->p_t) + 127.0L * y355_rq_pow2(rr->p_r) + y355_rq_pow2(dp) < lim &&
        tb * nm * y355_rq_pow2(rr->n_t) + 127.0L * y355_rq_pow2(rr->n_r) + y355_rq_pow2(dn) < lim)
        *narrow = 1;
    return Y355_RQ_OK;
}
// the statistics pass: the 64-bit epilogue up to t' with no requantisation (residual, res: up to the sum u, whose exponent is
// G = max(E, s_r)).  *frac_bits = the exponent of the tracked integers
inline Y355RqErr y355_rq_stat(const Y355RqFixed &cf, bool res, int s_r, RequantG *rq, Requant *rq1, ResQ *rr, int *frac_bits) {
    int fb = cf.E;
    long double lim = cf.tw * cf.slope();
    *rr = ResQ{};
    if (res) {
        const int G = std::max(fb, s_r);
        rr->t_sh = G - fb;
        rr->r_sh = G - s_r;
        if (rr->t_sh > 62 || rr->r_sh > 62) return Y355RqErr{Y355_RQ_ERANGE, "residual layer: exponent gap too large"};
        lim = lim * y355_rq_pow2(rr->t_sh) + 127.0L * y355_rq_pow2(rr->r_sh);
        fb = G;
    }
    if (lim >= y355_rq_pow2(62)) return Y355_RQ_62;
    *rq = RequantG{cf.shl, 0, cf.lk, cf.nm, 0, 0};
    *rq1 = y355_rq_base(cf, 0);
    rq1->wide = 1;
    *frac_bits = fb;
    return Y355_RQ_OK;
}
