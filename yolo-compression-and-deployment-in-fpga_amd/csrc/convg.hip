// yolo355 -- generic chunked-K implicit-GEMM convolution (3x3/pad 1 or 1x1; stride 1, or 2 for 3x3) for gfx950,
// in two arithmetic types:
//   bf16 : BN-folded fp32 models run as bf16 x bf16 -> fp32 on v_mfma_f32_16x16x32_bf16
//          (SlimYOLOv2.forward, models/slim_yolo_v2.py:549-622; utils.modules.Conv2d :6-18)
//   int8 : the integer pipeline of conv3x3.hip for layers it cannot hold (more than 256 input
//          channels, 1x1 kernels, LeakyReLU slopes that are not a power of two:
//          models/tiny_yolo_v3.py:9-273, backbone/darknet.py:211-255)
//
// Same mapping as conv3x3.hip -- GEMM rows = output pixels of a TH x TW tile (2x2 pooling windows
// in adjacent rows), columns = output channels, nine taps = nine constant LDS offsets -- with the
// input patch staged in CHUNKS of CHB bytes per pixel, so the LDS slab is independent of the
// number of input channels.  A k-step is always 64 bytes of one pixel: 32 bf16 or 64 int8
// channels; byte-wise the A/B fragments of the two MFMA shapes are identical (lane (g, j)
// holds 16 bytes of row/column j at k-offset 16 g), which is why one kernel serves both.
#include "y355_common.h"
#include "convg_shared.h"
#include <climits>
#include <type_traits>

// integer epilogue with a general LeakyReLU slope neg_mul / 2^lk (DESIGN.md "requantisation"):
//   t = acc * 2^shl + bias;  t' = t >= 0 ? t * 2^lk : t * neg_mul;  q = clamp(RNE(t' * 2^-sh))
// shl: the output channel's own shift (per-channel weight exponents), a per-lane value
__device__ __forceinline__ long long requant_g(int acc, int shl, long long bias, const RequantG &rq) {
    long long t = (long long)acc * (1ll << shl) + bias;
    t = t >= 0 ? t * (1ll << rq.lk) : t * (long long)rq.neg_mul;
    return y355_rne_shift<long long>(t, rq.sh);
}

// the same with the int8 residual added before the one rounding (ResQ, y355_common.h)
__device__ __forceinline__ long long requant_g_res(int acc, int shl, long long bias, const RequantG &rq, int qr, const ResQ &rr) {
    long long t = (long long)acc * (1ll << shl) + bias;
    t = t >= 0 ? t * (1ll << rq.lk) : t * (long long)rq.neg_mul;
    const long long u = t * (1ll << rr.t_sh) + (long long)qr * (1ll << rr.r_sh);
    return y355_rne_shift<long long>(u, rr.sh);
}
// (the p_* / n_* shifts come from F = max(sa_in + max_c e_w, e_b), lk and the activation exponents: none depends on shl[c])
__device__ __forceinline__ int requant_gen32_res_t(int t, const Requant &rq, int qr, const ResQ &rr) {
    if (t >= 0) return y355_rne_shift32(t * (1 << rr.p_t) + qr * (1 << rr.p_r), rr.p_d);
    return y355_rne_shift32(t * rq.neg_mul * (1 << rr.n_t) + qr * (1 << rr.n_r), rr.n_d);
}
__device__ __forceinline__ int requant_gen32_res(int acc, int bias, const Requant &rq, int qr, const ResQ &rr) {
    const int t = (acc << rq.shl) + bias;
    if (t >= 0) return y355_rne_shift32(t * (1 << rr.p_t) + qr * (1 << rr.p_r), rr.p_d);
    return y355_rne_shift32(t * rq.neg_mul * (1 << rr.n_t) + qr * (1 << rr.n_r), rr.n_d);
}

// NT residual bytes of one pixel (int8, halo layout of the residual tensor), sign-extended; one vector load
template <int NT>
__device__ __forceinline__ void load_res_i8(const char *src, int (&r)[NT]) {
    static_assert(NT == 2 || NT == 4 || NT == 8, "NT");
    if constexpr (NT == 2) {
        const unsigned int v = *(const unsigned short *)src;
        r[0] = (int)(signed char)(v & 0xffu);
        r[1] = (int)(signed char)(v >> 8);
    } else {
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += 4) {
            const unsigned int v = *(const unsigned int *)(src + t0);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[t0 + k] = (int)(signed char)((v >> (8 * k)) & 0xffu);
        }
    }
}

// ---- statistics mode (STAT) of the int8 kernels: calibration on the int8 graph itself (y355_net_calibrate).  The 64-bit
// epilogue up to t' (residual layers: up to the sum u = t' 2^(G-E) + q_r 2^(G-s_r)) on every UN-POOLED output of the tile
// (the reference tracks in front of the pool, models/slim_yolo_v2.py:229-231), |.| in int64, reduced within the wave, ONE
// 64-bit atomicMax per wave into the op's slot (p.ctr->absmax).  Nothing else is written.  acc[m][t][r]: as the epilogues
// read it -- POOL: position r of 2x2 window (wm MT + m) 4 + g; otherwise tile row (wm MT + m) 16 + 4 g + r.
template <int MT, int NT, int TH, int TW, bool POOL, int S, bool PC>
__device__ __forceinline__ void convg_stat(const ConvGParams &p, const v4i (&acc)[MT][NT], int nlane, int wm, int g, int lane,
                                           int b, int y0, int x0) {
    constexpr int BM = TH * TW;
    const RequantG rq = p.rq;
    // the map the accumulators live on: the conv's own output (before any pool)
    const int Ho = S == 2 ? (p.H + 1) >> 1 : p.H, Wo = S == 2 ? (p.W + 1) >> 1 : p.W;
    const char *resb = (!POOL && p.res) ? p.res + (size_t)b * (Ho + 2) * (Wo + 2) * p.res_pb + p.res_off : nullptr;
    long long biasw[NT];
    int shl[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        biasw[t] = p.bias_w[nlane + t];
        shl[t] = PC ? p.shl_w[nlane + t] : rq.shl;
    }
    unsigned long long amax = 0;
    auto rowpos = [&](int m, int r, int &oy, int &ox) -> bool {
        if constexpr (POOL) {
            const int w = (wm * MT + m) * 4 + g;
            oy = y0 + 2 * (w / (TW / 2)) + (r >> 1);
            ox = x0 + 2 * (w % (TW / 2)) + (r & 1);
            return (w * 4 < BM) && oy < Ho && ox < Wo;
        } else {
            const int row = (wm * MT + m) * 16 + 4 * g + r;
            oy = y0 + row / TW;
            ox = x0 + row % TW;
            return row < BM && oy < Ho && ox < Wo;
        }
    };
    // One row at a time, in order: the running maximum passes through an opaque register barrier after every row, so the rows
    // form a serial chain.  (Left free, the compiler evaluates the 4 MT NT independent 64-bit values breadth-first and
    // reduces them as a tree: about 140 registers of temporaries, which the 8-wave tiles do not have.)
    unsigned int amax_lo = 0, amax_hi = 0;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int oy, ox;
            const bool valid = rowpos(m, r, oy, ox);
            int qr[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) qr[t] = 0;
            if (resb && valid) load_res_i8<NT>(resb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * p.res_pb + nlane, qr);
            amax = ((unsigned long long)amax_hi << 32) | amax_lo;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                long long v = (long long)acc[m][t][r] * (1ll << shl[t]) + biasw[t];
                v = v >= 0 ? v * (1ll << rq.lk) : v * (long long)rq.neg_mul;
                if (resb) v = v * (1ll << p.rr.t_sh) + (long long)qr[t] * (1ll << p.rr.r_sh);
                const unsigned long long a = (unsigned long long)(v < 0 ? -v : v);
                amax = (valid && a > amax) ? a : amax;
            }
            amax_lo = (unsigned int)amax;
            amax_hi = (unsigned int)(amax >> 32);
            asm volatile("" : "+v"(amax_lo), "+v"(amax_hi));
        }
    }
    amax = ((unsigned long long)amax_hi << 32) | amax_lo;
    const unsigned long long wmax = y355_wave_max_u64(amax);
    if (lane == 0 && wmax && p.ctr) atomicMax(&p.ctr->absmax, wmax);
}

// ---- four waves per workgroup (round 1): one tile per workgroup, stage -> barrier -> k-steps -> barrier per chunk.  Kept for
// the thin layers and the small / stride-2 tiles, where its 2-3 workgroups per CU overlap each other's phases.
// PC: the layer's weight exponents differ between output channels (ConvGParams::pc): the accumulator shift is the lane's own
// (bias word / shl_w); otherwise rq.shl, wave-uniform, and the code of the per-tensor layers is what it was
template <bool BF, int CHB, int BN, int TH, int TW, bool POOL, int WM, int WN, int S, bool NARROW = false, bool PC = false, bool STAT = false>
__global__ __launch_bounds__(256) void convg_kernel(const ConvGParams p) {
    using T = ConvGTile<CHB, BN, TH, TW, POOL, WM, WN, S>;
    constexpr bool THIN = T::THIN;
    constexpr int PW = T::PW, NPIX = T::NPIX, STRIDE = T::STRIDE, CPP = T::CPP, SUB = T::SUB, BM = T::BM, MT = T::MT, NT = T::NT;
    static_assert(WM * WN == 4, "4 waves");
    using ACC = MmaAcc<BF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    int bid = y355_xcd_remap(blockIdx.x, gridDim.x);
    const int nb = bid % p.nblk;
    bid /= p.nblk;
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int H = p.H, W = p.W;
    const int y0 = ty * TH, x0 = tx * TW;
    const int taps = p.taps;
    const int kpc = THIN ? 5 : SUB * taps;       // k-steps per chunk
    const int KS = kpc * p.nchunks;

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, g = lane >> 4;

    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int row = (wm * MT + m) * 16 + li;
        row = min(row, BM - 1);
        int oy, ox;
        if constexpr (POOL) {
            const int w = row >> 2, r = row & 3;
            oy = 2 * (w / (TW / 2)) + (r >> 1);
            ox = 2 * (w % (TW / 2)) + (r & 1);
        } else {
            oy = row / TW;
            ox = row % TW;
        }
        abase[m] = (S * oy * PW + S * ox) * STRIDE + (THIN ? 0 : g * 16);
    }
    int kofs[THIN ? 5 : 1];
    if constexpr (THIN) {
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
            const int tap = min(2 * ks + (g >> 1), 8);
            kofs[ks] = ((tap / 3) * PW + tap % 3) * STRIDE + (g & 1) * 16;
        }
    } else {
        kofs[0] = 0;
    }

    ACC acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = ACC{};

    const char *wp = p.w + ((size_t)(nb * KS) * WN + wn) * NT * 1024 + lane * 16;
    constexpr size_t WSTEP = (size_t)WN * NT * 1024;
    v4i bcur[NT], bnext[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bcur[t] = *(const v4i *)(wp + t * 1024);
    int ksg = 0;

    auto kstep = [&](int ko) {
        const int nx = min(ksg + 1, KS - 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) bnext[t] = *(const v4i *)(wp + (size_t)nx * WSTEP + t * 1024);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const v4i a = *(const v4i *)(smem + abase[m] + ko);
#pragma unroll
            for (int t = 0; t < NT; ++t) mma_step<BF>(acc[m][t], a, bcur[t]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) bcur[t] = bnext[t];
        ++ksg;
    };

    const char *inb = p.in + (size_t)b * (H + 2) * (W + 2) * p.in_pb;
    for (int ch = 0; ch < p.nchunks; ++ch) {
        if (ch) __syncthreads();
        // ---- stage CHB bytes of every patch pixel, 16 B per thread per step (tail clamped)
        {
            constexpr int ITEMS = NPIX * CPP;
            constexpr int BATCH = 8;
            const char *src0 = inb + ch * CHB;
            for (int it0 = tid; it0 < ITEMS; it0 += 256 * BATCH) {
                v4i v[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int it = min(it0 + u * 256, ITEMS - 1);
                    const int pix = it / CPP, c = it % CPP;
                    const int py = pix / PW, px = pix % PW;
                    const int gy = min(S * y0 + py, H + 1), gx = min(S * x0 + px, W + 1);
                    v[u] = *(const v4i *)(src0 + ((size_t)gy * (W + 2) + gx) * p.in_pb + c * 16);
                }
#pragma unroll
                for (int u = 0; u < BATCH; ++u) {
                    const int it = min(it0 + u * 256, ITEMS - 1);
                    const int pix = it / CPP, c = it % CPP;
                    *(v4i *)(smem + pix * STRIDE + c * 16) = v[u];
                }
            }
        }
        __syncthreads();
        CONVG_WALK_CHUNK(T, T::SUB, taps, kofs, kstep)
    }

    // ---- epilogue
    const int nlane = nb * BN + wn * (NT * 16) + li * NT;       // first of this lane's NT channels
    if constexpr (STAT && !BF) {                                // statistics mode: the maximum only
        convg_stat<MT, NT, TH, TW, POOL, S, PC>(p, acc, nlane, wm, g, lane, b, y0, x0);
        return;
    }
    const int halo = p.out_halo;
    const int Ho = POOL ? (H >> 1) : (S == 2 ? (H + 1) >> 1 : H), Wo = POOL ? (W >> 1) : (S == 2 ? (W + 1) >> 1 : W);
    char *outb = p.out + (size_t)b * (Ho + 2 * halo) * (Wo + 2 * halo) * p.out_pb + p.out_off;
    const char *resb = p.res ? p.res + (size_t)b * (Ho + 2) * (Wo + 2) * p.res_pb + p.res_off : nullptr;
    unsigned int nsat = 0;

    float biasf[NT];
    long long biasw[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if constexpr (BF) { biasf[t] = p.bias_f[nlane + t]; biasw[t] = 0; }
        else { biasw[t] = p.bias_w[nlane + t]; biasf[t] = 0.f; }
    }
    int biasn[NT];                                         // NARROW: the biases fit 32 bits too
#pragma unroll
    for (int t = 0; t < NT; ++t) biasn[t] = (int)biasw[t];
    int shlw[PC ? NT : 1] = {};                                         // PC, 64-bit epilogue: the channel's shift (NARROW: in the upper half of biasw, y355_pc_word)
    if constexpr (PC && !NARROW && !BF) {
#pragma unroll
        for (int t = 0; t < NT; ++t) shlw[t] = p.shl_w[nlane + t];
    }
    const float slope = p.slope;
    const RequantG rq = p.rq;
    Requant rqn{};
    rqn.shl = rq.shl; rqn.sh = rq.sh; rqn.lk = rq.lk; rqn.neg_mul = rq.neg_mul; rqn.split = rq.split;

    auto finish = [&](const float (&vf)[NT], const int (&vi)[NT], bool valid, int oy, int ox) {
        char *dst = outb + ((size_t)(oy + halo) * (Wo + 2 * halo) + ox + halo) * p.out_pb;
        if constexpr (BF) {
            float y[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float x = vf[t] + biasf[t];
                y[t] = x >= 0.f ? x : x * slope;
            }
            if (resb && valid) {                        // the residual is a bf16 activation: exact in fp32
                const unsigned short *r = (const unsigned short *)(resb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * p.res_pb) + nlane;
#pragma unroll
                for (int t = 0; t < NT; ++t) y[t] += __uint_as_float((unsigned int)r[t] << 16);
            }
            if (valid) {
                if (p.out_f32) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) ((float *)dst)[nlane + t] = y[t];
                } else {
                    store_bf16<NT>(dst + (size_t)nlane * 2, y);
                }
            }
        } else {
            int q[NT];
            if (resb) {                                 // residual: added before the one rounding (ResQ)
                int qr[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) qr[t] = 0;
                if (valid) load_res_i8<NT>(resb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * p.res_pb + nlane, qr);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if constexpr (NARROW) {
                        const int qq = PC ? requant_gen32_res_t(y355_pc_t(vi[t], biasw[t]), rqn, qr[t], p.rr) : requant_gen32_res(vi[t], biasn[t], rqn, qr[t], p.rr);
                        q[t] = y355_clamp8<int>(qq);
                        nsat += (valid && q[t] != qq) ? 1u : 0u;
                    } else {
                        const long long qq = requant_g_res(vi[t], PC ? shlw[PC ? t : 0] : rq.shl, biasw[t], rq, qr[t], p.rr);
                        q[t] = y355_clamp8<long long>(qq);
                        nsat += (valid && (long long)q[t] != qq) ? 1u : 0u;
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if constexpr (NARROW) {
                        const int qq = PC ? y355_requant_gen32_t(y355_pc_t(vi[t], biasw[t]), rqn) : y355_requant_gen32(vi[t], biasn[t], rqn);
                        q[t] = y355_clamp8<int>(qq);
                        nsat += (valid && q[t] != qq) ? 1u : 0u;
                    } else {
                        const long long qq = requant_g(vi[t], PC ? shlw[PC ? t : 0] : rq.shl, biasw[t], rq);
                        q[t] = y355_clamp8<long long>(qq);
                        nsat += (valid && (long long)q[t] != qq) ? 1u : 0u;
                    }
                }
            }
            if (valid) store_i8<NT>(dst + nlane, q);
        }
    };

#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if constexpr (POOL) {
            // monotone epilogue: pool the raw accumulators first
            const int w = (wm * MT + m) * 4 + g;
            const int wy = w / (TW / 2), wx = w % (TW / 2);
            const int oy = (y0 >> 1) + wy, ox = (x0 >> 1) + wx;
            const bool valid = (w * 4 < BM) && oy < Ho && ox < Wo;
            float vf[NT];
            int vi[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const ACC a = acc[m][t];
                if constexpr (BF) { vf[t] = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])); vi[t] = 0; }
                else { vi[t] = max(max(a[0], a[1]), max(a[2], a[3])); vf[t] = 0.f; }
            }
            finish(vf, vi, valid, oy, ox);
            __builtin_amdgcn_sched_barrier(0);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (wm * MT + m) * 16 + 4 * g + r;
                const int oy = y0 + row / TW, ox = x0 + row % TW;
                const bool valid = row < BM && oy < Ho && ox < Wo;
                float vf[NT];
                int vi[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if constexpr (BF) { vf[t] = acc[m][t][r]; vi[t] = 0; }
                    else { vi[t] = acc[m][t][r]; vf[t] = 0.f; }
                }
                finish(vf, vi, valid, oy, ox);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (!BF) {
        if (nsat && p.ctr) atomicAdd(&p.ctr->sat, (unsigned long long)nsat);
    }
}


// ---- eight waves per workgroup (round 2)
// One tile per workgroup, eight waves (96 accumulators per wave instead of 176: two waves per SIMD).  The input patch is staged
// in chunks of CHB bytes per pixel through TWO LDS slabs: the global loads of chunk c + 1 are issued before the k-steps of
// chunk c and written to the other slab after them, one barrier per chunk.  B fragments come straight from global memory
// (L2-resident), two k-steps ahead.  Measured (B = 64, slim fp32 / B = 128, tiny int8): 59.9 -> 63.8 k and 50.8 -> 63.1 k img/s.
// Persistent workgroups with the next tile's first chunk prefetched across the epilogue were built too and were SLOWER
// (58.2 k / 49.2 k): the extra live state spills, and one 8-wave workgroup per CU has nothing to overlap its epilogue with.
// What bounds this kernel now is the B path: 16-32 KB of fragments per k-step per CU through the vector-memory pipe
// (profiles/r02_notes.md); the int8 ring kernels avoid exactly that with LDS-DMA weight rings.
template <bool BF, int CHB, int BN, int TH, int TW, bool POOL, int WM, int WN, int S, bool NARROW = false, bool PC = false, bool STAT = false>
__global__ __launch_bounds__(WM * WN * 64) void convg8_kernel(const ConvGParams p, const int total) {
    constexpr int NTHR = WM * WN * 64;
    using T = ConvGTile<CHB, BN, TH, TW, POOL, WM, WN, S>;
    constexpr bool THIN = T::THIN;
    constexpr int PW = T::PW, NPIX = T::NPIX, STRIDE = T::STRIDE, CPP = T::CPP, SUB = T::SUB, BM = T::BM, MT = T::MT, NT = T::NT, SLAB = T::SLAB;
    static_assert(WM * WN == 8, "8 waves");
    using ACC = MmaAcc<BF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int H = p.H, W = p.W;
    const int taps = p.taps;
    const int kpc = THIN ? 5 : SUB * taps;       // k-steps per chunk
    const int KS = kpc * p.nchunks;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, g = lane >> 4;

    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int row = (wm * MT + m) * 16 + li;
        row = min(row, BM - 1);
        int oy, ox;
        if constexpr (POOL) {
            const int w = row >> 2, r = row & 3;
            oy = 2 * (w / (TW / 2)) + (r >> 1);
            ox = 2 * (w % (TW / 2)) + (r & 1);
        } else {
            oy = row / TW;
            ox = row % TW;
        }
        abase[m] = (S * oy * PW + S * ox) * STRIDE + (THIN ? 0 : g * 16);
    }
    int kofs[THIN ? 5 : 1];
    if constexpr (THIN) {
#pragma unroll
        for (int ks = 0; ks < 5; ++ks) {
            const int tap = min(2 * ks + (g >> 1), 8);
            kofs[ks] = ((tap / 3) * PW + tap % 3) * STRIDE + (g & 1) * 16;
        }
    } else {
        kofs[0] = 0;
    }

    int bid = y355_xcd_remap(blockIdx.x, gridDim.x);
    if (bid >= total) return;
    const int nb = bid % p.nblk;
    bid /= p.nblk;
    const int x0 = (bid % p.tiles_x) * TW;
    bid /= p.tiles_x;
    const int y0 = (bid % p.tiles_y) * TH;
    const int b = bid / p.tiles_y;

    // ---- staging: CHB bytes of every patch pixel, 16 B per thread per item (tail clamped: duplicates rewrite the same
    // bytes).  The item -> address arithmetic is recomputed per chunk on purpose: hoisted out of the loops it costs three
    // registers per item for the whole kernel.
    constexpr int ITEMS = NPIX * CPP;
    constexpr int NIT = (ITEMS + NTHR - 1) / NTHR;
    v4i stg[NIT];
    auto stage_load = [&](int bb, int yy, int xx, int ch) {
        const char *src0 = p.in + (size_t)bb * (H + 2) * (W + 2) * p.in_pb + ch * CHB;
        int tl = tid;
        asm volatile("" : "+v"(tl));
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int it = min(tl + u * NTHR, ITEMS - 1);
            const int pix = it / CPP, c = it % CPP;
            const int py = pix / PW, px = pix % PW;
            const int gy = min(S * yy + py, H + 1), gx = min(S * xx + px, W + 1);
            stg[u] = *(const v4i *)(src0 + ((size_t)gy * (W + 2) + gx) * p.in_pb + c * 16);
        }
    };
    auto stage_store = [&](char *dst) {
        int tl = tid;
        asm volatile("" : "+v"(tl));
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int it = min(tl + u * NTHR, ITEMS - 1);
            const int pix = it / CPP, c = it % CPP;
            *(v4i *)(dst + pix * STRIDE + c * 16) = stg[u];
        }
    };
    constexpr size_t WSTEP = (size_t)WN * NT * 1024;
    constexpr bool DEEP = !STAT;                 // B fragments two k-steps ahead (the statistics instantiations: one, to stay inside the register budget)
    v4i b0[NT], b1[NT];
    auto load_b01 = [&](const char *wp) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            b0[t] = *(const v4i *)(wp + t * 1024);
            if constexpr (DEEP) b1[t] = *(const v4i *)(wp + (size_t)min(1, KS - 1) * WSTEP + t * 1024);
            else b1[t] = b0[t];
        }
    };

    stage_load(b, y0, x0, 0);
    const char *wp = p.w + ((size_t)(nb * KS) * WN + wn) * NT * 1024 + lane * 16;
    load_b01(wp);
    stage_store(smem);
    __syncthreads();
    int cur = 0;                                 // slab holding the chunk about to be consumed
    unsigned int nsat = 0;
    const float slope = p.slope;
    const RequantG rq = p.rq;
    const int halo = p.out_halo;
    const int Ho = POOL ? (H >> 1) : (S == 2 ? (H + 1) >> 1 : H), Wo = POOL ? (W >> 1) : (S == 2 ? (W + 1) >> 1 : W);

    {
        ACC acc[MT][NT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[m][t] = ACC{};
        int ksg = 0;
        const char *slab = smem;
        auto kstep = [&](int ko) {
            const int nx = min(ksg + (DEEP ? 2 : 1), KS - 1);
            v4i bn[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[t] = *(const v4i *)(wp + (size_t)nx * WSTEP + t * 1024);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const v4i a = *(const v4i *)(slab + abase[m] + ko);
#pragma unroll
                for (int t = 0; t < NT; ++t) mma_step<BF>(acc[m][t], a, b0[t]);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if constexpr (DEEP) { b0[t] = b1[t]; b1[t] = bn[t]; }
                else b0[t] = bn[t];
            }
            ++ksg;
        };

        for (int ch = 0; ch < p.nchunks; ++ch) {
            const bool more = ch + 1 < p.nchunks;
            slab = smem + cur * SLAB;
            if (more && !STAT) stage_load(b, y0, x0, ch + 1);       // in flight under this chunk's k-steps
            CONVG_WALK_CHUNK(T, 1, taps, kofs, kstep)
            if (more) {
                if constexpr (STAT) stage_load(b, y0, x0, ch + 1);       // (behind them: the staging registers stay free under the k-steps)
                stage_store(smem + (cur ^ 1) * SLAB);
                __syncthreads();
                cur ^= 1;
            }
        }
        // ---- epilogue
        const int nlane = nb * BN + wn * (NT * 16) + li * NT;       // first of this lane's NT channels
        if constexpr (STAT && !BF) {                                // statistics mode: the maximum only
            convg_stat<MT, NT, TH, TW, POOL, S, PC>(p, acc, nlane, wm, g, lane, b, y0, x0);
            return;
        }
        char *outb = p.out + (size_t)b * (Ho + 2 * halo) * (Wo + 2 * halo) * p.out_pb + p.out_off;
        const char *resb = p.res ? p.res + (size_t)b * (Ho + 2) * (Wo + 2) * p.res_pb + p.res_off : nullptr;

        float biasf[NT];
        long long biasw[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (BF) { biasf[t] = p.bias_f[nlane + t]; biasw[t] = 0; }
            else { biasw[t] = p.bias_w[nlane + t]; biasf[t] = 0.f; }
        }
        int biasn[NT];                                         // NARROW: the biases fit 32 bits too
#pragma unroll
        for (int t = 0; t < NT; ++t) biasn[t] = (int)biasw[t];
        int shlw[PC ? NT : 1] = {};                                     // PC, 64-bit epilogue: the channel's shift (NARROW: in the upper half of biasw, y355_pc_word)
        if constexpr (PC && !NARROW && !BF) {
#pragma unroll
            for (int t = 0; t < NT; ++t) shlw[t] = p.shl_w[nlane + t];
        }
        Requant rqn{};
        rqn.shl = rq.shl; rqn.sh = rq.sh; rqn.lk = rq.lk; rqn.neg_mul = rq.neg_mul; rqn.split = rq.split;

        auto finish = [&](const float (&vf)[NT], const int (&vi)[NT], bool valid, int oy, int ox) {
            char *dst = outb + ((size_t)(oy + halo) * (Wo + 2 * halo) + ox + halo) * p.out_pb;
            if constexpr (BF) {
                float y[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float x = vf[t] + biasf[t];
                    y[t] = x >= 0.f ? x : x * slope;
                }
                if (resb && valid) {                        // the residual is a bf16 activation: exact in fp32
                    const unsigned short *r = (const unsigned short *)(resb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * p.res_pb) + nlane;
#pragma unroll
                    for (int t = 0; t < NT; ++t) y[t] += __uint_as_float((unsigned int)r[t] << 16);
                }
                if (valid) {
                    if (p.out_f32) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) ((float *)dst)[nlane + t] = y[t];
                    } else {
                        store_bf16<NT>(dst + (size_t)nlane * 2, y);
                    }
                }
            } else {
                int q[NT];
                if (resb) {                                 // residual: added before the one rounding (ResQ)
                    int qr[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) qr[t] = 0;
                    if (valid) load_res_i8<NT>(resb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * p.res_pb + nlane, qr);
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if constexpr (NARROW) {
                            const int qq = PC ? requant_gen32_res_t(y355_pc_t(vi[t], biasw[t]), rqn, qr[t], p.rr) : requant_gen32_res(vi[t], biasn[t], rqn, qr[t], p.rr);
                            q[t] = y355_clamp8<int>(qq);
                            nsat += (valid && q[t] != qq) ? 1u : 0u;
                        } else {
                            const long long qq = requant_g_res(vi[t], PC ? shlw[PC ? t : 0] : rq.shl, biasw[t], rq, qr[t], p.rr);
                            q[t] = y355_clamp8<long long>(qq);
                            nsat += (valid && (long long)q[t] != qq) ? 1u : 0u;
                        }
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if constexpr (NARROW) {
                            const int qq = PC ? y355_requant_gen32_t(y355_pc_t(vi[t], biasw[t]), rqn) : y355_requant_gen32(vi[t], biasn[t], rqn);
                            q[t] = y355_clamp8<int>(qq);
                            nsat += (valid && q[t] != qq) ? 1u : 0u;
                        } else {
                            const long long qq = requant_g(vi[t], PC ? shlw[PC ? t : 0] : rq.shl, biasw[t], rq);
                            q[t] = y355_clamp8<long long>(qq);
                            nsat += (valid && (long long)q[t] != qq) ? 1u : 0u;
                        }
                    }
                }
                if (valid) store_i8<NT>(dst + nlane, q);
            }
        };

#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if constexpr (POOL) {
                // monotone epilogue: pool the raw accumulators first
                const int w = (wm * MT + m) * 4 + g;
                const int wy = w / (TW / 2), wx = w % (TW / 2);
                const int oy = (y0 >> 1) + wy, ox = (x0 >> 1) + wx;
                const bool valid = (w * 4 < BM) && oy < Ho && ox < Wo;
                float vf[NT];
                int vi[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const ACC a = acc[m][t];
                    if constexpr (BF) { vf[t] = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])); vi[t] = 0; }
                    else { vi[t] = max(max(a[0], a[1]), max(a[2], a[3])); vf[t] = 0.f; }
                }
                finish(vf, vi, valid, oy, ox);
                __builtin_amdgcn_sched_barrier(0);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = (wm * MT + m) * 16 + 4 * g + r;
                    const int oy = y0 + row / TW, ox = x0 + row % TW;
                    const bool valid = row < BM && oy < Ho && ox < Wo;
                    float vf[NT];
                    int vi[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        if constexpr (BF) { vf[t] = acc[m][t][r]; vi[t] = 0; }
                        else { vi[t] = acc[m][t][r]; vf[t] = 0.f; }
                    }
                    finish(vf, vi, valid, oy, ox);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    if constexpr (!BF) {
        if (nsat && p.ctr) atomicAdd(&p.ctr->sat, (unsigned long long)nsat);
    }
}

// ------------------------------------------------------------------------------------------
template <bool BF, int CHB, int BN, int TH, int TW, bool POOL, int WM, int WN, int S = 1>
struct ConvGInst {
    static constexpr size_t SLAB = ConvGTile<CHB, BN, TH, TW, POOL, WM, WN, S>::SLAB;
    static constexpr bool EIGHT = (WM * WN == 8);
    static constexpr size_t LDS = EIGHT ? 2 * SLAB : SLAB;
    // the instantiations of this tile: the plain one; int8 also the 32-bit epilogue (NARROW) and / or per-channel shifts (PC),
    // and statistics mode (STAT: the 64-bit epilogue's, per-tensor or per-channel).  f(NARROW, PC, STAT) as std::bool_constant
    template <class F>
    static int variant(bool narrow, bool pc, bool stat, F &&f) {
        using Y = std::true_type;
        using N = std::false_type;
        if constexpr (!BF) {
            if (stat) return pc ? f(N{}, Y{}, Y{}) : f(N{}, N{}, Y{});
            if (narrow) return pc ? f(Y{}, Y{}, N{}) : f(Y{}, N{}, N{});
            if (pc) return f(N{}, Y{}, N{});
        }
        return f(N{}, N{}, N{});
    }
    // the 4-wave and the 8-wave kernel behind one name, with its launch geometry; one tile per workgroup (persistent 8-wave
    // workgroups measured slower: slim fp32, B = 64, 58.2 k vs 63.8 k img/s)
    template <bool NARROW, bool PC, bool STAT>
    struct Kernel {
        static const void *fn() {
            if constexpr (EIGHT) return (const void *)convg8_kernel<BF, CHB, BN, TH, TW, POOL, WM, WN, S, NARROW, PC, STAT>;
            else return (const void *)convg_kernel<BF, CHB, BN, TH, TW, POOL, WM, WN, S, NARROW, PC, STAT>;
        }
        static int launch(ConvGParams p, int nblocks, hipStream_t s) {
            void *args[] = {&p, &nblocks};              // (p) for 4 waves, (p, total) for 8: the runtime reads as many as the kernel has
            const size_t lds = EIGHT && p.nchunks > 1 ? 2 * SLAB : SLAB;
            return (int)hipLaunchKernel(fn(), dim3(nblocks), dim3(EIGHT ? 512 : 256), args, lds, s);
        }
        static int prepare() { return (int)hipFuncSetAttribute(fn(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS); }
    };
    static int launch_as(bool narrow, bool stat, const ConvGParams &p, int nblocks, hipStream_t s) {
        return variant(narrow, p.pc, stat, [&](auto n, auto pc, auto st) { return Kernel<decltype(n)::value, decltype(pc)::value, decltype(st)::value>::launch(p, nblocks, s); });
    }
    static void launch(const ConvGParams &p, int nblocks, hipStream_t s) { launch_as(p.rq.narrow, false, p, nblocks, s); }
    static void launch_stat(const ConvGParams &p, int nblocks, hipStream_t s) {      // int8 only
        if constexpr (!BF) launch_as(false, true, p, nblocks, s);
    }
    static int prepare() {
        for (int v = 0; v < (BF ? 1 : 8); ++v)
            if (int e = variant(v & 1, v & 2, v & 4, [](auto n, auto pc, auto st) { return Kernel<decltype(n)::value, decltype(pc)::value, decltype(st)::value>::prepare(); })) return e;
        return 0;
    }
    static constexpr ConvGInfo info() {
        return ConvGInfo{BF ? 1 : 0, CHB, BN, TH, TW, POOL ? 1 : 0, WM, WN, BN / 16 / WN, S, LDS, &launch, &prepare, &launch_stat};
    }
};

#define CONVG_SET(BF)                                                                                   \
    ConvGInst<BF, 32, 32, 16, 52, true, 4, 1>::info(),     /* 0 thin, pooled     (conv2)            */ \
    ConvGInst<BF, 32, 64, 13, 26, false, 2, 2>::info(),    /* 1 thin                                */ \
    ConvGInst<BF, 64, 64, 13, 26, false, 4, 2>::info(),    /* 2 64 B chunks      (conv3_1)          */ \
    ConvGInst<BF, 64, 64, 26, 26, true, 8, 1>::info(),     /* 3 64 B, pooled     (conv3_2, conv4_2) */ \
    ConvGInst<BF, 128, 128, 13, 26, false, 4, 2>::info(),  /* 4 128 B chunks     (conv4_1)          */ \
    ConvGInst<BF, 256, 256, 13, 13, false, 2, 4>::info(),  /* 5 256 B chunks     (conv5..7)         */ \
    ConvGInst<BF, 256, 64, 13, 13, false, 4, 1>::info(),   /* 6 256 B, few couts (pred)             */ \
    ConvGInst<BF, 64, 64, 8, 16, false, 4, 1>::info(),     /* 7 small tiles, any shape              */ \
    ConvGInst<BF, 64, 64, 8, 16, true, 4, 1>::info(),      /* 8 small tiles, pooled                 */ \
    ConvGInst<BF, 64, 64, 8, 16, false, 4, 1, 2>::info(),  /* 9 stride 2 (darknet53 down-sampling)  */ \
    ConvGInst<BF, 128, 64, 13, 13, false, 4, 2>::info()    /* 10 13x13 maps, 64 couts per workgroup: fills the chip at small batches */

static const ConvGInfo g_convg[2][Y355_G_COUNT] = {{CONVG_SET(false)}, {CONVG_SET(true)}};

const ConvGInfo *y355_convg_kernel(int bf, int id) {
    return (id >= 0 && id < Y355_G_COUNT) ? &g_convg[bf ? 1 : 0][id] : nullptr;
}

int y355_prepare_convg(void) {
    for (int bf = 0; bf < 2; ++bf)
        for (int i = 0; i < Y355_G_COUNT; ++i)
            if (int e = g_convg[bf][i].prepare()) return e;
    return 0;
}

// Pick the instantiation for a layer: `in_pb` bytes per input pixel (multiple of 32), real output
// channels `cout`, pooled or not, on an H x W map.
int y355_convg_select(int in_pb, int cout, int pool, int H, int W, int stride, int batch_hint) {
    if (stride == 2) return (in_pb % 64 == 0 && !pool) ? 9 : -1;
    const bool small = (H < 13 || W < 13);
    if (in_pb == 32) return pool ? 0 : 1;
    if (pool) return small ? 8 : 3;
    if (small) return 7;
    if (cout <= 64) return (in_pb % 256 == 0) ? 6 : 2;
    if (cout <= 128) return (in_pb % 128 == 0) ? 4 : 2;
    if (in_pb % 256 == 0) {
        // 256 output channels per workgroup on 13x13 tiles: too few workgroups for 256 CUs on small maps at small batches
        const long wgs = (long)((H + 12) / 13) * ((W + 12) / 13) * ((cout + 255) / 256) * (batch_hint > 0 ? batch_hint : 1 << 20);
        return wgs >= 192 ? 5 : 10;
    }
    return (in_pb % 128 == 0) ? 4 : 2;
}

int y355_convg_ksteps(const ConvGInfo &ki, int in_pb, int taps) {
    return ki.chb == 32 ? 5 : (in_pb / 64) * taps;
}

size_t y355_convg_packed_bytes(const ConvGInfo &ki, int in_pb, int taps, int cout_pad) {
    return (size_t)(cout_pad / ki.bn) * y355_convg_ksteps(ki, in_pb, taps) * ki.wn * ki.nt * 1024;
}

// B-fragment order as conv3x3.hip (y355_pack_weights), y355_pack_bfrags.  k-steps run chunk-major:
// ks = (chunk * SUB + sub) * taps + tap covers input bytes [64*(chunk*SUB+sub), +64); thin kernels: k-step ks holds taps 2 ks
// and 2 ks + 1, 32 bytes each.  `w` is [cout][cin][k][k] (k = 1 or 3), fp32 or int8.
void y355_convg_pack(const ConvGInfo &ki, const float *w_f, const int8_t *w_q, int cout, int cin, int ksize,
                     int in_pb, int cout_pad, char *dst) {
    const int taps = ksize * ksize, KS = y355_convg_ksteps(ki, in_pb, taps);
    const int kel = ki.bf ? 32 : 64;                      // elements of a k-step
    const bool thin = ki.chb == 32;
    y355_pack_bfrags(ki.bf, KS, ki.bn, ki.wn, ki.nt, w_f, w_q, cout, cin, taps, cout_pad, dst, [=](int ks, int k, int &tap, int &ci) {
        if (thin) { tap = 2 * ks + k / (kel / 2); ci = k % (kel / 2); }
        else { tap = ks % taps; ci = (ks / taps) * kel + k; }
    });
}

// ------------------------------------------------------------------------------------------
// First layer of the bf16 nets: fp32 NCHW (or uint8 frames) -> bf16 -> conv3x3(3 -> 16) + bias + LeakyReLU + 2x2 max
// pool -> bf16 NHWC16 with halo (SlimYOLOv2.conv1 + pool1, models/slim_yolo_v2.py:551-552).
// LDS patch of 8-byte pixels (r, g, b, 0); K = 3 filter rows x 2 pixels x 4 per MFMA, two MFMAs
// (pixel columns 0-1, then column 2) per 16 pixels x 16 channels.
// U8: the input is the camera frame (uint8 HWC BGR, p.x_u8): BaseTransform + BGR->RGB through a per-channel table of the bf16
// values (y355_norm_u8 rounded to bf16 as the fp32 load would be), so the patch holds the same bits.
template <int TW, bool U8 = false>
__global__ __launch_bounds__(256) void conv1_bf16_kernel(const Conv1FParams p) {
    constexpr int TH = 16;
    constexpr int PW = TW + 2, PH = TH + 2;
    constexpr int NW = (TH / 2) * (TW / 2);
    constexpr int MT_TOT = TH * TW / 16;
    __shared__ __attribute__((aligned(16))) uint2 patch[PH * PW + 8];
    __shared__ __attribute__((aligned(16))) unsigned short otile[NW * 16];

    const int tid = threadIdx.x;
    int bid = y355_xcd_remap(blockIdx.x, gridDim.x);
    const int tx = bid % p.tiles_x;
    bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int H = p.H, W = p.W;
    const int y0 = ty * TH, x0 = tx * TW;
    if constexpr (U8) {
        __shared__ unsigned short lut[3 * 256];
#pragma unroll
        for (int c = 0; c < 3; ++c) lut[c * 256 + tid] = __builtin_bit_cast(unsigned short, (__bf16)y355_norm_u8(tid, p.nmean[c], p.nstd[c]));
        __syncthreads();
        const uint8_t *fb = p.x_u8 + (size_t)b * H * W * 3;
        for (int it = tid; it < PH * PW; it += 256) {
            const int py = it / PW, px = it % PW;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            const bool inside = (gy >= 0) && (gy < H) && (gx >= 0) && (gx < W);
            const size_t o = ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * 3;
            unsigned short h[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] = inside ? lut[c * 256 + fb[o + (2 - c)]] : (unsigned short)0;     // RGB c = BGR byte 2 - c
            patch[it] = make_uint2((unsigned int)h[0] | ((unsigned int)h[1] << 16), (unsigned int)h[2]);
        }
    } else {
    const float *xb = p.x + (size_t)b * 3 * H * W;
    const size_t plane = (size_t)H * W;
    for (int it0 = tid; it0 < PH * PW; it0 += 256 * 4) {
        float v[4][3];
        bool inside[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int it = min(it0 + u * 256, PH * PW - 1);
            const int py = it / PW, px = it % PW;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            inside[u] = (gy >= 0) && (gy < H) && (gx >= 0) && (gx < W);
            const size_t o = (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[u][c] = xb[c * plane + o];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int it = min(it0 + u * 256, PH * PW - 1);
            unsigned short h[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] = inside[u] ? __builtin_bit_cast(unsigned short, (__bf16)v[u][c]) : (unsigned short)0;
            uint2 w;
            w.x = (unsigned int)h[0] | ((unsigned int)h[1] << 16);
            w.y = (unsigned int)h[2];
            patch[it] = w;
        }
    }
    }
    if (tid < 8) patch[PH * PW + tid] = make_uint2(0u, 0u);
    __syncthreads();

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    const v4i bw0 = *(const v4i *)(p.w + lane * 16);
    const v4i bw1 = *(const v4i *)(p.w + 1024 + lane * 16);
    const float bias = p.bias[li];
    const float slope = p.slope;
    const int Ho = H >> 1, Wo = W >> 1;
    for (int mt = wave; mt < MT_TOT; mt += 4) {
        const int row = mt * 16 + li;
        const int w = row >> 2, r = row & 3;
        const int oy = 2 * (w / (TW / 2)) + (r >> 1);
        const int ox = 2 * (w % (TW / 2)) + (r & 1);
        const uint2 *src = patch + (oy + min(g, 2)) * PW + ox;
        const uint2 s0 = src[0], s1 = src[1], s2 = src[2], s3 = src[3];
        const v4i a0 = {(int)s0.x, (int)s0.y, (int)s1.x, (int)s1.y};
        const v4i a1 = {(int)s2.x, (int)s2.y, (int)s3.x, (int)s3.y};
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a0), __builtin_bit_cast(v8bf, bw0), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, a1), __builtin_bit_cast(v8bf, bw1), acc, 0, 0, 0);
        const int wo = mt * 4 + g;
        const float x = fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3])) + bias;
        const float y = x >= 0.f ? x : x * slope;
        otile[wo * 16 + li] = __builtin_bit_cast(unsigned short, (__bf16)y);
    }
    __syncthreads();
    char *outb = p.out + (size_t)b * (Ho + 2) * (Wo + 2) * 32;
    for (int it = tid; it < NW * 2; it += 256) {
        const int w = it >> 1, hf = it & 1;
        const int wy = w / (TW / 2), wx = w % (TW / 2);
        const int oy = (y0 >> 1) + wy, ox = (x0 >> 1) + wx;
        if (oy < Ho && ox < Wo)
            *(v4i *)(outb + ((size_t)(oy + 1) * (Wo + 2) + ox + 1) * 32 + hf * 16) = *(const v4i *)((const char *)otile + w * 32 + hf * 16);
    }
}

static int conv1f_tw(int W) { return (W % 104 == 0) ? 104 : 32; }

void y355_conv1f_tiles(int H, int W, int *tx, int *ty) {
    const int tw = conv1f_tw(W);
    *tx = (W + tw - 1) / tw;
    *ty = (H + 15) / 16;
}

void y355_launch_conv1f(const Conv1FParams &p, hipStream_t s) {
    const int n = p.tiles_x * p.tiles_y * p.B;
    const bool big = conv1f_tw(p.W) == 104;
    if (p.x) {
        if (big) hipLaunchKernelGGL((conv1_bf16_kernel<104>), dim3(n), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((conv1_bf16_kernel<32>), dim3(n), dim3(256), 0, s, p);
    } else {                                                  // uint8 frames (y355_net_forward_u8)
        if (big) hipLaunchKernelGGL((conv1_bf16_kernel<104, true>), dim3(n), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((conv1_bf16_kernel<32, true>), dim3(n), dim3(256), 0, s, p);
    }
}

// two B fragments: lane (g = filter row, j = cout) holds k = 4 d' + c, d' = 0,1 -> pixel column
// d = 2 f + d' of fragment f (column 3 and colour 3 are zero)
void y355_pack_conv1f(const float *w /*[16][3][3][3]*/, char *dst /*2048*/) {
    for (int f = 0; f < 2; ++f)
        for (int l = 0; l < 64; ++l) {
            const int g = l >> 4, j = l & 15;
            for (int e = 0; e < 8; ++e) {
                const int d = 2 * f + (e >> 2), c = e & 3;
                float v = 0.f;
                if (g < 3 && d < 3 && c < 3) v = w[((j * 3 + c) * 3 + g) * 3 + d];
                const unsigned short h = y355_bf16_rne(v);
                memcpy(dst + f * 1024 + l * 16 + e * 2, &h, 2);
            }
        }
}
