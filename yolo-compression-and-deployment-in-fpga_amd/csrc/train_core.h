// The kernels and host helpers the training libraries share (train.hip: the BN-folded SlimYOLOv2, DESIGN.md section 6m;
// bntrain.hip: the BatchNorm SlimYOLOv2, section 6n; qtrain.hip: the fake-quantised BN-folded SlimYOLOv2, section 6o): the layer table, the convolution forward / data-gradient kernel with its
// epilogues, the weight-gradient and reduce kernels, the SGD + pack kernel, launch_conv and the weight gradient's plan.  Each
// library compiles its own copy (everything here is hidden or static); the including file has pushed hidden visibility and
// included y355_host.h.  The handle and the entry points' bodies on top of these are train_host.h's.
#ifndef Y355_TRAIN_CORE_H
#define Y355_TRAIN_CORE_H

typedef __bf16 tv8bf __attribute__((ext_vector_type(8)));
typedef float tv4f __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;                           // the bit pattern

constexpr int NL = 10;
constexpr float SLOPE = 0.125f;
// layer k = 1..10 (index k - 1): input channels, output channels (pred: from the configuration), pooled, the divisor of its grid
constexpr int kCin[NL] = {3, 16, 32, 64, 64, 128, 128, 256, 256, 256};
constexpr int kCout[NL] = {16, 32, 64, 64, 128, 128, 256, 256, 256, 0};
constexpr bool kPool[NL] = {true, true, false, true, false, true, false, false, false, false};
constexpr int kDiv[NL] = {1, 2, 4, 4, 8, 8, 16, 16, 16, 16};

__device__ __host__ inline int ilog2_(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}
inline int pow2_at_least(int v, int lo) {
    int p = lo;
    while (p < v) p *= 2;
    return p;
}

struct LayerDesc {
    int cin, cinp, cout, coutp;      // cinp: channels of the stored input (8 for the image); coutp: of G_k (pred: padded)
    int ct;                          // 16-row tiles a wave of the forward takes (1, 2, 4); the pack holds a multiple of it
    int ksf, ksd;                    // k-steps of the forward and of the data gradient
    int dct;                         // tiles a wave of the data gradient takes
    size_t woff, boff;               // of the flat parameter arrays
    size_t wf_off, wd_off;           // of the pack array (elements)
};
struct NetDesc {
    LayerDesc L[NL];
    size_t total;                    // parameters
};

inline int tiles_per_wave(int channels) {
    const int t = (channels + 15) / 16;
    return t >= 3 ? 4 : t;
}
// elements of layer L's forward pack: its 16-row tiles, rounded up to what a wave takes, times its k-steps of 64 x 8
inline size_t forward_pack_size(const LayerDesc &L) { return (size_t)(((L.cout + 15) / 16 + L.ct - 1) / L.ct * L.ct) * L.ksf * 512; }
// where a pack of `ks` k-steps keeps the element (row, kidx) of the A operand: tile row >> 4, k-step kidx >> 5, lane
// (g = (kidx >> 3) & 3, i = row & 15), element kidx & 7
__device__ __host__ inline size_t pack_index(int row, int ks, int kidx) {
    return ((((size_t)(row >> 4) * ks + (kidx >> 5)) * 64 + ((kidx >> 3) & 3) * 16 + (row & 15)) << 3) + (kidx & 7);
}

// ---------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ bf16_t rb_(float v) { return __builtin_bit_cast(bf16_t, (__bf16)v); }
__device__ __forceinline__ uint2 rb4_(const float (&v)[4]) {
    uint2 u;
    u.x = (unsigned)rb_(v[0]) | ((unsigned)rb_(v[1]) << 16);
    u.y = (unsigned)rb_(v[2]) | ((unsigned)rb_(v[3]) << 16);
    return u;
}

__global__ __launch_bounds__(256) void train_input_kernel(const float *__restrict__ x, bf16_t *__restrict__ a0, size_t npix, size_t hw) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const size_t b = p / hw, yx = p - b * hw;
    const float *s = x + b * 3 * hw + yx;
    uint4 u;
    u.x = (unsigned)rb_(s[0]) | ((unsigned)rb_(s[hw]) << 16);
    u.y = (unsigned)rb_(s[2 * hw]);
    u.z = 0;
    u.w = 0;
    *(uint4 *)(a0 + p * 8) = u;
}

__global__ __launch_bounds__(256) void train_dpred_kernel(const float *__restrict__ dp, bf16_t *__restrict__ g, size_t n, int cout, int coutp_log2,
                                                          size_t hw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t p = i >> coutp_log2;
    const int c = (int)(i & (((size_t)1 << coutp_log2) - 1));
    const size_t b = p / hw, yx = p - b * hw;
    g[i] = c < cout ? rb_(dp[(b * cout + c) * hw + yx]) : (bf16_t)0;
}

// M_Z (bntrain.hip alone): Z_k = rb(conv + bias) on the pre-pool grid, no slope and no pool.  M_Q* (qtrain.hip alone, DESIGN.md
// section 6o): the epilogues of the fake-quantised network -- the output rounded to 8 bits at the power of two of its tracker,
// a state byte per output element (bits 0-1: the window position, bit 2: the selected z <= 0, bit 3: clipped), the tracker's
// max|v| and clipped count through integer atomics; the data gradient reads slope and mask from the state byte of A_{k-1}.
enum { M_FWD = 0, M_FWD_POOL = 1, M_PRED = 2, M_DGRAD = 3, M_DGRAD_UNPOOL = 4, M_Z = 5, M_QFWD = 6, M_QFWD_POOL = 7, M_QPRED = 8, M_QDGRAD = 9,
       M_QDGRAD_UNPOOL = 10 };
enum { Q_POS = 3, Q_NEG = 4, Q_CLIP = 8 };          // the state byte's fields
struct ConvArgs {
    const bf16_t *in;                // NHWC, cinp channels, on the H x W grid
    const bf16_t *w;                 // packed A fragments
    const float *bias;
    int cinp_log2, ks;               // k-steps
    int B, H, W;
    int cout;                        // real output channels
    int outc;                        // channels of the NHWC output (and of act_prev / idx_prev / idx)
    void *out;
    unsigned char *idx;              // M_FWD_POOL: I_k
    const bf16_t *act_prev;          // data gradient: A_{k-1}
    const unsigned char *idx_prev;   // M_DGRAD_UNPOOL: I_{k-1}
    // M_Q* alone
    float qs, qi;                    // 2^e and 2^-e of the output's tracker
    unsigned char *state;            // S_k, on the output's grid at outc channels
    const unsigned char *state_prev; // data gradient: S_{k-1}
    unsigned int *stats;             // {bits of max|v|, elements with |rne(v 2^e)| > 127} of the output's tracker
};

// A tracker's statistics st = {bits of max|v|, clipped count} from every lane of a wave: the wave's maximum and sum, then at most
// one atomic each.  Integers, exact in any order.  The maximum only grows, so a wave that reads a value at least its own has
// nothing to add (a stale read costs an atomic, never a result): nearly every wave of a layer skips the contended address.
__device__ __forceinline__ void wave_stats_(unsigned int vmax, unsigned int n, unsigned int *st) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        vmax = max(vmax, (unsigned int)__shfl_xor((int)vmax, m));
        n += (unsigned int)__shfl_xor((int)n, m);
    }
    if ((threadIdx.x & 63) == 0) {
        if (vmax > __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st, vmax);
        if (n) atomicAdd(st + 1, n);
    }
}

// clip(rne(v 2^e), -127, 127) and whether it clipped; a zero comes out as +0 (the integer 0 has no sign)
__device__ __forceinline__ float quant_(float v, float qs, bool &clipped) {
    const float r = rintf(v * qs);
    clipped = fabsf(r) > 127.f;
    return fminf(fmaxf(r, -127.f), 127.f) + 0.0f;
}

template <int MODE, int CT>
__global__ __launch_bounds__(256) void train_conv_kernel(const ConvArgs a) {
    constexpr bool POOL = MODE == M_FWD_POOL || MODE == M_QFWD_POOL;
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int H = a.H, W = a.W;
    const size_t hw = (size_t)H * W, npix = (size_t)a.B * hw;
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t npo = (size_t)a.B * Ho * Wo;
    if ((POOL ? wave * 16 : wave * 64) >= (POOL ? npo : npix)) return;          // wave-uniform

    // the lane's column of each of the four sets: its pixel (linear, and y, x) or none
    size_t pl[4];
    int py[4], px[4];
    bool ok[4];
    size_t q_pool = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if constexpr (POOL) {
            const size_t q = wave * 16 + j;
            q_pool = q;
            ok[s] = q < npo;
            const size_t qq = ok[s] ? q : 0;
            const size_t b = qq / ((size_t)Ho * Wo), r = qq - b * Ho * Wo;
            py[s] = 2 * (int)(r / Wo) + (s >> 1);
            px[s] = 2 * (int)(r % Wo) + (s & 1);
            pl[s] = b * hw + (size_t)py[s] * W + px[s];
        } else {
            const size_t q = (wave * 4 + s) * 16 + j;
            ok[s] = q < npix;
            pl[s] = ok[s] ? q : 0;
            const size_t r = pl[s] % hw;
            py[s] = (int)(r / W);
            px[s] = (int)(r % W);
        }
    }

    tv4f acc[4][CT];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[s][t] = tv4f{0.f, 0.f, 0.f, 0.f};

    const int cmask = (1 << a.cinp_log2) - 1;
    const bf16_t *wp = a.w + ((size_t)blockIdx.y * CT * a.ks * 64 + lane) * 8;
    for (int ks = 0; ks < a.ks; ++ks) {
        const int k0 = ks * 32 + 8 * g;
        const int tap = k0 >> a.cinp_log2, ci = k0 & cmask;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        uint4 bfrag[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int yy = py[s] + dy, xx = px[s] + dx;
            const bool in = ok[s] && tap < 9 && yy >= 0 && yy < H && xx >= 0 && xx < W;
            bfrag[s] = uint4{0, 0, 0, 0};
            if (in) bfrag[s] = *(const uint4 *)(a.in + (((size_t)((long long)pl[s] + (long long)dy * W + dx)) << a.cinp_log2) + ci);
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const uint4 af = *(const uint4 *)(wp + ((size_t)t * a.ks + ks) * 512);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tv8bf, af), __builtin_bit_cast(tv8bf, bfrag[s]), acc[s][t], 0, 0, 0);
        }
    }

    // lane: column j of every set, rows 4 g .. 4 g + 3 of every tile
    [[maybe_unused]] unsigned int vmax = 0, nclip = 0;        // M_Q*: of the lane's elements before the pool
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int co = ((int)blockIdx.y * CT + t) * 16 + 4 * g;
        if constexpr (MODE == M_FWD || MODE == M_FWD_POOL) {
            float v[4][4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = acc[s][t][r] + a.bias[co + r];
                    v[s][r] = z > 0.f ? z : z * SLOPE;
                }
            if constexpr (POOL) {
                if (ok[0]) {
                    float best[4];
                    unsigned int pos = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        best[r] = v[0][r];
                        unsigned int w = 0;
#pragma unroll
                        for (int s = 1; s < 4; ++s)
                            if (v[s][r] > best[r]) {
                                best[r] = v[s][r];
                                w = s;
                            }
                        pos |= w << (8 * r);
                    }
                    *(uint2 *)((bf16_t *)a.out + q_pool * a.outc + co) = rb4_(best);
                    *(unsigned int *)(a.idx + q_pool * a.outc + co) = pos;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    if (ok[s]) *(uint2 *)((bf16_t *)a.out + pl[s] * a.outc + co) = rb4_(v[s]);
            }
        } else if constexpr (MODE == M_QFWD || MODE == M_QFWD_POOL) {
            float v[4][4];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = acc[s][t][r] + a.bias[co + r];
                    v[s][r] = z > 0.f ? z : z * SLOPE;
                    if (ok[s]) {
                        vmax = max(vmax, __builtin_bit_cast(unsigned int, fabsf(v[s][r])));
                        nclip += fabsf(v[s][r] * a.qs) >= 127.5f ? 1u : 0u;               // |rne(t)| > 127: 127.5 ties to 128
                    }
                }
            if constexpr (POOL) {
                if (ok[0]) {
                    float out[4];
                    unsigned int st = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float best = v[0][r];
                        unsigned int w = 0;
#pragma unroll
                        for (int s = 1; s < 4; ++s)
                            if (v[s][r] > best) {
                                best = v[s][r];
                                w = s;
                            }
                        bool c;
                        out[r] = quant_(best, a.qs, c) * a.qi;
                        st |= (w | (best <= 0.f ? Q_NEG : 0u) | (c ? Q_CLIP : 0u)) << (8 * r);
                    }
                    *(uint2 *)((bf16_t *)a.out + q_pool * a.outc + co) = rb4_(out);
                    *(unsigned int *)(a.state + q_pool * a.outc + co) = st;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (!ok[s]) continue;
                    float out[4];
                    unsigned int st = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        bool c;
                        out[r] = quant_(v[s][r], a.qs, c) * a.qi;
                        st |= ((v[s][r] <= 0.f ? Q_NEG : 0u) | (c ? Q_CLIP : 0u)) << (8 * r);
                    }
                    *(uint2 *)((bf16_t *)a.out + pl[s] * a.outc + co) = rb4_(out);
                    *(unsigned int *)(a.state + pl[s] * a.outc + co) = st;
                }
            }
        } else if constexpr (MODE == M_QPRED) {                   // a.outc: the padded channels of S_10 (P itself has a.cout)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                const size_t b = pl[s] / hw, yx = pl[s] - b * hw;
                unsigned int st = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.cout) {
                        const float z = acc[s][t][r] + a.bias[co + r];
                        vmax = max(vmax, __builtin_bit_cast(unsigned int, fabsf(z)));
                        bool c;
                        ((float *)a.out)[(b * a.cout + co + r) * hw + yx] = quant_(z, a.qs, c) * a.qi;
                        nclip += c ? 1u : 0u;
                        st |= (c ? Q_CLIP : 0u) << (8 * r);
                    }
                if (co < a.outc) *(unsigned int *)(a.state + pl[s] * a.outc + co) = st;
            }
        } else if constexpr (MODE == M_QDGRAD || MODE == M_QDGRAD_UNPOOL) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                const size_t at = pl[s] * a.outc + co;
                const unsigned int st = *(const unsigned int *)(a.state_prev + at);
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned int sb = st >> (8 * r);
                    v[r] = (sb & Q_CLIP) ? 0.f : acc[s][t][r] * ((sb & Q_NEG) ? SLOPE : 1.0f);
                }
                if constexpr (MODE == M_QDGRAD) {
                    *(uint2 *)((bf16_t *)a.out + at) = rb4_(v);
                } else {
                    const size_t b = pl[s] / hw;
                    const size_t row = (b * 2 * H + 2 * (size_t)py[s]) * 2 * W + 2 * (size_t)px[s];
#pragma unroll
                    for (int wpos = 0; wpos < 4; ++wpos) {
                        float u[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) u[r] = ((st >> (8 * r)) & Q_POS) == (unsigned)wpos ? v[r] : 0.f;
                        *(uint2 *)((bf16_t *)a.out + (row + (size_t)(wpos >> 1) * 2 * W + (wpos & 1)) * a.outc + co) = rb4_(u);
                    }
                }
            }
        } else if constexpr (MODE == M_Z) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                float z[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) z[r] = acc[s][t][r] + a.bias[co + r];
                *(uint2 *)((bf16_t *)a.out + pl[s] * a.outc + co) = rb4_(z);
            }
        } else if constexpr (MODE == M_PRED) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                const size_t b = pl[s] / hw, yx = pl[s] - b * hw;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.cout) ((float *)a.out)[(b * a.cout + co + r) * hw + yx] = acc[s][t][r] + a.bias[co + r];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                const size_t at = pl[s] * a.outc + co;
                const uint2 ap = *(const uint2 *)(a.act_prev + at);
                const short a16[4] = {(short)(ap.x & 0xffff), (short)(ap.x >> 16), (short)(ap.y & 0xffff), (short)(ap.y >> 16)};
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[s][t][r] * (a16[r] > 0 ? 1.0f : SLOPE);       // bf16 > 0: sign clear, not zero
                if constexpr (MODE == M_DGRAD) {
                    *(uint2 *)((bf16_t *)a.out + at) = rb4_(v);
                } else {
                    const unsigned int pos = *(const unsigned int *)(a.idx_prev + at);
                    const size_t b = pl[s] / hw;
                    const size_t row = (b * 2 * H + 2 * (size_t)py[s]) * 2 * W + 2 * (size_t)px[s];
#pragma unroll
                    for (int wpos = 0; wpos < 4; ++wpos) {
                        float u[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) u[r] = ((pos >> (8 * r)) & 0xff) == (unsigned)wpos ? v[r] : 0.f;
                        *(uint2 *)((bf16_t *)a.out + (row + (size_t)(wpos >> 1) * 2 * W + (wpos & 1)) * a.outc + co) = rb4_(u);
                    }
                }
            }
        }
    }
    if constexpr (MODE == M_QFWD || MODE == M_QFWD_POOL || MODE == M_QPRED) wave_stats_(vmax, nclip, a.stats);
}

struct WgradArgs {
    const bf16_t *g;                 // G_k, NHWC, coutp channels
    const bf16_t *act;               // A_{k-1}, NHWC, cinp channels
    float *ws;                       // [run][(co * cinp + ci) * 9 + tap | cout * cinp * 9 + co]
    size_t ws_stride, npix, chunk;   // chunk: pixels of a run, a multiple of 32
    int H, W, cinp, coutp, cout;
};

template <int MT>
__global__ __launch_bounds__(64) void train_wgrad_kernel(const WgradArgs a) {
    const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
    const int H = a.H, W = a.W;
    const size_t hw = (size_t)H * W;
    const size_t start = (size_t)blockIdx.z * a.chunk, end = start + a.chunk < a.npix ? start + a.chunk : a.npix;
    const bool with_bias = blockIdx.x == 0;
    const int ci = (int)blockIdx.x * 16 + j;
    const bool ci_ok = ci < a.cinp;

    tv4f acc[MT][9], accb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        accb[t] = tv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[t][tap] = tv4f{0.f, 0.f, 0.f, 0.f};
    }
    const uint4 ones = uint4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};     // eight bf16 1.0

    for (size_t p0 = start; p0 < end; p0 += 32) {
        const size_t pb = p0 + 8 * g;
        const size_t r0 = pb % hw;
        int y = (int)(r0 / W), x = (int)(r0 % W);
        int ys[8], xs[8];
        bool v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            ys[e] = y;
            xs[e] = x;
            v[e] = pb + e < end;
            if (++x == W) {
                x = 0;
                if (++y == H) y = 0;
            }
        }
        uint4 gf[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int co = ((int)blockIdx.y * MT + t) * 16 + j;
            unsigned short h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (v[e] && co < a.cout) ? a.g[(pb + e) * a.coutp + co] : (unsigned short)0;
            gf[t] = uint4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16), (unsigned)h[4] | ((unsigned)h[5] << 16),
                          (unsigned)h[6] | ((unsigned)h[7] << 16)};
        }
        if (with_bias) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
                accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tv8bf, gf[t]), __builtin_bit_cast(tv8bf, ones), accb[t], 0, 0, 0);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            unsigned short h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int yy = ys[e] + dy, xx = xs[e] + dx;
                const bool in = v[e] && ci_ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
                h[e] = in ? a.act[(size_t)((long long)(pb + e) + (long long)dy * W + dx) * a.cinp + ci] : (unsigned short)0;
            }
            const uint4 af = uint4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16),
                                   (unsigned)h[4] | ((unsigned)h[5] << 16), (unsigned)h[6] | ((unsigned)h[7] << 16)};
#pragma unroll
            for (int t = 0; t < MT; ++t)
                acc[t][tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tv8bf, gf[t]), __builtin_bit_cast(tv8bf, af), acc[t][tap], 0, 0, 0);
        }
    }

    // lane: column j (input channel ci), rows 4 g .. 4 g + 3 (output channels) of every tile
    float *ws = a.ws + (size_t)blockIdx.z * a.ws_stride;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = ((int)blockIdx.y * MT + t) * 16 + 4 * g + r;
            if (co >= a.cout) continue;
            if (ci_ok) {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) ws[((size_t)co * a.cinp + ci) * 9 + tap] = acc[t][tap][r];
            }
            if (with_bias && j == 0) ws[(size_t)a.cout * a.cinp * 9 + co] = accb[t][r];
        }
}

// dW [cout][cin][9] and db [cout] of one layer: the runs added in their order
__global__ __launch_bounds__(256) void train_reduce_kernel(const float *__restrict__ ws, size_t ws_stride, int runs, int cin, int cinp, int cout,
                                                           float *__restrict__ dw, float *__restrict__ db) {
    const size_t nw = (size_t)cout * cin * 9;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw + cout) return;
    size_t src;
    if (i < nw) {
        const size_t co = i / ((size_t)cin * 9), rem = i - co * cin * 9;
        src = (co * cinp + rem / 9) * 9 + rem % 9;
    } else {
        src = (size_t)cout * cinp * 9 + (i - nw);
    }
    float q[4] = {0.f, 0.f, 0.f, 0.f};                       // run r into q[r % 4]: four loads in flight, the order fixed all the same
    int r = 0;
    for (; r + 4 <= runs; r += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] += ws[(size_t)(r + u) * ws_stride + src];
    }
    for (int u = 0; r < runs; ++r, ++u) q[u] += ws[(size_t)r * ws_stride + src];
    const float s = (q[0] + q[1]) + (q[2] + q[3]);
    if (i < nw) dw[i] = s;
    else db[i - nw] = s;
}

// torch.optim.SGD (dampening 0, no Nesterov) on every parameter, then rb(W) into the two packs.  update == 0: the packs alone.
__global__ __launch_bounds__(256) void train_sgd_kernel(const NetDesc d, float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ buf,
                                                        bf16_t *__restrict__ packs, float lr, float momentum, float weight_decay, int first,
                                                        int update) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d.total) return;
    float w = p[i];
    if (update) {
        float gr = grad[i];
        gr = gr + weight_decay * w;
        float b = first ? gr : momentum * buf[i] + gr;
        buf[i] = b;
        w = w - lr * b;
        p[i] = w;
    }
    int k = 0;
    while (k < NL - 1 && i >= d.L[k + 1].woff) ++k;
    const LayerDesc &L = d.L[k];
    if (i >= L.boff) return;                                  // a bias
    const size_t e = i - L.woff;
    const int co = (int)(e / ((size_t)L.cin * 9)), rem = (int)(e - (size_t)co * L.cin * 9), ci = rem / 9, tap = rem % 9;
    const bf16_t h = rb_(w);
    {                                                         // pack_index, kept as written: the inline moves the kernel's code
        const int kidx = tap * L.cinp + ci;
        packs[L.wf_off + ((((size_t)(co >> 4) * L.ksf + (kidx >> 5)) * 64 + ((kidx >> 3) & 3) * 16 + (co & 15)) << 3) + (kidx & 7)] = h;
    }
    if (k > 0) {                                              // rotated by 180 degrees, (co, ci) transposed
        const int kidx = (8 - tap) * L.coutp + co;
        packs[L.wd_off + ((((size_t)(ci >> 4) * L.ksd + (kidx >> 5)) * 64 + ((kidx >> 3) & 3) * 16 + (ci & 15)) << 3) + (kidx & 7)] = h;
    }
}

static int wgrad_mt(const LayerDesc &L) { return L.cout >= 64 ? 4 : (L.cout >= 32 ? 2 : 1); }
static int wgrad_tiles(const LayerDesc &L) { return ((L.cinp + 15) / 16) * ((L.cout + 16 * wgrad_mt(L) - 1) / (16 * wgrad_mt(L))); }
static int wgrad_max_runs(const LayerDesc &L) { return std::max(1, 2048 / wgrad_tiles(L)); }       // about 2048 waves per layer
static size_t wgrad_stride(const LayerDesc &L) { return (size_t)L.cout * L.cinp * 9 + L.cout; }

// The split of a layer's npix = B H W pixels into runs of chunk pixels (a multiple of 32; the last run may be shorter): at most
// wgrad_max_runs(L) of them.  y355_train_backward launches from it and y355_train_wgrad_plan reports it.
struct WgradPlan {
    size_t npix, chunk;
    int max_runs, runs;
};
static WgradPlan wgrad_plan(const LayerDesc &L, int B, int H, int W) {
    WgradPlan p;
    p.npix = (size_t)B * H * W;
    p.max_runs = wgrad_max_runs(L);
    const size_t want = std::min<size_t>((size_t)p.max_runs, (p.npix + 31) / 32);
    p.chunk = ((p.npix + want - 1) / want + 31) / 32 * 32;
    p.runs = (int)((p.npix + p.chunk - 1) / p.chunk);
    return p;
}

template <int MODE>
static hipError_t launch_conv(const ConvArgs &a, int ct, int tiles, hipStream_t s) {
    const bool pool = MODE == M_FWD_POOL || MODE == M_QFWD_POOL;
    const size_t cols = pool ? (size_t)a.B * (a.H / 2) * (a.W / 2) : (size_t)a.B * a.H * a.W;
    const size_t waves = pool ? (cols + 15) / 16 : (cols + 63) / 64;
    const dim3 grid((unsigned)((waves + 3) / 4), (unsigned)((tiles + ct - 1) / ct)), block(256);
    if (ct == 1) hipLaunchKernelGGL((train_conv_kernel<MODE, 1>), grid, block, 0, s, a);
    else if (ct == 2) hipLaunchKernelGGL((train_conv_kernel<MODE, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((train_conv_kernel<MODE, 4>), grid, block, 0, s, a);
    return hipGetLastError();
}
#endif
