// yolo355_convgrad -- a differentiable convolution of any geometry the operator API accepts, on the bf16 MFMA of gfx950: forward,
// data gradient, weight and bias gradient from fp32 tensors that stay on the device; C ABI in include/yolo355_convgrad.h, linked
// into libyolo355_convgrad.so on its own (nothing of libyolo355.so is used).  The arithmetic contract is DESIGN.md section 6p.
// These are the kernels of train_core.h without its assumptions (3x3 / pad 1 / stride 1, power-of-two channels): no LDS, no
// speed asserted.
//
// Layouts.  The staged operands rb(x) and G are NHWC bf16 with the channels padded with zeros to a multiple of 8 (cp), so a
// lane's MFMA fragment of eight consecutive k = tap * cp + c lies inside one tap and is one 16-byte load.  K = taps * cp is cut
// into k-steps of 32; weights are packed per (16-row tile, k-step) as the 64 x 16 bytes of the A operand (lane (g, i): row i,
// k = 8 g .. 8 g + 7), zeros where the row, the tap or the channel does not exist.
//
// The kernels:
//   cg_stage_kernel   fp32 NCHW -> bf16 NHWC, channels padded; <true>: G = rb(dy * (y > 0 ? 1 : slope))
//   cg_pack_kernel    rb(W) into the A fragments, every element of the pack written; <false>: rows co, k = tap * cinp + ci (the
//                     forward); <true>: rows ci, k = (taps - 1 - tap) * coutp + co (the data gradient: flipped, transposed)
//   cg_conv_kernel    implicit GEMM, rows = output channels of the pass, columns = 64 pixels of its output grid per wave, gathered
//                     under the tap predicate (<false>: iy = oy s + ky d - pad inside the map; <true>: oy = (iy + pad - ky d) / s
//                     where s divides it and oy lies inside G's grid); a tap outside is not loaded.  Epilogue: + bias, slope,
//                     fp32 NCHW, every element of the output once.
//   cg_wgrad_kernel   rows = output channels of G, columns = 16 input channels of rb(x) at one tap, summed over a run of
//                     pixels; one wave per (tile, tap, run), partial sums to a workspace; the wave of tap 0 / tile 0 adds the
//                     bias-gradient row
//   cg_reduce_kernel  adds the runs in a fixed order (four interleaved chains, then their sum): no atomics
#include "../../include/yolo355_convgrad.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_CONVGRAD_OK == Y355_OK && Y355_CONVGRAD_EINVAL == Y355_EINVAL && Y355_CONVGRAD_EHIP == Y355_EHIP,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_convgrad_last_error's text
#ifndef Y355_HOSTCHECK                                   // (convgrad_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

typedef __bf16 cv8bf __attribute__((ext_vector_type(8)));
typedef float cv4f __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;                           // the bit pattern

// ---------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ bf16_t rb_(float v) { return __builtin_bit_cast(bf16_t, (__bf16)v); }
__device__ __forceinline__ uint4 pack8_(const unsigned short (&h)[8]) {
    return uint4{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16), (unsigned)h[4] | ((unsigned)h[5] << 16),
                 (unsigned)h[6] | ((unsigned)h[7] << 16)};
}

// dst [npix][cp] = rb(src [B][c][hw]) (MASK: times the slope where y <= 0), channels c .. cp - 1 zero; one thread per pixel and
// group of eight channels, consecutive threads on consecutive pixels
template <bool MASK>
__global__ __launch_bounds__(256) void cg_stage_kernel(const float *__restrict__ src, const float *__restrict__ y, float slope,
                                                       bf16_t *__restrict__ dst, size_t npix, size_t hw, int c, int cp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix * (size_t)(cp >> 3)) return;
    const size_t cg = i / npix, p = i - cg * npix;
    const size_t b = p / hw, yx = p - b * hw;
    unsigned short h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int ch = (int)cg * 8 + e;
        float v = 0.f;
        if (ch < c) {
            const size_t at = (b * c + ch) * hw + yx;
            v = src[at];
            if constexpr (MASK) v = v * (y[at] > 0.f ? 1.0f : slope);
        }
        h[e] = rb_(v);
    }
    *(uint4 *)(dst + p * cp + cg * 8) = pack8_(h);
}

struct PackArgs {
    size_t n;                        // elements of the pack: tiles (rounded up to what a wave takes) * ks * 512
    int ks, rows, kc, kcp, ntaps, cin;       // kc / kcp: the channels of k and their padded count
};
template <bool DGRAD>
__global__ __launch_bounds__(256) void cg_pack_kernel(const float *__restrict__ w, bf16_t *__restrict__ pack, const PackArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const size_t rest = i >> 9;
    const size_t tile = rest / a.ks;
    const int ksi = (int)(rest - tile * a.ks);
    const size_t row = tile * 16 + (lane & 15);
    const int kidx = ksi * 32 + (lane >> 4) * 8 + e;
    const int tapk = kidx / a.kcp, ch = kidx - tapk * a.kcp;
    float v = 0.f;
    if (row < (size_t)a.rows && tapk < a.ntaps && ch < a.kc) {
        if constexpr (DGRAD) v = w[((size_t)ch * a.cin + row) * a.ntaps + (a.ntaps - 1 - tapk)];       // row = ci, ch = co
        else v = w[(row * a.cin + ch) * a.ntaps + tapk];                                                // row = co, ch = ci
    }
    pack[i] = rb_(v);
}

struct ConvArgs {
    const bf16_t *in;                // NHWC, cp channels, on the hin x win grid
    const bf16_t *w;                 // packed A fragments
    const float *bias;               // or null
    float *out;                      // NCHW, c channels, on the hout x wout grid
    float slope;
    int cp, ks;
    int B, hin, win, hout, wout;
    int c;                           // real rows
    int kh, kw, sh, sw, dh, dw, pt, pl;
};

template <bool DGRAD, int CT>
__global__ __launch_bounds__(256) void cg_conv_kernel(const ConvArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t hwo = (size_t)a.hout * a.wout, npix = (size_t)a.B * hwo;
    if (wave * 64 >= npix) return;                                               // wave-uniform

    // the lane's column of each of the four sets: its pixel (image, y, x) or none
    size_t pb[4], pyx[4];
    int py[4], px[4];
    bool ok[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const size_t q = (wave * 4 + s) * 16 + j;
        ok[s] = q < npix;
        const size_t qq = ok[s] ? q : 0;
        pb[s] = qq / hwo;
        pyx[s] = qq - pb[s] * hwo;
        py[s] = (int)(pyx[s] / a.wout);
        px[s] = (int)(pyx[s] % a.wout);
    }

    cv4f acc[4][CT];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[s][t] = cv4f{0.f, 0.f, 0.f, 0.f};

    // k = 32 ks + 8 g as (tap = ky * kw + kx, channel ch), walked by carries: cp >= 8, so at most four carries per k-step
    int ch = 8 * g, ky = 0, kx = 0;
    const bf16_t *wp = a.w + ((size_t)blockIdx.y * CT * a.ks * 64 + lane) * 8;
    for (int ks = 0; ks < a.ks; ++ks) {
        while (ch >= a.cp) {
            ch -= a.cp;
            if (++kx == a.kw) {
                kx = 0;
                ++ky;
            }
        }
        const bool tap_ok = ky < a.kh;                                           // the last k-step may run past the taps
        uint4 bfrag[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            int iy, ix;
            bool in = ok[s] && tap_ok;
            if constexpr (DGRAD) {                                               // the flipped tap (kh - 1 - ky, kw - 1 - kx)
                const int ty = py[s] + a.pt - (a.kh - 1 - ky) * a.dh, tx = px[s] + a.pl - (a.kw - 1 - kx) * a.dw;
                in = in && ty >= 0 && tx >= 0 && ty % a.sh == 0 && tx % a.sw == 0;
                iy = ty / a.sh;
                ix = tx / a.sw;
                in = in && iy < a.hin && ix < a.win;
            } else {
                iy = py[s] * a.sh + ky * a.dh - a.pt;
                ix = px[s] * a.sw + kx * a.dw - a.pl;
                in = in && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win;
            }
            bfrag[s] = uint4{0, 0, 0, 0};
            if (in) bfrag[s] = *(const uint4 *)(a.in + ((pb[s] * a.hin + (size_t)iy) * a.win + (size_t)ix) * a.cp + ch);
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const uint4 af = *(const uint4 *)(wp + ((size_t)t * a.ks + ks) * 512);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cv8bf, af), __builtin_bit_cast(cv8bf, bfrag[s]), acc[s][t], 0, 0, 0);
        }
        ch += 32;
    }

    // lane: column j of every set, rows 4 g .. 4 g + 3 of every tile
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = ((int)blockIdx.y * CT + t) * 16 + 4 * g + r;
            if (row >= a.c) continue;
            const float bias = a.bias ? a.bias[row] : 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!ok[s]) continue;
                float z = acc[s][t][r];
                if (a.bias) z = z + bias;
                a.out[(pb[s] * a.c + row) * hwo + pyx[s]] = z > 0.f ? z : z * a.slope;
            }
        }
}

struct WgradArgs {
    const bf16_t *g;                 // G, NHWC, coutp channels, on the ho x wo grid
    const bf16_t *x;                 // rb(x), NHWC, cinp channels, on the h x w grid
    float *ws;                       // [run][(co * cin + ci) * ntaps + tap | cout * cin * ntaps + co]
    size_t ws_stride, npix, chunk;   // chunk: pixels of a run, a multiple of 32
    int h, w, ho, wo, cin, cinp, cout, coutp;
    int kw, ntaps, sh, sw, dh, dw, pt, pl, ci_tiles;
};

template <int MT>
__global__ __launch_bounds__(64) void cg_wgrad_kernel(const WgradArgs a) {
    const int lane = threadIdx.x, j = lane & 15, g = lane >> 4;
    const size_t hwo = (size_t)a.ho * a.wo;
    const size_t start = (size_t)blockIdx.z * a.chunk, end = start + a.chunk < a.npix ? start + a.chunk : a.npix;
    const bool with_bias = blockIdx.x == 0;
    const int tap = (int)blockIdx.x / a.ci_tiles, cit = (int)blockIdx.x - tap * a.ci_tiles;
    const int offy = (tap / a.kw) * a.dh - a.pt, offx = (tap % a.kw) * a.dw - a.pl;
    const int ci = cit * 16 + j;
    const bool ci_ok = ci < a.cin;

    cv4f acc[MT], accb[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = accb[t] = cv4f{0.f, 0.f, 0.f, 0.f};
    const uint4 ones = uint4{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};     // eight bf16 1.0

    for (size_t p0 = start; p0 < end; p0 += 32) {
        const size_t pb = p0 + 8 * g;
        size_t b = pb / hwo;
        const size_t r0 = pb - b * hwo;
        int oy = (int)(r0 / a.wo), ox = (int)(r0 % a.wo);
        bool v[8];
        unsigned short hx[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[e] = pb + e < end;
            const int iy = oy * a.sh + offy, ix = ox * a.sw + offx;
            const bool in = v[e] && ci_ok && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
            hx[e] = in ? a.x[((b * a.h + (size_t)iy) * a.w + (size_t)ix) * a.cinp + ci] : (unsigned short)0;
            if (++ox == a.wo) {
                ox = 0;
                if (++oy == a.ho) {
                    oy = 0;
                    ++b;
                }
            }
        }
        const uint4 xf = pack8_(hx);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int co = ((int)blockIdx.y * MT + t) * 16 + j;
            unsigned short hg[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) hg[e] = (v[e] && co < a.cout) ? a.g[(pb + e) * a.coutp + co] : (unsigned short)0;
            const uint4 gf = pack8_(hg);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cv8bf, gf), __builtin_bit_cast(cv8bf, xf), acc[t], 0, 0, 0);
            if (with_bias) accb[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cv8bf, gf), __builtin_bit_cast(cv8bf, ones), accb[t], 0, 0, 0);
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
            if (ci_ok) ws[((size_t)co * a.cin + ci) * a.ntaps + tap] = acc[t][r];
            if (with_bias && j == 0) ws[(size_t)a.cout * a.cin * a.ntaps + co] = accb[t][r];
        }
}

// dw [nw] and db [nb] (either may be null): the runs added in their order
__global__ __launch_bounds__(256) void cg_reduce_kernel(const float *__restrict__ ws, size_t ws_stride, int runs, size_t nw, size_t nb,
                                                        float *__restrict__ dw, float *__restrict__ db) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nw + nb) return;
    float q[4] = {0.f, 0.f, 0.f, 0.f};                       // run r into q[r % 4]: four loads in flight, the order fixed all the same
    int r = 0;
    for (; r + 4 <= runs; r += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] += ws[(size_t)(r + u) * ws_stride + i];
    }
    for (int u = 0; r < runs; ++r, ++u) q[u] += ws[(size_t)r * ws_stride + i];
    const float s = (q[0] + q[1]) + (q[2] + q[3]);
    if (i < nw) {
        if (dw) dw[i] = s;
    } else if (db) {
        db[i - nw] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------- the handle
struct ConvGradDev {                 // the device memory, all of it y355_convgrad::own's
    bf16_t *wf = nullptr, *wd = nullptr;         // the packs, from the create
    bf16_t *xs = nullptr, *gs = nullptr;         // workspaces, grown on demand: rb(x), G
    float *ws = nullptr;                         // the weight gradient's runs
    size_t xs_cap = 0, gs_cap = 0, ws_cap = 0;
};
struct y355_convgrad : ConvGradDev {
    DevOwner own;
    int device_id = 0;
    int cin = 0, cout = 0, cinp = 0, coutp = 0, ntaps = 0;
    y355_convgrad_geom g{};
    float slope = 1.f;
    int ct = 1, dct = 1;             // 16-row tiles a wave of the forward / of the data gradient takes
    int ksf = 0, ksd = 0;            // their k-steps
    size_t wf_n = 0, wd_n = 0;       // elements of the packs
};

static int tiles_per_wave(int channels) {
    const int t = (channels + 15) / 16;
    return t >= 3 ? 4 : t;
}
static size_t pack_size(int rows, int ct, int ks) { return (size_t)(((rows + 15) / 16 + ct - 1) / ct * ct) * ks * 512; }

static int geom_limits(const char *who, const y355_convgrad_geom *g) {
    const std::string w(who);
    if (!g) return y355_fail(Y355_EINVAL, w + ": null argument");
    if (g->kh < 1 || g->kh > 32 || g->kw < 1 || g->kw > 32) return y355_fail(Y355_EINVAL, w + ": kernel size must be 1..32");
    if (g->stride_h < 1 || g->stride_h > 16 || g->stride_w < 1 || g->stride_w > 16) return y355_fail(Y355_EINVAL, w + ": stride must be 1..16");
    if (g->dil_h < 1 || g->dil_h > 32 || g->dil_w < 1 || g->dil_w > 32) return y355_fail(Y355_EINVAL, w + ": dilation must be 1..32");
    for (int p : {g->pad_top, g->pad_bottom, g->pad_left, g->pad_right})
        if (p < 0 || p > 64) return y355_fail(Y355_EINVAL, w + ": padding must be 0..64 per side");
    return 0;
}
// y355_conv_geom_out_size's rule (ops.hip geom_out)
static int geom_out(const char *who, const y355_convgrad_geom *g, int batch, int height, int width, int *ho, int *wo) {
    if (int rc = geom_limits(who, g)) return rc;
    const std::string w(who);
    if (batch < 1 || height < 1 || width < 1) return y355_fail(Y355_EINVAL, w + ": bad shape");
    const int hn = height + g->pad_top + g->pad_bottom - g->dil_h * (g->kh - 1) - 1;
    const int wn = width + g->pad_left + g->pad_right - g->dil_w * (g->kw - 1) - 1;
    if (hn < 0 || wn < 0) return y355_fail(Y355_EINVAL, w + ": the dilated kernel is larger than the padded input (Ho or Wo < 1)");
    *ho = hn / g->stride_h + 1;
    *wo = wn / g->stride_w + 1;
    if ((long long)batch * *ho * *wo > 0x7fffffffll || (long long)batch * (height + 2) * (width + 2) > 0x7fffffffll)
        return y355_fail(Y355_EINVAL, w + ": too many pixels");
    return 0;
}

// The split of npix = B Ho Wo pixels into runs of chunk pixels (a multiple of 32; the last run may be shorter), at most about
// 2048 waves of the weight gradient in all.  y355_convgrad_backward launches from it and y355_convgrad_wgrad_plan reports it.
struct WgradPlan {
    size_t npix, chunk, last;
    int runs, mt;
};
static int wgrad_mt(int cout) { return cout >= 64 ? 4 : (cout >= 32 ? 2 : 1); }
static WgradPlan wgrad_plan(const y355_convgrad *h, int B, int ho, int wo) {
    WgradPlan p;
    p.mt = wgrad_mt(h->cout);
    const size_t tiles = (size_t)((h->cin + 15) / 16) * ((h->cout + 16 * p.mt - 1) / (16 * p.mt)) * h->ntaps;
    const size_t max_runs = std::max<size_t>(1, 2048 / tiles);
    p.npix = (size_t)B * ho * wo;
    const size_t want = std::min<size_t>(max_runs, (p.npix + 31) / 32);
    p.chunk = ((p.npix + want - 1) / want + 31) / 32 * 32;
    p.runs = (int)((p.npix + p.chunk - 1) / p.chunk);
    p.last = p.npix - (size_t)(p.runs - 1) * p.chunk;
    return p;
}
static size_t wgrad_stride(const y355_convgrad *h) { return (size_t)h->cout * h->cin * h->ntaps + h->cout; }

// y355_convgrad_create in two parts, as the host check runs them on the CPU: the rules and the host state (no device call), ...
int convgrad_open(int device_id, int cin, int cout, const y355_convgrad_geom *g, float neg_slope, const DevMem &mem, y355_convgrad **out) {
    if (!out) return y355_fail(Y355_EINVAL, "y355_convgrad_create: null argument");
    *out = nullptr;
    if (device_id < 0) return y355_fail(Y355_EINVAL, "y355_convgrad_create: device_id must be >= 0");
    if (cin < 1 || cin > Y355_CONVGRAD_MAX_CHANNELS || cout < 1 || cout > Y355_CONVGRAD_MAX_CHANNELS)
        return y355_fail(Y355_EINVAL, "y355_convgrad_create: cin and cout must be 1..4096");
    if (int rc = geom_limits("y355_convgrad_create", g)) return rc;
    if (!(neg_slope >= 0.f) || !(neg_slope <= 3.0e38f)) return y355_fail(Y355_EINVAL, "y355_convgrad_create: neg_slope must be finite and >= 0");
    y355_convgrad *h = new y355_convgrad;
    h->own = DevOwner{mem, {}};
    h->device_id = device_id;
    h->cin = cin;
    h->cout = cout;
    h->cinp = (cin + 7) / 8 * 8;
    h->coutp = (cout + 7) / 8 * 8;
    h->g = *g;
    h->ntaps = g->kh * g->kw;
    h->slope = neg_slope;
    h->ct = tiles_per_wave(cout);
    h->dct = tiles_per_wave(cin);
    h->ksf = (h->ntaps * h->cinp + 31) / 32;
    h->ksd = (h->ntaps * h->coutp + 31) / 32;
    h->wf_n = pack_size(cout, h->ct, h->ksf);
    h->wd_n = pack_size(cin, h->dct, h->ksd);
    *out = h;
    return Y355_OK;
}
// ... the two packs (on the current device), both or neither, ...
int convgrad_buffers(y355_convgrad *h) {
    const size_t mark = y355_dev_mark(h->own);
    int rc = y355_dev_get(h->own, &h->wf, h->wf_n, true);
    rc = rc ? rc : y355_dev_get(h->own, &h->wd, h->wd_n, true);
    if (rc) {
        y355_dev_rollback(h->own, mark);
        h->wf = h->wd = nullptr;
    }
    return rc;
}
// ... and the workspaces of one call, grown where too small: rb(x) (forward, weight gradient), G and the runs (backward).  One
// that cannot grow is left null at capacity 0; the others stay.
int convgrad_workspaces(y355_convgrad *h, size_t xs_n, size_t gs_n, size_t ws_n) {
    int rc = xs_n ? y355_dev_grow(h->own, &h->xs_cap, xs_n, &h->xs) : 0;
    rc = rc || !gs_n ? rc : y355_dev_grow(h->own, &h->gs_cap, gs_n, &h->gs);
    rc = rc || !ws_n ? rc : y355_dev_grow(h->own, &h->ws_cap, ws_n, &h->ws);
    return rc;
}
DevOwner &convgrad_owner(y355_convgrad *h) { return h->own; }
void convgrad_caps(const y355_convgrad *h, size_t *caps) {
    caps[0] = h->xs ? h->xs_cap : 0;
    caps[1] = h->gs ? h->gs_cap : 0;
    caps[2] = h->ws ? h->ws_cap : 0;
    caps[3] = h->wf_n;
    caps[4] = h->wd_n;
}
void convgrad_free(y355_convgrad *h) {
    y355_dev_release_all(h->own);
    delete h;
}

// the shape of a pass: (Ho, Wo) and the staged sizes, refused where a staged tensor passes 2^36 elements
struct PassShape {
    int ho, wo;
    size_t npix_in, npix_out;
};
static int pass_shape(const char *who, const y355_convgrad *h, int batch, int height, int width, PassShape *s) {
    if (int rc = geom_out(who, &h->g, batch, height, width, &s->ho, &s->wo)) return rc;
    s->npix_in = (size_t)batch * height * width;
    s->npix_out = (size_t)batch * s->ho * s->wo;
    if (s->npix_in * h->cinp > ((size_t)1 << 36) || s->npix_out * h->coutp > ((size_t)1 << 36))
        return y355_fail(Y355_EINVAL, std::string(who) + ": tensor too large");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------- launches
static hipError_t launch_stage(const float *src, const float *y, float slope, bf16_t *dst, size_t npix, size_t hw, int c, int cp, hipStream_t s) {
    const size_t n = npix * (size_t)(cp / 8);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (y) hipLaunchKernelGGL((cg_stage_kernel<true>), grid, block, 0, s, src, y, slope, dst, npix, hw, c, cp);
    else hipLaunchKernelGGL((cg_stage_kernel<false>), grid, block, 0, s, src, (const float *)nullptr, 1.0f, dst, npix, hw, c, cp);
    return hipGetLastError();
}
static hipError_t launch_pack(const y355_convgrad *h, const float *w, bool dgrad, hipStream_t s) {
    PackArgs a{};
    a.n = dgrad ? h->wd_n : h->wf_n;
    a.ks = dgrad ? h->ksd : h->ksf;
    a.rows = dgrad ? h->cin : h->cout;
    a.kc = dgrad ? h->cout : h->cin;
    a.kcp = dgrad ? h->coutp : h->cinp;
    a.ntaps = h->ntaps;
    a.cin = h->cin;
    const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    if (dgrad) hipLaunchKernelGGL((cg_pack_kernel<true>), grid, block, 0, s, w, h->wd, a);
    else hipLaunchKernelGGL((cg_pack_kernel<false>), grid, block, 0, s, w, h->wf, a);
    return hipGetLastError();
}
template <bool DGRAD>
static hipError_t launch_conv(const y355_convgrad *h, const float *bias, float *out, int B, int height, int width, int ho, int wo, hipStream_t s) {
    ConvArgs a{};
    a.in = DGRAD ? h->gs : h->xs;
    a.w = DGRAD ? h->wd : h->wf;
    a.bias = bias;
    a.out = out;
    a.slope = DGRAD ? 1.0f : h->slope;
    a.cp = DGRAD ? h->coutp : h->cinp;
    a.ks = DGRAD ? h->ksd : h->ksf;
    a.B = B;
    a.hin = DGRAD ? ho : height;
    a.win = DGRAD ? wo : width;
    a.hout = DGRAD ? height : ho;
    a.wout = DGRAD ? width : wo;
    a.c = DGRAD ? h->cin : h->cout;
    a.kh = h->g.kh, a.kw = h->g.kw, a.sh = h->g.stride_h, a.sw = h->g.stride_w, a.dh = h->g.dil_h, a.dw = h->g.dil_w;
    a.pt = h->g.pad_top, a.pl = h->g.pad_left;
    const int ct = DGRAD ? h->dct : h->ct, tiles = (a.c + 15) / 16;
    const size_t waves = ((size_t)B * a.hout * a.wout + 63) / 64;
    const dim3 grid((unsigned)((waves + 3) / 4), (unsigned)((tiles + ct - 1) / ct)), block(256);
    if (ct == 1) hipLaunchKernelGGL((cg_conv_kernel<DGRAD, 1>), grid, block, 0, s, a);
    else if (ct == 2) hipLaunchKernelGGL((cg_conv_kernel<DGRAD, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((cg_conv_kernel<DGRAD, 4>), grid, block, 0, s, a);
    return hipGetLastError();
}
static hipError_t launch_wgrad(const y355_convgrad *h, const WgradPlan &plan, int height, int width, int ho, int wo, float *dw, float *db, hipStream_t s) {
    WgradArgs a{};
    a.g = h->gs;
    a.x = h->xs;
    a.ws = h->ws;
    a.ws_stride = wgrad_stride(h);
    a.npix = plan.npix;
    a.chunk = plan.chunk;
    a.h = height, a.w = width, a.ho = ho, a.wo = wo;
    a.cin = h->cin, a.cinp = h->cinp, a.cout = h->cout, a.coutp = h->coutp;
    a.kw = h->g.kw, a.ntaps = h->ntaps, a.sh = h->g.stride_h, a.sw = h->g.stride_w, a.dh = h->g.dil_h, a.dw = h->g.dil_w;
    a.pt = h->g.pad_top, a.pl = h->g.pad_left;
    a.ci_tiles = (h->cin + 15) / 16;
    const dim3 grid((unsigned)(a.ci_tiles * h->ntaps), (unsigned)((h->cout + 16 * plan.mt - 1) / (16 * plan.mt)), (unsigned)plan.runs), block(64);
    if (plan.mt == 1) hipLaunchKernelGGL((cg_wgrad_kernel<1>), grid, block, 0, s, a);
    else if (plan.mt == 2) hipLaunchKernelGGL((cg_wgrad_kernel<2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((cg_wgrad_kernel<4>), grid, block, 0, s, a);
    if (const hipError_t e = hipGetLastError()) return e;
    const size_t nw = (size_t)h->cout * h->cin * h->ntaps, nb = (size_t)h->cout;
    hipLaunchKernelGGL(cg_reduce_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, h->ws, a.ws_stride, plan.runs, nw, nb, dw, db);
    return hipGetLastError();
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_convgrad_last_error(void) { return g_err.c_str(); }

int y355_convgrad_out_size(const y355_convgrad_geom *g, int32_t height, int32_t width, int32_t *ho, int32_t *wo) {
    if (!ho || !wo) return y355_fail(Y355_EINVAL, "y355_convgrad_out_size: null argument");
    return geom_out("y355_convgrad_out_size", g, 1, height, width, ho, wo);
}

int y355_convgrad_create(int32_t device_id, int32_t cin, int32_t cout, const y355_convgrad_geom *g, float neg_slope, y355_convgrad **out) {
    if (int rc = convgrad_open(device_id, cin, cout, g, neg_slope, y355_hip_mem(), out)) return rc;
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    int rc = e != hipSuccess ? y355_fail(Y355_EHIP, std::string("y355_convgrad_create: ") + hipGetErrorString(e))
                             : (device_id >= count ? y355_fail(Y355_EINVAL, "y355_convgrad_create: no such device") : 0);
    if (!rc) {
        DeviceGuard gd;
        const hipError_t es = gd.set(device_id);
        rc = es != hipSuccess ? y355_fail(Y355_EHIP, std::string("y355_convgrad_create: ") + hipGetErrorString(es)) : convgrad_buffers(*out);
    }
    if (rc) {
        convgrad_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_convgrad_destroy(y355_convgrad *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->device_id);
    convgrad_free(h);
}

int y355_convgrad_wgrad_plan(const y355_convgrad *h, int32_t batch, int32_t height, int32_t width, int32_t *out) {
    if (!h || !out) return y355_fail(Y355_EINVAL, "y355_convgrad_wgrad_plan: null argument");
    PassShape ps;
    if (int rc = pass_shape("y355_convgrad_wgrad_plan", h, batch, height, width, &ps)) return rc;
    const WgradPlan p = wgrad_plan(h, batch, ps.ho, ps.wo);
    out[0] = (int32_t)p.npix;
    out[1] = p.runs;
    out[2] = (int32_t)p.chunk;
    out[3] = (int32_t)p.last;
    return Y355_CONVGRAD_OK;
}

int y355_convgrad_forward(y355_convgrad *h, const void *x_dev, const void *w_dev, const void *bias_dev, int32_t batch, int32_t height,
                          int32_t width, void *y_dev, void *stream) {
    if (!h || !x_dev || !w_dev || !y_dev) return y355_fail(Y355_EINVAL, "y355_convgrad_forward: null argument");
    PassShape ps;
    if (int rc = pass_shape("y355_convgrad_forward", h, batch, height, width, &ps)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    if (int rc = convgrad_workspaces(h, ps.npix_in * h->cinp, 0, 0)) return rc;
    HIPCHK(launch_stage((const float *)x_dev, nullptr, 1.0f, h->xs, ps.npix_in, (size_t)height * width, h->cin, h->cinp, s));
    HIPCHK(launch_pack(h, (const float *)w_dev, false, s));
    HIPCHK(launch_conv<false>(h, (const float *)bias_dev, (float *)y_dev, batch, height, width, ps.ho, ps.wo, s));
    return Y355_CONVGRAD_OK;
}

int y355_convgrad_backward(y355_convgrad *h, const void *x_dev, const void *w_dev, const void *y_dev, const void *dy_dev, int32_t batch,
                           int32_t height, int32_t width, void *dx_dev, void *dw_dev, void *db_dev, void *stream) {
    if (!h || !x_dev || !w_dev || !dy_dev) return y355_fail(Y355_EINVAL, "y355_convgrad_backward: null argument");
    if (!y_dev && h->slope != 1.0f) return y355_fail(Y355_EINVAL, "y355_convgrad_backward: y is needed unless neg_slope is 1");
    PassShape ps;
    if (int rc = pass_shape("y355_convgrad_backward", h, batch, height, width, &ps)) return rc;
    if (!dx_dev && !dw_dev && !db_dev) return Y355_CONVGRAD_OK;
    const bool want_w = dw_dev || db_dev;
    const WgradPlan plan = wgrad_plan(h, batch, ps.ho, ps.wo);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    if (int rc = convgrad_workspaces(h, want_w ? ps.npix_in * h->cinp : 0, ps.npix_out * h->coutp, want_w ? (size_t)plan.runs * wgrad_stride(h) : 0))
        return rc;
    HIPCHK(launch_stage((const float *)dy_dev, h->slope != 1.0f ? (const float *)y_dev : nullptr, h->slope, h->gs, ps.npix_out,
                        (size_t)ps.ho * ps.wo, h->cout, h->coutp, s));
    if (dx_dev) {
        HIPCHK(launch_pack(h, (const float *)w_dev, true, s));
        HIPCHK(launch_conv<true>(h, nullptr, (float *)dx_dev, batch, height, width, ps.ho, ps.wo, s));
    }
    if (want_w) {
        HIPCHK(launch_stage((const float *)x_dev, nullptr, 1.0f, h->xs, ps.npix_in, (size_t)height * width, h->cin, h->cinp, s));
        HIPCHK(launch_wgrad(h, plan, height, width, ps.ho, ps.wo, (float *)dw_dev, (float *)db_dev, s));
    }
    return Y355_CONVGRAD_OK;
}

}  // extern "C"
