// yolo355 -- the element-wise ops between the convolutions of the y355_net graphs (net.hip): max-pool, bilinear x2, reorg,
// SPP and the network input, each in a bf16 and an int8 form, and the maxima of a calibration step.  Every tensor is NHWC
// with a one-pixel zero halo, [B][H + 2][W + 2][pb bytes]; a launcher owns its grid size.
#include "y355_common.h"

#include <algorithm>

namespace {
// byte offset of pixel (b, y, x) of a halo'd tensor of H x W pixels of pb bytes
__device__ __forceinline__ size_t px_off(size_t b, int H, int W, int y, int x, int pb) {
    return ((b * (H + 2) + y + 1) * (size_t)(W + 2) + x + 1) * pb;
}

// flat work-item index -> (c, x, y, b), c fastest: i = ((b * H + y) * W + x) * C + c
struct Item { int c, x, y; size_t b; };
__device__ __forceinline__ Item item_of(size_t i, int C, int W, int H) {
    Item it;
    it.c = (int)(i % C);
    size_t r = i / C;
    it.x = (int)(r % W);
    r /= W;
    it.y = (int)(r % H);
    it.b = r / H;
    return it;
}

// F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) (models/tiny_yolo_v3.py:188):
// src = dst * (in - 1) / (out - 1), the two-tap blend of torch's upsample_bilinear2d in fp32.
struct Bilin { int y0, x0, y1, x1; float ly, lx, hy, hx; };
__device__ __forceinline__ Bilin bilin_taps(int y, int x, int Hin, int Win, float ry, float rx) {
    Bilin t;
    const float sy = ry * (float)y, sx = rx * (float)x;
    t.y0 = (int)sy;
    t.x0 = (int)sx;
    t.y1 = min(t.y0 + 1, Hin - 1);
    t.x1 = min(t.x0 + 1, Win - 1);
    t.ly = sy - (float)t.y0;
    t.lx = sx - (float)t.x0;
    t.hy = 1.f - t.ly;
    t.hx = 1.f - t.lx;
    return t;
}
__device__ __forceinline__ float bilin_blend(const Bilin &t, float f00, float f01, float f10, float f11) {
    return t.hy * (t.hx * f00 + t.lx * f01) + t.ly * (t.hx * f10 + t.lx * f11);
}

// one pixel of uint8 HWC BGR frames [B][sh][sw][3] as the H x W network input sees it: resized on the fly when tab != null
// (y355_resize_px), else the frames are at the network size
__device__ __forceinline__ void bgr_px(const uint8_t *frames, const int *tab, size_t b, int sh, int sw, int H, int W, int y, int x,
                                       int u[3]) {
    if (tab) {
        y355_resize_px(frames + b * sh * sw * 3, tab, sh, sw, H, W, y, x, u);
    } else {
        const uint8_t *px = frames + ((b * H + y) * W + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = px[c];
    }
}

__device__ __forceinline__ int grid_stride() { return gridDim.x * blockDim.x; }
__device__ __forceinline__ size_t grid_first() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

// element-wise max of four 16-byte groups: 8 bf16 channels (compared as fp32) or 16 int8 channels
template <bool BF>
__device__ __forceinline__ uint4 max4x16(const uint4 (&v)[4]) {
    unsigned int o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int w[4] = {((const unsigned int *)&v[0])[k], ((const unsigned int *)&v[1])[k], ((const unsigned int *)&v[2])[k],
                                   ((const unsigned int *)&v[3])[k]};
        unsigned int res = 0;
        if constexpr (BF) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int sh = 16 * hf;
                const float a = __uint_as_float(((w[0] >> sh) & 0xffffu) << 16), bb = __uint_as_float(((w[1] >> sh) & 0xffffu) << 16);
                const float cc = __uint_as_float(((w[2] >> sh) & 0xffffu) << 16), d = __uint_as_float(((w[3] >> sh) & 0xffffu) << 16);
                const float m = fmaxf(fmaxf(a, bb), fmaxf(cc, d));
                res |= (__float_as_uint(m) >> 16) << sh;
            }
        } else {
#pragma unroll
            for (int by = 0; by < 4; ++by) {
                int m = -128;
#pragma unroll
                for (int j = 0; j < 4; ++j) m = max(m, (int)(signed char)((w[j] >> (8 * by)) & 0xffu));
                res |= (unsigned int)(m & 0xff) << (8 * by);
            }
        }
        o[k] = res;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// 2x2 max-pool, stride 1 or 2: 16 bytes of one output pixel per thread; the zero halo IS the padding
template <bool BF>
__global__ void pool_kernel(const char *in, char *out, int B, int Hin, int Win, int in_pb, int cbytes, int Ho, int Wo, int out_pb,
                            int stride) {
    const int cg = cbytes / 16;
    const size_t total = (size_t)B * Ho * Wo * cg;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, cg, Wo, Ho);
        const char *src = in + px_off(it.b, Hin, Win, it.y * stride, it.x * stride, in_pb) + it.c * 16;
        uint4 v[4];
        v[0] = *(const uint4 *)src;
        v[1] = *(const uint4 *)(src + in_pb);
        v[2] = *(const uint4 *)(src + (size_t)(Win + 2) * in_pb);
        v[3] = *(const uint4 *)(src + (size_t)(Win + 2) * in_pb + in_pb);
        *(uint4 *)(out + px_off(it.b, Ho, Wo, it.y, it.x, out_pb) + it.c * 16) = max4x16<BF>(v);
    }
}

__global__ void upsample_bf16_kernel(const char *in, char *out, int B, int Hin, int Win, int in_pb, int C, int out_pb, int out_off,
                                     float ry, float rx) {
    const int Ho = 2 * Hin, Wo = 2 * Win;
    const size_t total = (size_t)B * Ho * Wo * C;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, C, Wo, Ho);
        const Bilin t = bilin_taps(it.y, it.x, Hin, Win, ry, rx);
        auto ld = [&](int yy, int xx) -> float {
            const unsigned short h = *(const unsigned short *)(in + px_off(it.b, Hin, Win, yy, xx, in_pb) + it.c * 2);
            return __uint_as_float((unsigned int)h << 16);
        };
        const float v = bilin_blend(t, ld(t.y0, t.x0), ld(t.y0, t.x1), ld(t.y1, t.x0), ld(t.y1, t.x1));
        *(unsigned short *)(out + px_off(it.b, Ho, Wo, it.y, it.x, out_pb) + out_off + it.c * 2) =
            __builtin_bit_cast(unsigned short, (__bf16)v);
    }
}

// int8 form of the bilinear x2: the blend of the integer values in fp32 (same expression as the bf16 kernel), rescaled by
// the power of two between the two tensors' exponents, rounded half-to-even.  Sixteen channels of one output pixel per
// thread (16-byte loads and stores; C % 16 == 0, 16-byte aligned pixels, fewer than 2^31 items: y355_upsample_i8_ok)
__global__ void upsample_i8_kernel(const char *in, char *out, int B, int Hin, int Win, int in_pb, int C, int out_pb, int out_off,
                                   float ry, float rx, float rescale) {
    const int Ho = 2 * Hin, Wo = 2 * Win, CG = C / 16;
    const int total = B * Ho * Wo * CG;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += grid_stride()) {
        const int cg = i % CG;
        int r = i / CG;
        const int x = r % Wo;
        r /= Wo;
        const int y = r % Ho;
        const int b = r / Ho;
        const Bilin t = bilin_taps(y, x, Hin, Win, ry, rx);
        auto ld = [&](int yy, int xx) { return *(const v4i *)(in + px_off(b, Hin, Win, yy, xx, in_pb) + cg * 16); };
        const v4i a00 = ld(t.y0, t.x0), a01 = ld(t.y0, t.x1), a10 = ld(t.y1, t.x0), a11 = ld(t.y1, t.x1);
        v4i o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned int word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = bilin_blend(t, (float)(signed char)(a00[w] >> (8 * k)), (float)(signed char)(a01[w] >> (8 * k)),
                                            (float)(signed char)(a10[w] >> (8 * k)), (float)(signed char)(a11[w] >> (8 * k)));
                const float q = fminf(fmaxf(rintf(v * rescale), -127.f), 127.f);
                word |= ((unsigned int)(int)q & 0xffu) << (8 * k);
            }
            o[w] = (int)word;
        }
        *(v4i *)(out + px_off(b, Ho, Wo, y, x, out_pb) + out_off + cg * 16) = o;
    }
}

// ---- int8 ops of the DarkNet graphs (DESIGN.md "int8 DarkNet"); clamps count into the op's counter
__device__ __forceinline__ void count_sat(Counters *ctr, unsigned int n) {
    if (n && ctr) atomicAdd(&ctr->sat, (unsigned long long)n);
}

// q_in * 2^d, rounded half-to-even (d < 0), clamped to +-127: the rescale between two tensors' exponents
__device__ __forceinline__ int rescale_i8(int q, int d, unsigned int &nsat) {
    const int r = d >= 0 ? q * (1 << min(d, 24)) : y355_rne_shift32(q, -d);
    const int c = y355_clamp8<int>(r);
    nsat += c != r ? 1u : 0u;
    return c;
}

// fp32 NCHW [B][3][H][W] -> bf16 NHWC16 with halo (channels 3..15 stay zero)
__global__ void input_bf16_kernel(const float *x, char *out, int B, int H, int W, int out_pb) {
    const size_t total = (size_t)B * H * W;
    const size_t plane = (size_t)H * W;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, 1, W, H);
        const float *src = x + it.b * 3 * plane + (size_t)it.y * W + it.x;
        unsigned short h3[4] = {__builtin_bit_cast(unsigned short, (__bf16)src[0]), __builtin_bit_cast(unsigned short, (__bf16)src[plane]),
                                __builtin_bit_cast(unsigned short, (__bf16)src[2 * plane]), 0};
        uint2 u;
        u.x = (unsigned int)h3[0] | ((unsigned int)h3[1] << 16);
        u.y = (unsigned int)h3[2];
        *(uint2 *)(out + px_off(it.b, H, W, it.y, it.x, out_pb)) = u;
    }
}

// fp32 NCHW [B][3][H][W] -> int8 NHWC32 with halo: q = clamp(RNE(x * 2^sa_in)) (the slim front end's input rule); one pixel
// per thread, one 16-byte store (channels 3..15 zero; 16..31 keep the allocation's zeros)
__global__ void input_i8_kernel(const float *x, char *out, int B, int H, int W, int out_pb, float in_scale, Counters *ctr) {
    const size_t total = (size_t)B * H * W;
    const size_t plane = (size_t)H * W;
    unsigned int nsat = 0;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, 1, W, H);
        const float *src = x + it.b * 3 * plane + (size_t)it.y * W + it.x;
        unsigned int w = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r = rintf(src[c * plane] * in_scale);
            const float q = fminf(fmaxf(r, -127.f), 127.f);
            nsat += q != r ? 1u : 0u;
            w |= ((unsigned int)(int)q & 0xffu) << (8 * c);
        }
        *(uint4 *)(out + px_off(it.b, H, W, it.y, it.x, out_pb)) = make_uint4(w, 0u, 0u, 0u);
    }
    count_sat(ctr, nsat);
}

// uint8 HWC BGR frames [B][sh][sw][3] -> the network input tensor with halo, bf16 NHWC16 (I8 = false) or int8 NHWC32 (I8):
// cv2.resize to the network size fused into the load when the frame is not at it (bgr_px), then BaseTransform + BGR->RGB
// through a per-channel byte table in LDS that holds what input_bf16_kernel / input_i8_kernel make of the normalised fp32
// value -- its bf16 (RNE), or clamp(RNE(x * 2^sa_in)) with bit 8 = "was clamped" (counted into ctr as input_i8_kernel
// counts).  One pixel per thread, one 16-byte store (bf16: channels 3..7 zero; int8: 3..15 zero; the rest of the pixel keeps
// the allocation's zeros).
template <bool I8>
__global__ __launch_bounds__(256) void input_u8_kernel(const uint8_t *frames, const int *tab, char *out, int B, int sh, int sw, int H,
                                                       int W, int out_pb, NormU8 nm, float in_scale, Counters *ctr) {
    __shared__ unsigned short lut[3 * 256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = y355_norm_u8(tid, nm.mean[c], nm.sd[c]);
        if constexpr (I8) {
            const float r = rintf(t * in_scale);
            const float q = fminf(fmaxf(r, -127.f), 127.f);
            lut[c * 256 + tid] = (unsigned short)(((int)q & 0xff) | (q != r ? 0x100 : 0));
        } else {
            lut[c * 256 + tid] = __builtin_bit_cast(unsigned short, (__bf16)t);
        }
    }
    __syncthreads();
    const size_t total = (size_t)B * H * W;
    unsigned int nsat = 0;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, 1, W, H);
        int u[3];
        bgr_px(frames, tab, it.b, sh, sw, H, W, it.y, it.x, u);
        // RGB channel c = BGR byte 2 - c
        const unsigned int e0 = lut[u[2]], e1 = lut[256 + u[1]], e2 = lut[512 + u[0]];
        uint4 v;
        if constexpr (I8) {
            nsat += ((e0 >> 8) & 1u) + ((e1 >> 8) & 1u) + ((e2 >> 8) & 1u);
            v = make_uint4((e0 & 0xffu) | ((e1 & 0xffu) << 8) | ((e2 & 0xffu) << 16), 0u, 0u, 0u);
        } else {
            v = make_uint4(e0 | (e1 << 16), e2, 0u, 0u);
        }
        *(uint4 *)(out + px_off(it.b, H, W, it.y, it.x, out_pb)) = v;
    }
    if constexpr (I8) count_sat(ctr, nsat);
}

// utils.modules.reorg_layer (utils/modules.py:48-57) on NHWC into a concat buffer: out[.., (sy*s+sx)*C + c] =
// in[s*y+sy][s*x+sx][c]; 16 bytes per thread (8 bf16 / 16 int8 channels).  int8 (I8): with the rescale 2^d, d = s_out - s_in
template <bool I8>
__global__ void reorg_kernel(const char *in, char *out, int B, int Hin, int Win, int in_pb, int C, int out_pb, int out_off, int s, int d,
                             Counters *ctr) {
    const int es = I8 ? 1 : 2;
    const int Ho = Hin / s, Wo = Win / s, cg = C * es / 16;
    const size_t total = (size_t)B * Ho * Wo * s * s * cg;
    unsigned int nsat = 0;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, cg * s * s, Wo, Ho);
        const int g = it.c % cg, k = it.c / cg;
        const uint4 v = *(const uint4 *)(in + px_off(it.b, Hin, Win, s * it.y + k / s, s * it.x + k % s, in_pb) + g * 16);
        unsigned int u[4] = {v.x, v.y, v.z, v.w};
        if (I8 && d != 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned int o = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    o |= ((unsigned int)rescale_i8((int)(signed char)((u[w] >> (8 * j)) & 0xffu), d, nsat) & 0xffu) << (8 * j);
                u[w] = o;
            }
        }
        *(uint4 *)(out + px_off(it.b, Ho, Wo, it.y, it.x, out_pb) + out_off + ((size_t)k * C * es + g * 16)) =
            make_uint4(u[0], u[1], u[2], u[3]);
    }
    if (I8) count_sat(ctr, nsat);
}

// utils.modules.SPP (utils/modules.py:66-72) on bf16 NHWC, in place in a 4C-channel buffer: channels [0, C) are x, the
// kernel writes max_pool 5 / 9 / 13 (stride 1, windows clipped to the map = -inf padding) to [C,2C), [2C,3C), [3C,4C).
// bf16 compares as fp32; 8 channels (16 bytes) per thread.
__global__ void spp_bf16_kernel(char *buf, int B, int H, int W, int pb, int C) {
    const int cg = C / 8;
    const size_t total = (size_t)B * H * W * cg;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, cg, W, H);
        float m5[8], m9[8], m13[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) m5[k] = m9[k] = m13[k] = -INFINITY;
        for (int dy = -6; dy <= 6; ++dy) {
            const int yy = it.y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -6; dx <= 6; ++dx) {
                const int xx = it.x + dx;
                if (xx < 0 || xx >= W) continue;
                const uint4 v = *(const uint4 *)(buf + px_off(it.b, H, W, yy, xx, pb) + it.c * 16);
                const unsigned int u[4] = {v.x, v.y, v.z, v.w};
                const int r = max(abs(dy), abs(dx));
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float f = __uint_as_float((k & 1) ? (u[k >> 1] & 0xffff0000u) : (u[k >> 1] << 16));
                    m13[k] = fmaxf(m13[k], f);
                    if (r <= 4) m9[k] = fmaxf(m9[k], f);
                    if (r <= 2) m5[k] = fmaxf(m5[k], f);
                }
            }
        }
        char *o = buf + px_off(it.b, H, W, it.y, it.x, pb) + it.c * 16;
        auto pack = [](const float (&m)[8]) {
            uint4 r;
            unsigned int w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (__float_as_uint(m[2 * k]) >> 16) | (__float_as_uint(m[2 * k + 1]) & 0xffff0000u);
            r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
            return r;
        };
        *(uint4 *)(o + (size_t)C * 2) = pack(m5);
        *(uint4 *)(o + (size_t)C * 4) = pack(m9);
        *(uint4 *)(o + (size_t)C * 6) = pack(m13);
    }
}

// the same on int8 NHWC: exact on the int8 values, no requantisation (the padding takes part in no max).  16 channels
// (16 bytes) per thread.
__global__ void spp_i8_kernel(char *buf, int B, int H, int W, int pb, int C) {
    const int cg = C / 16;
    const size_t total = (size_t)B * H * W * cg;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, cg, W, H);
        int m5[16], m9[16], m13[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m5[k] = m9[k] = m13[k] = -128;
        for (int dy = -6; dy <= 6; ++dy) {
            const int yy = it.y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -6; dx <= 6; ++dx) {
                const int xx = it.x + dx;
                if (xx < 0 || xx >= W) continue;
                const uint4 v = *(const uint4 *)(buf + px_off(it.b, H, W, yy, xx, pb) + it.c * 16);
                const unsigned int u[4] = {v.x, v.y, v.z, v.w};
                const int r = max(abs(dy), abs(dx));
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int f = (int)(signed char)((u[k >> 2] >> (8 * (k & 3))) & 0xffu);
                    m13[k] = max(m13[k], f);
                    if (r <= 4) m9[k] = max(m9[k], f);
                    if (r <= 2) m5[k] = max(m5[k], f);
                }
            }
        }
        char *o = buf + px_off(it.b, H, W, it.y, it.x, pb) + it.c * 16;
        auto pack = [](const int (&m)[16]) {
            unsigned int w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k >> 2] |= ((unsigned int)m[k] & 0xffu) << (8 * (k & 3));
            return make_uint4(w[0], w[1], w[2], w[3]);
        };
        *(uint4 *)(o + (size_t)C) = pack(m5);
        *(uint4 *)(o + (size_t)C * 2) = pack(m9);
        *(uint4 *)(o + (size_t)C * 3) = pack(m13);
    }
}

// ---- maxima: each reduces within the wave and issues one atomicMax per wave on the bits of a non-negative fp32 / on an
// unsigned int; nothing else is written
__global__ void absmax_bf16_kernel(const char *t, size_t n_elems, unsigned int *out) {
    float m = 0.f;
    for (size_t i = grid_first(); i < n_elems; i += (size_t)grid_stride()) {
        const unsigned short h = ((const unsigned short *)t)[i];
        m = fmaxf(m, fabsf(__uint_as_float((unsigned int)h << 16)));
    }
    const unsigned int u = y355_wave_max_u32(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0) atomicMax(out, u);
}

// bilinear x2 (y355_net_calibrate): max |blend| of upsample_i8_kernel's fp32 expression, before the rescale
__global__ void upsample_i8_max_kernel(const char *in, int B, int Hin, int Win, int in_pb, int C, float ry, float rx, unsigned int *out) {
    const int Ho = 2 * Hin, Wo = 2 * Win;
    const size_t total = (size_t)B * Ho * Wo * C;
    float m = 0.f;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, C, Wo, Ho);
        const Bilin t = bilin_taps(it.y, it.x, Hin, Win, ry, rx);
        auto ld = [&](int yy, int xx) -> float { return (float)*(const signed char *)(in + px_off(it.b, Hin, Win, yy, xx, in_pb) + it.c); };
        m = fmaxf(m, fabsf(bilin_blend(t, ld(t.y0, t.x0), ld(t.y0, t.x1), ld(t.y1, t.x0), ld(t.y1, t.x1))));
    }
    const unsigned int u = y355_wave_max_u32(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0 && u) atomicMax(out, u);
}

// max |q| over the first C channels of an int8 tensor's interior (reorg's source bytes)
__global__ void absmax_i8_kernel(const char *in, int B, int H, int W, int pb, int C, unsigned int *out) {
    const size_t total = (size_t)B * H * W * C;
    unsigned int m = 0;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, C, W, H);
        const int q = (int)*(const signed char *)(in + px_off(it.b, H, W, it.y, it.x, pb) + it.c);
        m = max(m, (unsigned int)abs(q));
    }
    const unsigned int u = y355_wave_max_u32(m);
    if ((threadIdx.x & 63) == 0 && u) atomicMax(out, u);
}

// max |x| of the normalised frames (the table entries y355_norm_u8 the H x W network input actually hits), read as
// input_u8_kernel reads them
__global__ __launch_bounds__(256) void absmax_u8_kernel(const uint8_t *frames, const int *tab, int B, int sh, int sw, int H, int W,
                                                        NormU8 nm, unsigned int *out) {
    const size_t total = (size_t)B * H * W;
    float m = 0.f;
    for (size_t i = grid_first(); i < total; i += (size_t)grid_stride()) {
        const Item it = item_of(i, 1, W, H);
        int u[3];
        bgr_px(frames, tab, it.b, sh, sw, H, W, it.y, it.x, u);
#pragma unroll
        for (int c = 0; c < 3; ++c) m = fmaxf(m, fabsf(y355_norm_u8(u[2 - c], nm.mean[c], nm.sd[c])));     // RGB c = BGR byte 2 - c
    }
    const unsigned int bits = y355_wave_max_u32(__float_as_uint(m));
    if ((threadIdx.x & 63) == 0 && bits) atomicMax(out, bits);
}

// 256-thread blocks for `total` grid-stride items, at most `cap`
dim3 blocks_for(size_t total, size_t cap) { return dim3((unsigned int)std::min<size_t>((total + 255) / 256, cap)); }
// align_corners ratio of the bilinear x2 along an axis of n input pixels
float up_ratio(int n) { return (float)(n - 1) / (float)(2 * n - 1); }
}  // namespace

void y355_launch_pool(bool bf, const NetMap &in, const NetMap &out, int B, int cbytes, int stride, hipStream_t s) {
    const dim3 grid = blocks_for((size_t)B * out.H * out.W * (cbytes / 16), 4096);
    if (bf)
        hipLaunchKernelGGL(pool_kernel<true>, grid, dim3(256), 0, s, in.dev, out.dev, B, in.H, in.W, in.pb, cbytes, out.H, out.W, out.pb, stride);
    else
        hipLaunchKernelGGL(pool_kernel<false>, grid, dim3(256), 0, s, in.dev, out.dev, B, in.H, in.W, in.pb, cbytes, out.H, out.W, out.pb, stride);
}

bool y355_upsample_i8_ok(const NetMap &in, const NetMap &out, int B, int C, int out_off) {
    return C % 16 == 0 && in.pb % 16 == 0 && out.pb % 16 == 0 && out_off % 16 == 0 && (long long)B * out.H * out.W * (C / 16) < (1ll << 31);
}

void y355_launch_upsample(bool bf, const NetMap &in, const NetMap &out, int B, int C, int out_off, float rescale, hipStream_t s) {
    const float ry = up_ratio(in.H), rx = up_ratio(in.W);
    if (bf)
        hipLaunchKernelGGL(upsample_bf16_kernel, blocks_for((size_t)B * out.H * out.W * C, 8192), dim3(256), 0, s, in.dev, out.dev, B, in.H,
                           in.W, in.pb, C, out.pb, out_off, ry, rx);
    else
        hipLaunchKernelGGL(upsample_i8_kernel, dim3((B * out.H * out.W * (C / 16) + 255) / 256), dim3(256), 0, s, in.dev, out.dev, B, in.H,
                           in.W, in.pb, C, out.pb, out_off, ry, rx, rescale);
}

void y355_launch_reorg(bool bf, const NetMap &in, const NetMap &out, int B, int C, int out_off, int stride, int d, Counters *ctr,
                       hipStream_t s) {
    const dim3 grid = blocks_for((size_t)B * out.H * out.W * stride * stride * (C / (bf ? 8 : 16)), 8192);
    if (bf)
        hipLaunchKernelGGL(reorg_kernel<false>, grid, dim3(256), 0, s, in.dev, out.dev, B, in.H, in.W, in.pb, C, out.pb, out_off, stride, 0,
                           (Counters *)nullptr);
    else
        hipLaunchKernelGGL(reorg_kernel<true>, grid, dim3(256), 0, s, in.dev, out.dev, B, in.H, in.W, in.pb, C, out.pb, out_off, stride, d, ctr);
}

void y355_launch_spp(bool bf, const NetMap &t, int B, int C, hipStream_t s) {
    const dim3 grid = blocks_for((size_t)B * t.H * t.W * (C / (bf ? 8 : 16)), 8192);
    if (bf) hipLaunchKernelGGL(spp_bf16_kernel, grid, dim3(256), 0, s, t.dev, B, t.H, t.W, t.pb, C);
    else hipLaunchKernelGGL(spp_i8_kernel, grid, dim3(256), 0, s, t.dev, B, t.H, t.W, t.pb, C);
}

void y355_launch_input(bool bf, const float *x, const uint8_t *u8, const int *tab, int sh, int sw, const NormU8 &nm, const NetMap &out,
                       int B, float in_scale, Counters *ctr, hipStream_t s) {
    const dim3 grid = blocks_for((size_t)B * out.H * out.W, 8192);
    if (u8 && bf)
        hipLaunchKernelGGL(input_u8_kernel<false>, grid, dim3(256), 0, s, u8, tab, out.dev, B, sh, sw, out.H, out.W, out.pb, nm, 1.0f,
                           (Counters *)nullptr);
    else if (u8)
        hipLaunchKernelGGL(input_u8_kernel<true>, grid, dim3(256), 0, s, u8, tab, out.dev, B, sh, sw, out.H, out.W, out.pb, nm, in_scale, ctr);
    else if (bf)
        hipLaunchKernelGGL(input_bf16_kernel, grid, dim3(256), 0, s, x, out.dev, B, out.H, out.W, out.pb);
    else
        hipLaunchKernelGGL(input_i8_kernel, grid, dim3(256), 0, s, x, out.dev, B, out.H, out.W, out.pb, in_scale, ctr);
}

void y355_launch_absmax_bf16(const char *t, size_t n_elems, unsigned int *out_bits, hipStream_t s) {
    hipLaunchKernelGGL(absmax_bf16_kernel, dim3(1024), dim3(256), 0, s, t, n_elems, out_bits);
}

void y355_launch_upsample_i8_max(const NetMap &in, int B, int C, unsigned int *out_bits, hipStream_t s) {
    hipLaunchKernelGGL(upsample_i8_max_kernel, blocks_for((size_t)B * 2 * in.H * 2 * in.W * C, 8192), dim3(256), 0, s, in.dev, B, in.H, in.W,
                       in.pb, C, up_ratio(in.H), up_ratio(in.W), out_bits);
}

void y355_launch_absmax_i8(const NetMap &in, int B, int C, unsigned int *out, hipStream_t s) {
    hipLaunchKernelGGL(absmax_i8_kernel, blocks_for((size_t)B * in.H * in.W * C, 8192), dim3(256), 0, s, in.dev, B, in.H, in.W, in.pb, C, out);
}

void y355_launch_absmax_u8(const uint8_t *frames, const int *tab, int B, int sh, int sw, int H, int W, const NormU8 &nm,
                           unsigned int *out_bits, hipStream_t s) {
    hipLaunchKernelGGL(absmax_u8_kernel, blocks_for((size_t)B * H * W, 4096), dim3(256), 0, s, frames, tab, B, sh, sw, H, W, nm, out_bits);
}
