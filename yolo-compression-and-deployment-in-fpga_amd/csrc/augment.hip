// yolo355_augment -- the pixel half of the reference's SSDAugmentation (utils/augmentations.py:413-431) on the GPU (gfx950): a
// list of uint8 HWC BGR frames of mixed sizes -> a normalised fp32 [n][3][H][W] batch, one launch per chunk of frames; C ABI and
// the whole contract (virtual image, photometric order, OpenCV's float resize and its two special cases) in
// include/yolo355_augment.h, linked into libyolo355_augment.so on its own (nothing of libyolo355.so is used).
//
//   augment_kernel<VEC>   one thread per four consecutive x of one output row, the lanes of a wave on consecutive x groups of
//                         that row (when up-scaling, neighbouring lanes read the same source bytes: the cache serves them).
//                         Per output pixel the two axes' taps come from y355_aug_tap (augment_tables.h) INLINE: a launch that
//                         keeps no state has no table to write to, and an entry costs five double operations beside the
//                         sixteen photometric chains of the thread.  Each tap is mapped back through mirror and (oy, ox): the
//                         fill, or three source bytes (read byte by byte, no alignment assumed) through the photometric chain,
//                         recomputed per tap rather than stored at 12 bytes per virtual pixel.  Then horizontal blend, vertical
//                         blend, / 255, - mean, / std and three stores, one per channel plane: VEC (W a multiple of 4 and the
//                         destination 16-byte aligned) 16 bytes per lane, otherwise one float at a time.  No LDS.
// The frame descriptors travel as kernel arguments by value (AugChunk), so there is no host table, no upload and nothing to keep
// alive between calls.  Every fp32 operation is written as its round-to-nearest intrinsic: no fused multiply-add whatever the
// flags, correctly rounded division -- the bits are tests/augment_ref.py's.
//
// Host side: y355_host.h's pieces (error return, HIPCHK, DeviceGuard).  Everything but the entry points of the public header is
// hidden, so that this library's y355_fail and error text stay its own in a process that also holds the other three.
#include <math.h>

#include "../../include/yolo355_augment.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
#include "augment_tables.h"
static_assert(Y355_AUGMENT_OK == Y355_OK && Y355_AUGMENT_EINVAL == Y355_EINVAL && Y355_AUGMENT_EHIP == Y355_EHIP &&
                  Y355_AUGMENT_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");
static_assert(sizeof(y355_augment_frame) == sizeof(y355_frame) && offsetof(y355_augment_frame, data_dev) == offsetof(y355_frame, data_dev) &&
                  offsetof(y355_augment_frame, height) == offsetof(y355_frame, height) && offsetof(y355_augment_frame, width) == offsetof(y355_frame, width) &&
                  offsetof(y355_augment_frame, row_bytes) == offsetof(y355_frame, row_bytes),
              "a y355_frame array (framelist.py) is passed as it is");
static_assert(sizeof(y355_augment_params) == 48, "the binding's AugParamsC");

#define THREADS 256
#define MODE_LINEAR 0
#define MODE_COPY 1                // equal sizes: OpenCV copies
#define MODE_AREA2 2               // exact 2x decimation of both axes: OpenCV's INTER_AREA integer-scale path

static thread_local std::string g_err;                  // y355_augment_last_error's text
#ifndef Y355_HOSTCHECK                                   // (augment_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

struct AugFrame {
    const uint8_t *src;
    long long pitch;        // bytes of one source row
    int sh, sw;
    int vh, vw, oy, ox;
    int flags, mode;
    float bri, con, sat, hue;
    float fill[3];
    int pad_;
};
constexpr int kAugChunk = 32;                 // frames per launch: 32 x 80 bytes of kernel arguments
struct AugChunk {
    AugFrame f[kAugChunk];
};
struct AugNorm {
    float mean[3], sd[3];
};
static_assert(sizeof(AugFrame) == 80, "the chunk's size below");
static_assert(sizeof(AugChunk) + sizeof(AugNorm) + 64 <= 4096, "kernel arguments: 4 KB");

// ------------------------------------------------------------------------------------------------------ device helpers
// PhotometricDistort on one source pixel (b, g, r); cv2.cvtColor's float BGR2HSV / HSV2BGR as include/yolo355_augment.h states
__device__ __forceinline__ void photometric(float &b, float &g, float &r, int flags, float bri, float con, float sat, float hue) {
    if (flags & Y355_AUG_BRIGHTNESS) {
        b = __fadd_rn(b, bri);
        g = __fadd_rn(g, bri);
        r = __fadd_rn(r, bri);
    }
    if (!(flags & Y355_AUG_HSV)) return;
    const bool contrast = flags & Y355_AUG_CONTRAST, first = flags & Y355_AUG_CONTRAST_FIRST;
    if (contrast && first) {
        b = __fmul_rn(b, con);
        g = __fmul_rn(g, con);
        r = __fmul_rn(r, con);
    }
    // BGR -> HSV (hrange 360: the hue scale is exactly 1)
    float v = r, vmin = r;
    if (v < g) v = g;
    if (v < b) v = b;
    if (vmin > g) vmin = g;
    if (vmin > b) vmin = b;
    float diff = __fsub_rn(v, vmin);
    float s = __fdiv_rn(diff, __fadd_rn(fabsf(v), 1.1920928955078125e-7f));
    diff = __fdiv_rn(60.f, __fadd_rn(diff, 1.1920928955078125e-7f));
    float h;
    if (v == r) h = __fmul_rn(__fsub_rn(g, b), diff);
    else if (v == g) h = __fadd_rn(__fmul_rn(__fsub_rn(b, r), diff), 120.f);
    else h = __fadd_rn(__fmul_rn(__fsub_rn(r, g), diff), 240.f);
    if (h < 0.f) h = __fadd_rn(h, 360.f);
    if (flags & Y355_AUG_SATURATION) s = __fmul_rn(s, sat);
    if (flags & Y355_AUG_HUE) {
        h = __fadd_rn(h, hue);
        if (h > 360.f) h = __fsub_rn(h, 360.f);
        if (h < 0.f) h = __fadd_rn(h, 360.f);
    }
    // HSV -> BGR
    if (s == 0.f) {
        b = g = r = v;
    } else {
        h = __fmul_rn(h, __fdiv_rn(6.f, 360.f));
        h = fmodf(h, 6.f);
        int sector = (int)floorf(h);
        h = __fsub_rn(h, (float)sector);
        if ((unsigned)sector >= 6u) {
            sector = 0;
            h = 0.f;
        }
        const float t0 = v, t1 = __fmul_rn(v, __fsub_rn(1.f, s)), t2 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, h))),
                    t3 = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, h))));
        // sector_data: {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0} as (b, g, r)
        b = sector == 0 || sector == 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
        g = sector == 0 ? t3 : (sector == 1 || sector == 2 ? t0 : (sector == 3 ? t2 : t1));
        r = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
    }
    if (contrast && !first) {
        b = __fmul_rn(b, con);
        g = __fmul_rn(g, con);
        r = __fmul_rn(r, con);
    }
}

// virtual pixel (vy, vx), both inside the virtual image: the fill, or the distorted source pixel
__device__ __forceinline__ void virt_px(const AugFrame &f, int vy, int vx, float *p) {
    const int x = (f.flags & Y355_AUG_MIRROR) ? f.vw - 1 - vx : vx;
    const int sy = vy - f.oy, sx = x - f.ox;
    if ((unsigned)sy < (unsigned)f.sh && (unsigned)sx < (unsigned)f.sw) {
        const uint8_t *q = f.src + (long long)sy * f.pitch + 3ll * sx;
        float b = (float)q[0], g = (float)q[1], r = (float)q[2];
        photometric(b, g, r, f.flags, f.bri, f.con, f.sat, f.hue);
        p[0] = b;
        p[1] = g;
        p[2] = r;
    } else {
        p[0] = f.fill[0];
        p[1] = f.fill[1];
        p[2] = f.fill[2];
    }
}

// ------------------------------------------------------------------------------------------------------ the kernel
template <bool VEC>
__global__ __launch_bounds__(THREADS) void augment_kernel(AugChunk ch, AugNorm nm, float *__restrict__ dst, int H, int W, int to_rgb) {
    const int gw = (W + 3) >> 2;
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= H * gw) return;
    const int n = blockIdx.y, y = i / gw, x0 = (i - y * gw) * 4;
    const AugFrame &f = ch.f[n];
    float o[3][4];
    AugTap ty = y355_aug_tap(y, f.vh, H, true);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = x0 + p;
        float d[3] = {0.f, 0.f, 0.f};
        if (x < W) {
            if (f.mode == MODE_COPY) {
                virt_px(f, y, x, d);
            } else if (f.mode == MODE_AREA2) {
                float a[3], b[3], c[3], e[3];
                virt_px(f, 2 * y, 2 * x, a);
                virt_px(f, 2 * y, 2 * x + 1, b);
                virt_px(f, 2 * y + 1, 2 * x, c);
                virt_px(f, 2 * y + 1, 2 * x + 1, e);
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    d[k] = __fmul_rn(__fadd_rn(0.f, __fadd_rn(__fadd_rn(__fadd_rn(a[k], b[k]), c[k]), e[k])), 0.25f);
            } else {
                const AugTap tx = y355_aug_tap(x, f.vw, W, false);
                float h0[3], h1[3], q[3];
                virt_px(f, ty.i0, tx.i0, h0);
                virt_px(f, ty.i1, tx.i0, h1);
                if (!tx.single) {
                    virt_px(f, ty.i0, tx.i1, q);
#pragma unroll
                    for (int k = 0; k < 3; ++k) h0[k] = __fadd_rn(__fmul_rn(h0[k], tx.c0), __fmul_rn(q[k], tx.c1));
                    virt_px(f, ty.i1, tx.i1, q);
#pragma unroll
                    for (int k = 0; k < 3; ++k) h1[k] = __fadd_rn(__fmul_rn(h1[k], tx.c0), __fmul_rn(q[k], tx.c1));
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) d[k] = __fadd_rn(__fmul_rn(h0[k], ty.c0), __fmul_rn(h1[k], ty.c1));
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k][p] = __fdiv_rn(__fsub_rn(__fdiv_rn(d[k], 255.f), nm.mean[k]), nm.sd[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float *out = dst + (((size_t)n * 3 + (to_rgb ? 2 - k : k)) * H + y) * (size_t)W + x0;
        if (VEC) {
            *(float4 *)out = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (x0 + p < W) out[p] = o[k][p];
        }
    }
}

// ------------------------------------------------------------------------------------------------------ host
static int check_args(const y355_augment_frame *frames, const y355_augment_params *params, int32_t n, int32_t dst_h, int32_t dst_w, const float *mean,
                      const float *std) {
    const int M = Y355_AUGMENT_MAX_SIDE;
    if (!frames || !params || !mean || !std) return y355_fail(Y355_AUGMENT_EINVAL, "y355_augment: null argument");
    if (n < 1) return y355_fail(Y355_AUGMENT_EINVAL, "n must be >= 1");
    if (dst_h < 1 || dst_w < 1 || dst_h > M || dst_w > M) return y355_fail(Y355_AUGMENT_EINVAL, "dst_h and dst_w must be 1..16384");
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(mean[c])) return y355_fail(Y355_AUGMENT_EINVAL, "mean must be finite");
        if (!std::isfinite(std[c]) || std[c] == 0.f) return y355_fail(Y355_AUGMENT_EINVAL, "std must be finite and non-zero");
    }
    for (int i = 0; i < n; ++i) {
        const y355_augment_frame &f = frames[i];
        const y355_augment_params &p = params[i];
        const std::string who = "frame " + std::to_string(i) + ": ";
        if (!f.data_dev) return y355_fail(Y355_AUGMENT_EINVAL, who + "null frame pointer");
        if (f.height < 1 || f.width < 1 || f.height > M || f.width > M) return y355_fail(Y355_AUGMENT_EINVAL, who + "height and width must be 1..16384");
        if (f.row_bytes != 0 && f.row_bytes < 3 * (int64_t)f.width) return y355_fail(Y355_AUGMENT_EINVAL, who + "row_bytes below width * 3");
        if (p.vh < 1 || p.vw < 1 || p.vh > M || p.vw > M) return y355_fail(Y355_AUGMENT_EINVAL, who + "vh and vw must be 1..16384");
        if (p.oy < -(1 << 24) || p.oy > (1 << 24) || p.ox < -(1 << 24) || p.ox > (1 << 24)) return y355_fail(Y355_AUGMENT_EINVAL, who + "oy and ox must be within +-2^24");
        if (p.flags & ~Y355_AUG_ALL_FLAGS) return y355_fail(Y355_AUGMENT_EINVAL, who + "unknown flags");
        if (!std::isfinite(p.brightness) || !std::isfinite(p.contrast) || !std::isfinite(p.saturation) || !std::isfinite(p.hue))
            return y355_fail(Y355_AUGMENT_EINVAL, who + "brightness, contrast, saturation and hue must be finite");
        if (!std::isfinite(p.fill[0]) || !std::isfinite(p.fill[1]) || !std::isfinite(p.fill[2])) return y355_fail(Y355_AUGMENT_EINVAL, who + "fill must be finite");
    }
    return Y355_AUGMENT_OK;
}
#pragma GCC visibility pop

// ------------------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char *y355_augment_last_error(void) { return g_err.c_str(); }

int y355_augment_abi(int32_t *frame_bytes, int32_t *params_bytes) {
    if (frame_bytes) *frame_bytes = (int32_t)sizeof(y355_augment_frame);
    if (params_bytes) *params_bytes = (int32_t)sizeof(y355_augment_params);
    return kAugChunk;
}

int y355_augment_check(const y355_augment_frame *frames, const y355_augment_params *params, int32_t n, int32_t dst_h, int32_t dst_w,
                       const float *mean, const float *std) {
    return check_args(frames, params, n, dst_h, dst_w, mean, std);
}

int y355_augment_run(int32_t device_id, const y355_augment_frame *frames, const y355_augment_params *params, int32_t n, int32_t dst_h,
                     int32_t dst_w, const float *mean, const float *std, int32_t to_rgb, void *dst_dev, void *stream) {
    if (int rc = check_args(frames, params, n, dst_h, dst_w, mean, std)) return rc;
    if (device_id < 0) return y355_fail(Y355_AUGMENT_EINVAL, "device_id < 0");
    if (!dst_dev) return y355_fail(Y355_AUGMENT_EINVAL, "y355_augment_run: null destination");
    hipStream_t s = (hipStream_t)stream;
    const int H = dst_h, W = dst_w;
    const bool vec = (W & 3) == 0 && ((uintptr_t)dst_dev & 15) == 0;
    AugNorm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean[c];
        nm.sd[c] = std[c];
    }
    DeviceGuard g;
    HIPCHK(g.set(device_id));
    for (int i0 = 0; i0 < n; i0 += kAugChunk) {
        const int m = std::min(kAugChunk, n - i0);
        AugChunk ch{};
        for (int k = 0; k < m; ++k) {
            const y355_augment_frame &f = frames[i0 + k];
            const y355_augment_params &p = params[i0 + k];
            AugFrame &a = ch.f[k];
            a.src = (const uint8_t *)f.data_dev;
            a.pitch = f.row_bytes ? (long long)f.row_bytes : 3ll * f.width;
            a.sh = f.height;
            a.sw = f.width;
            a.vh = p.vh;
            a.vw = p.vw;
            a.oy = p.oy;
            a.ox = p.ox;
            a.flags = p.flags;
            a.mode = p.vh == H && p.vw == W ? MODE_COPY : (p.vh == 2 * H && p.vw == 2 * W ? MODE_AREA2 : MODE_LINEAR);
            a.bri = p.brightness;
            a.con = p.contrast;
            a.sat = p.saturation;
            a.hue = p.hue;
            for (int c = 0; c < 3; ++c) a.fill[c] = p.fill[c];
        }
        float *out = (float *)dst_dev + (size_t)i0 * 3 * H * W;
        const dim3 grid((unsigned)((H * ((W + 3) >> 2) + THREADS - 1) / THREADS), (unsigned)m);
        if (vec) hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(THREADS), 0, s, ch, nm, out, H, W, to_rgb ? 1 : 0);
        else hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(THREADS), 0, s, ch, nm, out, H, W, to_rgb ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return Y355_AUGMENT_OK;
}

}  // extern "C"
