// yolo355 -- the operator layer: the stand-alone y355_* entry points that the drop-in modules (utils.modules), the composed
// YOLOv2 / v3 models and the operator tests go through.  Tensors are NCHW like the reference's.  Every operator has ONE
// implementation:
//   element-wise (reorg, SPP, 2x2 max-pool, bilinear 2x upsampling, on fp32)
//       the *_dev form checks the shape and launches on the caller's stream; the host-pointer form checks the pointers,
//       uploads, calls the *_dev form on the null stream, synchronises and downloads (host_form).  The two int8 helpers of
//       the slim path (input fake-quant, int8 max-pool) have a host-pointer form only.
//   convolution: y355_conv_op, an operator whose weights live packed on the device
//       bf16  conv_forward_bf16: conv + bias + LeakyReLU(slope) [+ residual], operands and result rounded to bf16, fp32
//             accumulation.  The 3x3 / 1x1 kernels of convg.hip and the general geometry of convgeom.hip differ in conv_plan
//             (kernel id, output size), in op_weights' packer and at the launch; the weight cache, the workspaces, the
//             re-zeroing for a new geometry, staging and unstaging are written once.
//       int8  y355_conv_op_forward_i8: Conv2d_fuse on a dyadic tensor, exact.  Exponent detection, then i8_prepare (weights,
//             the requantisation constants cached per exponent, workspaces), staging with the dyadic verdict, i8_launch (the
//             Y355_K_GEN16.. kernels of conv3x3.hip, or convgeom.hip) and unstaging.
//       The host-pointer forms run on a temporary operator made by the same create functions: y355_conv2d_bf16 and
//       y355_conv2d_geom_bf16 through conv_forward_bf16; y355_conv3x3_i8_raw and y355_conv_geom_i8_raw, whose input is int8
//       at a GIVEN exponent, enter below the exponent detection, at i8_prepare / i8_launch.  y355_conv3x3_i8_fused (the
//       requantising layer with its statistics pass) shares the kernel ladder, the parameter fill and the host layout helpers.
// Errors: HIPCHK returns Y355_EHIP with the failing call.  Device memory has one mechanism, the library's (y355_host.h): an
// operator's belongs to its ConvOpMem (conv_op_state.h, run on the CPU by `make hostcheck`), a call's to a DevScope and a
// temporary operator to an OpOwner, so no return path frees by hand.  Argument checks come before the first HIP call.
#include "../../include/yolo355.h"
#include "conv_op_state.h"
#include "y355_common.h"
#include "y355_requant.h"       // y355_rq_layer: the integer epilogue of a stand-alone layer

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {
inline int grid_for(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 16384); }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- kernels: element-wise ------------------------------------------------------------------------------------------------
// AveragedRangeTracker.quantize_activation on the network input (models/slim_yolo_v2.py:33-38): q = clamp(RNE(x * 2^sa), +-127)
__global__ void quantize_f32_i8_kernel(const float *x, int8_t *q, size_t n, float scale, unsigned long long *nclamped) {
    unsigned int c = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float r = rintf(x[i] * scale);
        const float rc = fminf(fmaxf(r, -127.f), 127.f);
        c += rc != r ? 1u : 0u;
        q[i] = (int8_t)(int)rc;
    }
    if (c) atomicAdd(nclamped, (unsigned long long)c);
}

// nn.MaxPool2d(2, 2) (models/slim_yolo_v2.py:61,65,71,77) on int8
__global__ void maxpool2x2_i8_kernel(const int8_t *in, int8_t *out, size_t planes, int H, int W) {
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t n = planes * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
        const size_t pl = i / ((size_t)Ho * Wo);
        const int8_t *s = in + (pl * H + 2 * y) * W + 2 * x;
        out[i] = (int8_t)max(max((int)s[0], (int)s[1]), max((int)s[W], (int)s[W + 1]));
    }
}

// utils.modules.reorg_layer (utils/modules.py:43-57): out[b][(sy*s+sx)*C + c][y][x] = in[b][c][s*y+sy][s*x+sx]  (bit-exact)
__global__ void reorg_f32_kernel(const float *in, float *out, int B, int C, int H, int W, int s) {
    const int Ho = H / s, Wo = W / s;
    const size_t n = (size_t)B * C * s * s * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
        const int oc = (int)((i / ((size_t)Wo * Ho)) % ((size_t)C * s * s));
        const int b = (int)(i / ((size_t)Wo * Ho * C * s * s));
        const int k = oc / C, c = oc % C, sy = k / s, sx = k % s;
        out[i] = in[(((size_t)b * C + c) * H + (size_t)s * y + sy) * W + (size_t)s * x + sx];
    }
}

// utils.modules.SPP (:59-72): cat[x, maxpool5(x), maxpool9(x), maxpool13(x)], stride 1, padding k/2 with -inf  (bit-exact)
__global__ void spp_f32_kernel(const float *in, float *out, size_t planes_b, int C, int H, int W) {
    // one thread per input element: writes x and the three window maxima (windows clipped to the map:
    // the -inf padding of max_pool2d never wins)
    const size_t n = planes_b * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        const float *pl = in + (b * C + c) * (size_t)H * W;
        float m5 = -INFINITY, m9 = -INFINITY, m13 = -INFINITY;
        for (int dy = -6; dy <= 6; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -6; dx <= 6; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                const float v = pl[(size_t)yy * W + xx];
                const int r = max(abs(dy), abs(dx));
                m13 = fmaxf(m13, v);
                if (r <= 4) m9 = fmaxf(m9, v);
                if (r <= 2) m5 = fmaxf(m5, v);
            }
        }
        float *ob = out + b * 4 * C * (size_t)H * W + (size_t)y * W + x;
        const size_t cs = (size_t)H * W;
        ob[(size_t)c * cs] = pl[(size_t)y * W + x];
        ob[((size_t)C + c) * cs] = m5;
        ob[((size_t)2 * C + c) * cs] = m9;
        ob[((size_t)3 * C + c) * cs] = m13;
    }
}

__global__ void maxpool2x2_f32_kernel(const float *in, float *out, size_t planes, int H, int W) {
    const int Ho = H >> 1, Wo = W >> 1;
    const size_t n = planes * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
        const size_t pl = i / ((size_t)Ho * Wo);
        const float *s = in + (pl * H + 2 * y) * W + 2 * x;
        out[i] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
    }
}
// F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) (models/yolo_v3.py:211,215)
__global__ void upsample2x_f32_kernel(const float *in, float *out, size_t planes, int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W;
    const float ry = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f, rx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const size_t n = planes * Ho * Wo;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
        const size_t pl = i / ((size_t)Ho * Wo);
        const float sy = ry * (float)y, sx = rx * (float)x;
        const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const float *s = in + pl * (size_t)H * W;
        const float top = (1.f - lx) * s[(size_t)y0 * W + x0] + lx * s[(size_t)y0 * W + x1];
        const float bot = (1.f - lx) * s[(size_t)y1 * W + x0] + lx * s[(size_t)y1 * W + x1];
        out[i] = (1.f - ly) * top + ly * bot;
    }
}

// ---- kernels: layouts of the convolutions ---------------------------------------------------------------------------------
// fp32 NCHW -> bf16 NHWC with a one-pixel halo and cpad channels (buffer zeroed beforehand)
__global__ void nchw_to_nhwc_bf16_kernel(const float *in, unsigned short *out, int B, int C, int H, int W, int cpad) {
    const size_t n = (size_t)B * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        out[((b * (H + 2) + y + 1) * (size_t)(W + 2) + x + 1) * cpad + c] = __builtin_bit_cast(unsigned short, (__bf16)in[i]);
    }
}
__global__ void nhwc_bf16_to_nchw_kernel(const unsigned short *in, float *out, int B, int C, int H, int W, int cpad) {
    const size_t n = (size_t)B * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        out[i] = __uint_as_float((unsigned int)in[((b * (H + 2) + y + 1) * (size_t)(W + 2) + x + 1) * cpad + c] << 16);
    }
}
__global__ void nhwc_f32_to_nchw_kernel(const float *in, float *out, int B, int C, int H, int W, int cpad) {
    const size_t n = (size_t)B * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        out[i] = in[((b * (H + 2) + y + 1) * (size_t)(W + 2) + x + 1) * cpad + c];
    }
}
// fp32 NCHW dyadic tensor -> int8 NHWC with halo (cpad channels): q = x * 2^sa; *bad += values that are not integers in [-127, 127]
__global__ void dyadic_to_nhwc_i8_kernel(const float *in, int8_t *out, int B, int C, int H, int W, int cpad, float scale, unsigned int *bad) {
    const size_t n = (size_t)B * C * H * W;
    unsigned int nb = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        const float v = in[i] * scale, r = rintf(v);
        nb += (r != v || !(fabsf(r) <= 127.f)) ? 1u : 0u;
        out[((b * (H + 2) + y + 1) * (size_t)(W + 2) + x + 1) * cpad + c] = (int8_t)(int)fminf(fmaxf(r, -127.f), 127.f);
    }
    if (nb) atomicAdd(bad, nb);
}
// t' [B][H][W][cpad] int64 -> fp32 NCHW: t' * 2^-F' (exact wherever the reference's own fp32 result is)
__global__ void raw_to_nchw_f32_kernel(const long long *raw, float *out, int B, int C, int H, int W, int cpad, float inv) {
    const size_t n = (size_t)B * C * H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W), y = (int)((i / W) % H);
        const int c = (int)((i / ((size_t)W * H)) % C);
        const size_t b = i / ((size_t)W * H * C);
        out[i] = (float)raw[((b * H + y) * (size_t)W + x) * cpad + c] * inv;
    }
}

// ---- host-side layout helpers of the int8 host-pointer forms ---------------------------------------------------------------
// int8 NCHW -> NHWC with a one-pixel halo and cpad channels, zero elsewhere; `bytes` = the device buffer's size
std::vector<int8_t> nhwc_halo_i8(const int8_t *q, int batch, int cin, int H, int W, int cpad, size_t bytes) {
    std::vector<int8_t> xin(bytes, 0);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < cin; ++c)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    xin[(((size_t)b * (H + 2) + y + 1) * (W + 2) + x + 1) * cpad + c] = q[(((size_t)b * cin + c) * H + y) * W + x];
    return xin;
}
// [B][Ho][Wo][cout_pad] -> NCHW, the cout real channels
template <class S, class D> void nhwc_to_nchw(const S *o, D *out, int batch, int cout, int Ho, int Wo, int cout_pad) {
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < cout; ++c)
            for (int y = 0; y < Ho; ++y)
                for (int x = 0; x < Wo; ++x)
                    out[(((size_t)b * cout + c) * Ho + y) * Wo + x] = (D)o[(((size_t)b * Ho + y) * Wo + x) * cout_pad + c];
}

// host-pointer form of an element-wise fp32 operator: upload, the *_dev form on the null stream, synchronise, download
template <class F> int host_form(int device_id, const float *x, size_t n_in, float *out, size_t n_out, F dev_form) {
    DevScope tmp;
    float *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipSetDevice(device_id));
    if (int rc = y355_dev_get(tmp, &d_in, n_in)) return rc;
    if (int rc = y355_dev_get(tmp, &d_out, n_out)) return rc;
    HIPCHK(hipMemcpy(d_in, x, n_in * 4, hipMemcpyHostToDevice));
    if (int rc = dev_form(d_in, d_out)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, n_out * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the shape checks of the element-wise operators; *n = elements of the input
int map_shape(int batch, int channels, int height, int width, int min_hw, size_t *n) {
    if (batch < 1 || channels < 1 || height < min_hw || width < min_hw) return y355_fail(Y355_EINVAL, "bad shape");
    *n = (size_t)batch * channels * height * width;
    return 0;
}
int reorg_shape(int batch, int channels, int height, int width, int stride, size_t *n) {
    if (stride < 1) return y355_fail(Y355_EINVAL, "bad shape");
    if (int rc = map_shape(batch, channels, height, width, stride, n)) return rc;
    if (height % stride || width % stride) return y355_fail(Y355_EINVAL, "reorg needs H, W divisible by the stride");
    return 0;
}
int pool_shape(int batch, int channels, int height, int width, size_t *n) {
    if (int rc = map_shape(batch, channels, height, width, 2, n)) return rc;
    if ((height | width) & 1) return y355_fail(Y355_EINVAL, "pooling needs even H, W");
    return 0;
}
}  // namespace

// ==========================================================================================================================
// Element-wise operators
extern "C" int y355_quantize_input_f32_i8(int device_id, const float *x, size_t n, int sa, int8_t *q, int64_t *clamped) {
    if (!x || !q) return y355_fail(Y355_EINVAL, "null argument");
    if (n == 0) return y355_fail(Y355_EINVAL, "empty tensor");
    if (sa < -64 || sa > 64) return y355_fail(Y355_EINVAL, "activation exponent out of range");
    DevScope tmp;
    float *d_in = nullptr;
    int8_t *d_out = nullptr;
    unsigned long long *d_cnt = nullptr;
    HIPCHK(hipSetDevice(device_id));
    if (int rc = y355_dev_get(tmp, &d_in, n)) return rc;
    if (int rc = y355_dev_get(tmp, &d_out, n)) return rc;
    if (int rc = y355_dev_get(tmp, &d_cnt, 1)) return rc;
    HIPCHK(hipMemcpy(d_in, x, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_cnt, 0, 8));
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(quantize_f32_i8_kernel, dim3(blocks), dim3(256), 0, 0, d_in, d_out, n, std::ldexp(1.0f, sa), d_cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(q, d_out, n, hipMemcpyDeviceToHost));
    unsigned long long c = 0;
    HIPCHK(hipMemcpy(&c, d_cnt, 8, hipMemcpyDeviceToHost));
    if (clamped) *clamped = (int64_t)c;
    return 0;
}

extern "C" int y355_maxpool2x2_i8(int device_id, const int8_t *in, int batch, int channels, int height, int width, int8_t *out) {
    if (!in || !out) return y355_fail(Y355_EINVAL, "null argument");
    size_t nin = 0;
    if (int rc = pool_shape(batch, channels, height, width, &nin)) return rc;
    const size_t nout = nin / 4;
    DevScope tmp;
    int8_t *d_in = nullptr, *d_out = nullptr;
    HIPCHK(hipSetDevice(device_id));
    if (int rc = y355_dev_get(tmp, &d_in, nin)) return rc;
    if (int rc = y355_dev_get(tmp, &d_out, nout)) return rc;
    HIPCHK(hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice));
    const int blocks = (int)std::min<size_t>((nout + 255) / 256, 8192);
    hipLaunchKernelGGL(maxpool2x2_i8_kernel, dim3(blocks), dim3(256), 0, 0, d_in, d_out, (size_t)batch * channels, height, width);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int y355_reorg_f32_dev(const float *x_dev, int batch, int channels, int height, int width, int stride, float *out_dev, void *stream) {
    if (!x_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = reorg_shape(batch, channels, height, width, stride, &n)) return rc;
    hipLaunchKernelGGL(reorg_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x_dev, out_dev, batch, channels, height, width, stride);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int y355_spp_f32_dev(const float *x_dev, int batch, int channels, int height, int width, float *out_dev, void *stream) {
    if (!x_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = map_shape(batch, channels, height, width, 1, &n)) return rc;
    hipLaunchKernelGGL(spp_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x_dev, out_dev, (size_t)batch, channels, height, width);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int y355_maxpool2x2_f32_dev(const float *in_dev, int batch, int channels, int height, int width, float *out_dev, void *stream) {
    if (!in_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = pool_shape(batch, channels, height, width, &n)) return rc;
    hipLaunchKernelGGL(maxpool2x2_f32_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, in_dev, out_dev, (size_t)batch * channels,
                       height, width);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int y355_upsample2x_f32_dev(const float *in_dev, int batch, int channels, int height, int width, float *out_dev, void *stream) {
    if (!in_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = map_shape(batch, channels, height, width, 1, &n)) return rc;
    hipLaunchKernelGGL(upsample2x_f32_kernel, dim3(grid_for(n * 4)), dim3(256), 0, (hipStream_t)stream, in_dev, out_dev, (size_t)batch * channels,
                       height, width);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int y355_reorg_f32(int device_id, const float *x, int batch, int channels, int height, int width, int stride, float *out) {
    if (!x || !out) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = reorg_shape(batch, channels, height, width, stride, &n)) return rc;
    return host_form(device_id, x, n, out, n,
                     [&](const float *dx, float *dy) { return y355_reorg_f32_dev(dx, batch, channels, height, width, stride, dy, nullptr); });
}
extern "C" int y355_spp_f32(int device_id, const float *x, int batch, int channels, int height, int width, float *out) {
    if (!x || !out) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = map_shape(batch, channels, height, width, 1, &n)) return rc;
    return host_form(device_id, x, n, out, n * 4,
                     [&](const float *dx, float *dy) { return y355_spp_f32_dev(dx, batch, channels, height, width, dy, nullptr); });
}
extern "C" int y355_maxpool2x2_f32(int device_id, const float *in, int batch, int channels, int height, int width, float *out) {
    if (!in || !out) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = pool_shape(batch, channels, height, width, &n)) return rc;
    return host_form(device_id, in, n, out, n / 4,
                     [&](const float *dx, float *dy) { return y355_maxpool2x2_f32_dev(dx, batch, channels, height, width, dy, nullptr); });
}
extern "C" int y355_upsample2x_f32(int device_id, const float *in, int batch, int channels, int height, int width, float *out) {
    if (!in || !out) return y355_fail(Y355_EINVAL, "null argument");
    size_t n = 0;
    if (int rc = map_shape(batch, channels, height, width, 1, &n)) return rc;
    return host_form(device_id, in, n, out, n * 4,
                     [&](const float *dx, float *dy) { return y355_upsample2x_f32_dev(dx, batch, channels, height, width, dy, nullptr); });
}

// ==========================================================================================================================
// y355_conv_op: a convolution whose weights are packed onto the device by the operator and whose workspaces grow on demand;
// single-threaded like an engine handle.  The forwards take DEVICE pointers (fp32 NCHW) and a stream, launch behind whatever
// that stream holds and return without waiting.  The int8 form needs two things on the HOST -- the input's exponent and the
// verdict "is x a dyadic int8 tensor" select the route and the requantisation constants: two 4-byte read-backs per call.
// General geometry (include/yolo355.h y355_conv_geom): any kernel size, stride, dilation and four zero pads on the
// implicit-GEMM kernel of convgeom.hip, in the same layouts -- input NHWC with a one-pixel halo, bf16 output NHWC with a halo,
// int8 t' [pixel][cout_pad] -- and with y355_rq_layer's integer epilogue (y355_requant.h) at the layer's tap count.
struct y355_conv_op {
    int device = 0, kind = 0;          // kind 0 bf16, 1 int8
    int cin = 0, cout = 0, ksize = 3, stride = 1;
    int geom = 0;                      // 1: general geometry g on convgeom.hip; 0: ksize / stride on convg.hip (bf16), 3x3 on conv3x3.hip (int8)
    y355_conv_geom g{};
    int cpad = 0;                      // channels of a staged input pixel (bf16 or int8 elements)
    // the device memory: the packed weights for the kernel id and padded width the last shapes selected (op_weights), the
    // int8 operator's create-time buffers, the workspaces
    ConvOpMem m;
    // bf16
    float slope = 1.f;
    std::vector<float> w_host, b_host;
    // int8
    std::vector<int8_t> qw;
    std::vector<int32_t> qb;
    int e_w = 0, e_b = 0, act = 0;
    int sa_cached = NO_SA;             // the input exponent rq / frac_bits / the device biases were made for
    Requant rq{};
    int frac_bits = 0;
    static constexpr int NO_SA = 1 << 30;
};

namespace {
struct OpOwner {                       // the temporary operator of a host-pointer form
    y355_conv_op *op = nullptr;
    ~OpOwner() { y355_conv_op_destroy(op); }
};

constexpr long long GEOM_I8_MAX_K = 133144;      // 127 * 127 * cin * kh * kw <= INT32_MAX

int geom_limits(const y355_conv_geom *g) {
    if (!g) return y355_fail(Y355_EINVAL, "null geometry");
    if (g->kh < 1 || g->kh > 32 || g->kw < 1 || g->kw > 32) return y355_fail(Y355_EINVAL, "kernel size 1..32");
    if (g->stride_h < 1 || g->stride_h > 16 || g->stride_w < 1 || g->stride_w > 16) return y355_fail(Y355_EINVAL, "stride 1..16");
    if (g->dil_h < 1 || g->dil_h > 32 || g->dil_w < 1 || g->dil_w > 32) return y355_fail(Y355_EINVAL, "dilation 1..32");
    for (int v : {g->pad_top, g->pad_bottom, g->pad_left, g->pad_right})
        if (v < 0 || v > 64) return y355_fail(Y355_EINVAL, "padding 0..64 on each side");
    return 0;
}

int geom_out(const y355_conv_geom *g, int batch, int height, int width, int *ho, int *wo) {
    if (int rc = geom_limits(g)) return rc;
    if (batch < 1 || height < 1 || width < 1) return y355_fail(Y355_EINVAL, "bad shape");
    const int hn = height + g->pad_top + g->pad_bottom - g->dil_h * (g->kh - 1) - 1;
    const int wn = width + g->pad_left + g->pad_right - g->dil_w * (g->kw - 1) - 1;
    if (hn < 0 || wn < 0) return y355_fail(Y355_EINVAL, "the dilated kernel is larger than the padded input (Ho or Wo < 1)");
    *ho = hn / g->stride_h + 1;
    *wo = wn / g->stride_w + 1;
    if ((long long)batch * *ho * *wo > 0x7fffffffll || (long long)batch * (height + 2) * (width + 2) > 0x7fffffffll)
        return y355_fail(Y355_EINVAL, "too many pixels");
    return 0;
}

int geom_i8_k(int cin, const y355_conv_geom *g) {
    if ((long long)cin * g->kh * g->kw > GEOM_I8_MAX_K)
        return y355_fail(Y355_ERANGE, "127 * 127 * cin * kh * kw does not fit the int32 accumulator (cin * kh * kw > 133144)");
    return 0;
}

ConvGeomParams geom_params(const y355_conv_geom &g, int batch, int height, int width, int ho, int wo, int in_pb, int cout_pad, int bn) {
    ConvGeomParams p{};
    p.B = batch; p.H = height; p.W = width; p.Ho = ho; p.Wo = wo; p.M = batch * ho * wo;
    p.in_pb = in_pb; p.nchunk = in_pb / 64;
    p.kh = g.kh; p.kw = g.kw; p.sh = g.stride_h; p.sw = g.stride_w; p.dh = g.dil_h; p.dw = g.dil_w; p.pt = g.pad_top; p.pl = g.pad_left;
    p.nblk = cout_pad / bn; p.cout_pad = cout_pad;
    return p;
}

int geom_act(int flags) { return (flags & Y355_OP_LEAKY) ? 1 : ((flags & Y355_OP_RELU) ? 2 : 0); }
int act_flags(int flags) {
    if ((flags & Y355_OP_LEAKY) && (flags & Y355_OP_RELU)) return y355_fail(Y355_EINVAL, "LeakyReLU and ReLU are exclusive");
    return 0;
}
int geom_flags(int flags) {
    if (int rc = act_flags(flags)) return rc;
    if (flags & Y355_OP_POOL) return y355_fail(Y355_EINVAL, "no fused max-pool on the general geometry");
    return 0;
}

// the generic 3x3 int8 kernel of conv3x3.hip for cin input channels (pool: the one with the fused max-pool): its id, and the
// channels its input pixels are padded to
int gen16_kernel(int cin, int pool, int *cpad) {
    *cpad = cin <= 16 ? 16 : cin <= 32 ? 32 : cin <= 64 ? 64 : cin <= 128 ? 128 : 256;
    const int sel = *cpad == 16 ? 0 : *cpad == 32 ? 1 : *cpad == 64 ? 2 : *cpad == 128 ? 3 : 4;
    return (pool ? Y355_K_GEN16P : Y355_K_GEN16) + sel;
}
int gen16_shape(int batch, int cin, int cout, int H, int W, int flags) {
    if (batch < 1 || cin < 1 || cin > 256 || cout < 1 || H < 1 || W < 1) return y355_fail(Y355_EINVAL, "bad shape (cin <= 256)");
    return act_flags(flags);
}
// the launch parameters of such a kernel, but for where the result goes (out / raw) and the pass (mode, guard)
ConvParams gen16_params(const ConvKernelInfo &ki, const int8_t *in, const int8_t *w, const int *bias_t, const long long *bias_w, Counters *ctr,
                        int batch, int H, int W, int cout_pad, const Requant &rq) {
    ConvParams p{};
    p.in = in; p.w = w; p.bias_t = bias_t; p.bias_w = bias_w; p.ctr = ctr;
    p.B = batch; p.H = H; p.W = W; p.cstride = cout_pad; p.out_halo = 0;
    p.tiles_x = (W + ki.tw - 1) / ki.tw; p.tiles_y = (H + ki.th - 1) / ki.th; p.nblk = cout_pad / ki.bn;
    p.rq = rq;
    return p;
}

// (batch, H, W, output type) as one word, never 0: what a workspace's halo and padding channels were last zeroed for
size_t geo_word(int batch, int height, int width, int out_fp32) {
    return ((size_t)batch << 40) ^ ((size_t)height << 20) ^ (size_t)width ^ ((size_t)out_fp32 << 62) ^ ((size_t)1 << 61);
}
// The workspaces of a forward at that geometry, grown and zeroed on s where they were last zeroed for another one; a failure
// leaves the recorded geometries alone, so the next forward zeroes again.  res_bytes 0: no residual.
int op_workspaces(y355_conv_op *op, size_t geo, size_t in_bytes, size_t out_bytes, bool out_halo, size_t res_bytes, hipStream_t s) {
    ConvOpZero z;
    if (int rc = y355_convop_workspaces(op->m, geo, in_bytes, out_bytes, out_halo, res_bytes, &z)) return rc;
    if (z.in) HIPCHK(hipMemsetAsync(op->m.in_dev, 0, in_bytes, s));
    if (z.out) HIPCHK(hipMemsetAsync(op->m.out_dev, 0, out_bytes, s));
    if (z.res) HIPCHK(hipMemsetAsync(op->m.res_dev, 0, res_bytes, s));
    y355_convop_zeroed(op->m, geo, z);
    return 0;
}

// what one forward at batch x height x width runs: the kernel, the output map, the padded output channels
struct ConvPlan {
    int kid = 0, Ho = 0, Wo = 0, cout_pad = 0;
    const ConvGInfo *kg = nullptr;     // bf16 3x3 / 1x1
};
// the output size only: the argument checks that come before any HIP call
int conv_out_size(const y355_conv_op *op, int batch, int height, int width, ConvPlan *pl) {
    if (op->geom) return geom_out(&op->g, batch, height, width, &pl->Ho, &pl->Wo);
    if (batch < 1 || height < 1 || width < 1) return y355_fail(Y355_EINVAL, "bad shape");
    pl->Ho = op->stride == 2 ? (height + 1) / 2 : height;
    pl->Wo = op->stride == 2 ? (width + 1) / 2 : width;
    return 0;
}
// the kernel for that size (the device is set: the general geometry sizes its tiles by the compute units)
int conv_plan(const y355_conv_op *op, int batch, int height, int width, ConvPlan *pl) {
    int bn = 0;
    if (op->geom) {
        pl->kid = y355_convgeom_select(batch * pl->Ho * pl->Wo, op->cout, y355_cu_count());
        bn = y355_convgeom_info(pl->kid)->bn;
    } else if (op->kind == 0) {
        pl->kid = y355_convg_select(op->cpad * 2, op->cout, 0, height, width, op->stride);
        pl->kg = y355_convg_kernel(1, pl->kid);
        if (!pl->kg) return y355_fail(Y355_EINVAL, "no kernel for this shape");
        bn = pl->kg->bn;
    } else {
        int cpad = 0;
        pl->kid = gen16_kernel(op->cin, 0, &cpad);
        bn = y355_conv_kernel(pl->kid)->bn;
    }
    pl->cout_pad = round_up(op->cout, bn);
    return 0;
}

// The packed weights for kernel pl.kid at pl.cout_pad output channels, with the bias vector that is padded alike: packed from
// the host copy on first use, and again when a map size selects another tile shape.
int op_weights(y355_conv_op *op, const ConvPlan &pl, hipStream_t s) {
    if (op->m.w_kid == pl.kid && op->m.w_cout_pad == pl.cout_pad) return 0;
    const int taps = op->geom ? op->g.kh * op->g.kw : op->ksize * op->ksize, in_pb = op->kind ? op->cpad : op->cpad * 2;
    const float *wf = op->kind ? nullptr : op->w_host.data();
    const int8_t *wq = op->kind ? op->qw.data() : nullptr;
    std::vector<char> wpk;
    if (op->geom) {
        wpk.resize(y355_convgeom_packed_bytes(pl.kid, in_pb, taps, pl.cout_pad));
        y355_convgeom_pack(pl.kid, op->kind ? 0 : 1, wf, wq, op->cout, op->cin, taps, in_pb, pl.cout_pad, wpk.data());
    } else if (op->kind == 0) {
        wpk.resize(y355_convg_packed_bytes(*pl.kg, in_pb, taps, pl.cout_pad));
        y355_convg_pack(*pl.kg, wf, nullptr, op->cout, op->cin, op->ksize, in_pb, pl.cout_pad, wpk.data());
    } else {
        const ConvKernelInfo &ki = *y355_conv_kernel(pl.kid);
        wpk.resize(y355_packed_bytes(ki, pl.cout_pad));
        y355_pack_weights(ki, wq, op->cout, op->cin, pl.cout_pad, (int8_t *)wpk.data());
    }
    std::vector<float> bpad;
    if (op->kind == 0) {
        bpad.assign(pl.cout_pad, 0.f);
        std::copy(op->b_host.begin(), op->b_host.end(), bpad.begin());
    }
    HIPCHK(hipStreamSynchronize(s));                               // a previous forward may still read the old fragments
    if (int rc = y355_convop_swap_weights(op->m, pl.kid, pl.cout_pad, wpk, op->kind ? nullptr : bpad.data(), s)) return rc;
    op->sa_cached = y355_conv_op::NO_SA;                           // the int8 biases are padded to the new width by i8_prepare
    return 0;
}

int attr_fail(int e) { return y355_fail(Y355_EHIP, std::string("kernel attributes: ") + hipGetErrorString((hipError_t)e)); }

y355_conv_op *op_new(int device_id, int kind, int cin, int cout, const y355_conv_geom *g) {
    y355_conv_op *op = new y355_conv_op();
    op->device = device_id; op->kind = kind; op->cin = cin; op->cout = cout;
    op->m.own.mem = y355_hip_mem();
    if (g) {
        op->geom = 1;
        op->g = *g;
    }
    return op;
}
}  // namespace

extern "C" void y355_conv_op_destroy(y355_conv_op *op) {
    if (!op) return;
    (void)hipSetDevice(op->device);
    (void)hipDeviceSynchronize();
    y355_convop_close(op->m);
    delete op;
}

extern "C" int y355_conv_geom_out_size(const y355_conv_geom *g, int height, int width, int *ho, int *wo) {
    if (!ho || !wo) return y355_fail(Y355_EINVAL, "null argument");
    return geom_out(g, 1, height, width, ho, wo);
}

// ---- create ----------------------------------------------------------------------------------------------------------------
static int create_bf16(int device_id, const float *w, const float *bias, int cin, int cout, int ksize, int stride, const y355_conv_geom *g,
                       float neg_slope, y355_conv_op **out) {
    HIPCHK(hipSetDevice(device_id));
    if (int e = g ? y355_prepare_convgeom() : y355_prepare_convg()) return attr_fail(e);
    y355_conv_op *op = op_new(device_id, 0, cin, cout, g);
    op->ksize = ksize; op->stride = stride; op->slope = neg_slope;
    const bool thin = !g && cin <= 16 && ksize == 3 && stride == 1;
    op->cpad = thin ? 16 : round_up(cin, 32);
    op->w_host.assign(w, w + (size_t)cout * cin * (g ? g->kh * g->kw : ksize * ksize));
    op->b_host.assign(cout, 0.f);
    if (bias) std::copy(bias, bias + cout, op->b_host.begin());
    *out = op;
    return 0;
}

extern "C" int y355_conv_op_create_bf16(int device_id, const float *w, const float *bias, int cin, int cout, int ksize, int stride,
                                        float neg_slope, y355_conv_op **out) {
    if (!w || !out) return y355_fail(Y355_EINVAL, "null argument");
    if (cin < 1 || cout < 1) return y355_fail(Y355_EINVAL, "bad shape");
    if (ksize != 1 && ksize != 3) return y355_fail(Y355_EINVAL, "kernel size 1 or 3 (padding k/2)");
    if (stride != 1 && !(stride == 2 && ksize == 3)) return y355_fail(Y355_EINVAL, "stride 1, or 2 with a 3x3 kernel");
    return create_bf16(device_id, w, bias, cin, cout, ksize, stride, nullptr, neg_slope, out);
}

extern "C" int y355_conv_op_create_bf16_geom(int device_id, const float *w, const float *bias, int cin, int cout, const y355_conv_geom *g,
                                             float neg_slope, y355_conv_op **out) {
    if (!w || !out || !g) return y355_fail(Y355_EINVAL, "null argument");
    if (cin < 1 || cout < 1) return y355_fail(Y355_EINVAL, "bad shape");
    if (int rc = geom_limits(g)) return rc;
    return create_bf16(device_id, w, bias, cin, cout, 3, 1, g, neg_slope, out);
}

// 3x3: the kernel depends on cin alone, so the weights are packed here and every forward finds them
static int create_i8(int device_id, const int8_t *q_w, const int32_t *q_b, int cin, int cout, const y355_conv_geom *g, int e_w, int e_b, int flags,
                     y355_conv_op **out) {
    HIPCHK(hipSetDevice(device_id));
    if (g) {
        if (int e = y355_prepare_convgeom()) return attr_fail(e);
    } else if (int e = y355_prepare_kernels()) {
        return e;
    }
    OpOwner own{op_new(device_id, 1, cin, cout, g)};
    y355_conv_op *op = own.op;
    op->e_w = e_w; op->e_b = e_b;
    op->act = geom_act(flags);
    op->qw.assign(q_w, q_w + (size_t)cout * cin * (g ? g->kh * g->kw : 9));
    op->qb.assign(q_b, q_b + cout);
    if (g) {
        op->cpad = round_up(cin, 64);
        if (int rc = y355_convop_create_i8(op->m, 0)) return rc;
    } else {
        ConvPlan pl;
        (void)gen16_kernel(cin, 0, &op->cpad);
        if (int rc = conv_plan(op, 1, 1, 1, &pl)) return rc;
        if (int rc = y355_convop_create_i8(op->m, pl.cout_pad)) return rc;
        if (int rc = op_weights(op, pl, nullptr)) return rc;
    }
    *out = op;
    own.op = nullptr;
    return 0;
}

extern "C" int y355_conv_op_create_i8(int device_id, const int8_t *q_w, const int32_t *q_b, int cin, int cout, int e_w, int e_b, int flags,
                                      y355_conv_op **out) {
    if (!q_w || !q_b || !out) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = gen16_shape(1, cin, cout, 1, 1, flags)) return rc;
    return create_i8(device_id, q_w, q_b, cin, cout, nullptr, e_w, e_b, flags, out);
}

extern "C" int y355_conv_op_create_i8_geom(int device_id, const int8_t *q_w, const int32_t *q_b, int cin, int cout, const y355_conv_geom *g,
                                           int e_w, int e_b, int flags, y355_conv_op **out) {
    if (!q_w || !q_b || !out || !g) return y355_fail(Y355_EINVAL, "null argument");
    if (cin < 1 || cout < 1) return y355_fail(Y355_EINVAL, "bad shape");
    if (int rc = geom_limits(g)) return rc;
    if (int rc = geom_flags(flags)) return rc;
    if (int rc = geom_i8_k(cin, g)) return rc;
    return create_i8(device_id, q_w, q_b, cin, cout, g, e_w, e_b, flags, out);
}

// ---- bf16 forward ----------------------------------------------------------------------------------------------------------
static int conv_forward_bf16(y355_conv_op *op, const float *x_dev, const float *residual_dev, int batch, int height, int width, int out_fp32,
                             float *out_dev, hipStream_t s) {
    if (out_fp32 && residual_dev) return y355_fail(Y355_EINVAL, "fp32 output (prediction layers) takes no residual");
    ConvPlan pl;
    if (int rc = conv_out_size(op, batch, height, width, &pl)) return rc;
    HIPCHK(hipSetDevice(op->device));
    if (int rc = conv_plan(op, batch, height, width, &pl)) return rc;
    if (int rc = op_weights(op, pl, s)) return rc;
    const int Ho = pl.Ho, Wo = pl.Wo, cout_pad = pl.cout_pad, in_pb = op->cpad * 2;
    const size_t n_in = (size_t)batch * op->cin * height * width, n_out = (size_t)batch * op->cout * Ho * Wo;
    const size_t in_bytes = (size_t)batch * (height + 2) * (width + 2) * in_pb;
    const size_t out_pb = (size_t)cout_pad * (out_fp32 ? 4 : 2), out_bytes = (size_t)batch * (Ho + 2) * (Wo + 2) * out_pb;
    // the staging kernels only write the interior and the real channels, so the halo and the padding channels stay zero for
    // every later call of the same geometry; a new geometry re-zeroes (cheap next to a reallocation).  convgeom.hip writes
    // every channel of a pixel it owns, so its output is not kept zero
    if (int rc = op_workspaces(op, geo_word(batch, height, width, out_fp32), in_bytes, out_bytes, !op->geom, residual_dev ? out_bytes : 0, s))
        return rc;
    if (residual_dev) {
        hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel, dim3(grid_for(n_out)), dim3(256), 0, s, residual_dev, (unsigned short *)op->m.res_dev, batch,
                           op->cout, Ho, Wo, cout_pad);
    }
    hipLaunchKernelGGL(nchw_to_nhwc_bf16_kernel, dim3(grid_for(n_in)), dim3(256), 0, s, x_dev, (unsigned short *)op->m.in_dev, batch, op->cin, height,
                       width, op->cpad);
    const char *res = residual_dev ? op->m.res_dev : nullptr;
    if (op->geom) {
        ConvGeomParams p = geom_params(op->g, batch, height, width, Ho, Wo, in_pb, cout_pad, y355_convgeom_info(pl.kid)->bn);
        p.in = op->m.in_dev; p.w = op->m.w_dev; p.bias_f = op->m.bias_dev; p.res = res; p.out = op->m.out_dev;
        p.out_pb = (int)out_pb; p.out_f32 = out_fp32 ? 1 : 0; p.slope = op->slope;
        y355_launch_convgeom(pl.kid, 1, p, s);
    } else {
        const ConvGInfo &ki = *pl.kg;
        ConvGParams p{};
        p.in = op->m.in_dev; p.out = op->m.out_dev; p.w = op->m.w_dev; p.bias_f = op->m.bias_dev;
        p.B = batch; p.H = height; p.W = width;
        p.in_pb = in_pb; p.nchunks = in_pb / ki.chb;
        p.out_pb = (int)out_pb; p.out_off = 0; p.out_halo = 1;
        p.tiles_x = (Wo + ki.tw - 1) / ki.tw; p.tiles_y = (Ho + ki.th - 1) / ki.th; p.nblk = cout_pad / ki.bn;
        p.taps = op->ksize * op->ksize;
        p.slope = op->slope;
        p.out_f32 = out_fp32 ? 1 : 0;
        p.res = res; p.res_pb = (int)out_pb; p.res_off = 0;
        ki.launch(p, p.tiles_x * p.tiles_y * p.nblk * batch, s);
    }
    HIPCHK(hipGetLastError());
    if (out_fp32)
        hipLaunchKernelGGL(nhwc_f32_to_nchw_kernel, dim3(grid_for(n_out)), dim3(256), 0, s, (const float *)op->m.out_dev, out_dev, batch, op->cout, Ho,
                           Wo, cout_pad);
    else
        hipLaunchKernelGGL(nhwc_bf16_to_nchw_kernel, dim3(grid_for(n_out)), dim3(256), 0, s, (const unsigned short *)op->m.out_dev, out_dev, batch,
                           op->cout, Ho, Wo, cout_pad);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int y355_conv_op_forward(y355_conv_op *op, const float *x_dev, const float *residual_dev, int batch, int height, int width,
                                    int out_fp32, float *out_dev, void *stream) {
    if (!op || op->kind != 0 || !x_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument / not a bf16 operator");
    if (batch < 1 || height < 1 || width < 1) return y355_fail(Y355_EINVAL, "bad shape");
    return conv_forward_bf16(op, x_dev, residual_dev, batch, height, width, out_fp32, out_dev, (hipStream_t)stream);
}

// host-pointer form on a temporary operator (owned): upload x and the residual, the shared forward on the null stream,
// synchronise, download
static int bf16_host_form(y355_conv_op *op_, const float *x, const float *residual, int batch, int height, int width, int out_fp32, float *out) {
    OpOwner own{op_};
    ConvPlan pl;
    if (int rc = conv_out_size(own.op, batch, height, width, &pl)) return rc;
    const size_t n_in = (size_t)batch * own.op->cin * height * width, n_out = (size_t)batch * own.op->cout * pl.Ho * pl.Wo;
    DevScope tmp;
    float *d_x = nullptr, *d_r = nullptr, *d_y = nullptr;
    if (int rc = y355_dev_get(tmp, &d_x, n_in)) return rc;
    if (int rc = y355_dev_get(tmp, &d_y, n_out)) return rc;
    HIPCHK(hipMemcpy(d_x, x, n_in * 4, hipMemcpyHostToDevice));
    if (residual) {
        if (int rc = y355_dev_get(tmp, &d_r, n_out)) return rc;
        HIPCHK(hipMemcpy(d_r, residual, n_out * 4, hipMemcpyHostToDevice));
    }
    if (int rc = conv_forward_bf16(own.op, d_x, d_r, batch, height, width, out_fp32, d_y, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_y, n_out * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int y355_conv2d_bf16(int device_id, const float *x, const float *w, const float *bias, const float *residual,
                                int batch, int cin, int cout, int height, int width, int ksize, int stride, float neg_slope,
                                int out_fp32, float *out) {
    if (!x || !w || !out) return y355_fail(Y355_EINVAL, "null argument");
    if (batch < 1 || cin < 1 || cout < 1 || height < 1 || width < 1) return y355_fail(Y355_EINVAL, "bad shape");
    if (out_fp32 && residual) return y355_fail(Y355_EINVAL, "fp32 output (prediction layers) takes no residual");
    y355_conv_op *op = nullptr;
    if (int rc = y355_conv_op_create_bf16(device_id, w, bias, cin, cout, ksize, stride, neg_slope, &op)) return rc;
    return bf16_host_form(op, x, residual, batch, height, width, out_fp32, out);
}

extern "C" int y355_conv2d_geom_bf16(int device_id, const float *x, const float *w, const float *bias, const float *residual, int batch,
                                     int cin, int cout, int height, int width, const y355_conv_geom *g, float neg_slope, int out_fp32,
                                     float *out) {
    if (!x || !w || !out || !g) return y355_fail(Y355_EINVAL, "null argument");
    if (cin < 1 || cout < 1) return y355_fail(Y355_EINVAL, "bad shape");
    int Ho = 0, Wo = 0;
    if (int rc = geom_out(g, batch, height, width, &Ho, &Wo)) return rc;
    if (out_fp32 && residual) return y355_fail(Y355_EINVAL, "fp32 output (prediction layers) takes no residual");
    y355_conv_op *op = nullptr;
    if (int rc = y355_conv_op_create_bf16_geom(device_id, w, bias, cin, cout, g, neg_slope, &op)) return rc;
    return bf16_host_form(op, x, residual, batch, height, width, out_fp32, out);
}

// ---- int8 forward ----------------------------------------------------------------------------------------------------------
// "Run an int8 input at exponent sa": everything up to the staging of the input -- the kernel and its weights, the integer
// epilogue for this exponent (cached), the workspaces (in_dev zeroed where the staging does not write; *in_bytes its size).
static int i8_prepare(y355_conv_op *op, int batch, int height, int width, int sa, hipStream_t s, ConvPlan *pl, size_t *in_bytes) {
    if (int rc = conv_plan(op, batch, height, width, pl)) return rc;
    if (int rc = op_weights(op, *pl, s)) return rc;
    if (sa != op->sa_cached) {
        Y355RqLayer q;              // no requantisation (t' is the result), retune 10, the weights' own bound unknown
        if (int rc = y355_rq_fail(y355_rq_layer(op->cin, op->geom ? op->g.kh * op->g.kw : 9, sa, op->e_w, op->e_b, 0, false, op->act, 10,
                                                op->qb.data(), op->cout, pl->cout_pad, 0, &q)))
            return rc;
        op->rq = q.rq;
        op->frac_bits = q.frac_bits;
        if (op->m.bt_dev) HIPCHK(hipMemcpy(op->m.bt_dev, q.bias_t.data(), sizeof(int) * pl->cout_pad, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(op->m.bw_dev, q.bias_w.data(), sizeof(long long) * pl->cout_pad, hipMemcpyHostToDevice));
        op->sa_cached = sa;
    }
    // the 3x3 kernels prefetch past the last pixel: 64 pixels of slack
    *in_bytes = ((size_t)batch * (height + 2) * (width + 2) + (op->geom ? 0 : 64)) * op->cpad;
    const size_t raw_bytes = sizeof(long long) * (size_t)batch * pl->Ho * pl->Wo * pl->cout_pad;
    return op_workspaces(op, geo_word(batch, height, width, 0), *in_bytes, raw_bytes, false, 0, s);     // t' has no halo
}
// conv + bias + activation without requantisation on the staged input: t' [pixel][cout_pad] int64 into out_dev
static int i8_launch(y355_conv_op *op, const ConvPlan &pl, int batch, int height, int width, hipStream_t s) {
    if (op->geom) {
        ConvGeomParams p = geom_params(op->g, batch, height, width, pl.Ho, pl.Wo, op->cpad, pl.cout_pad, y355_convgeom_info(pl.kid)->bn);
        p.in = op->m.in_dev; p.w = op->m.w_dev; p.bias_w = op->m.bw_dev; p.raw = (long long *)op->m.out_dev;
        p.shl = op->rq.shl; p.lk = op->rq.lk; p.neg_mul = op->rq.neg_mul;
        y355_launch_convgeom(pl.kid, 0, p, s);
    } else {
        const ConvKernelInfo &ki = *y355_conv_kernel(pl.kid);
        HIPCHK(hipMemsetAsync(op->m.ctr_dev, 0, sizeof(Counters), s));
        ConvParams p = gen16_params(ki, (const int8_t *)op->m.in_dev, (const int8_t *)op->m.w_dev, op->m.bt_dev, op->m.bw_dev, op->m.ctr_dev, batch, height,
                                    width, pl.cout_pad, op->rq);
        p.raw = (long long *)op->m.out_dev; p.mode = 1; p.guard = 0;      // statistics mode dumps t'
        ki.launch(p, p.tiles_x * p.tiles_y * p.nblk * batch, s);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// Conv2d_fuse(x) for a dyadic x (utils/modules.py:20-29 on the fake-quantised operands of the quantized path): exact.
// *exact = 0: x is not a dyadic int8 tensor (out_dev untouched) -- the caller takes the bf16 route.
extern "C" int y355_conv_op_forward_i8(y355_conv_op *op, const float *x_dev, int batch, int height, int width, float *out_dev, void *stream,
                                       int32_t *sa_in, int32_t *exact) {
    if (!op || op->kind != 1 || !x_dev || !out_dev || !exact) return y355_fail(Y355_EINVAL, "null argument / not an int8 operator");
    ConvPlan pl;
    if (int rc = conv_out_size(op, batch, height, width, &pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(op->device));
    *exact = 0;
    const size_t n_in = (size_t)batch * op->cin * height * width, n_out = (size_t)batch * op->cout * pl.Ho * pl.Wo;
    // (1) the exponent of x: floor(log2(127 / max|x|)) -- the tensor is q / 2^e with |q| <= 127 (prep.as_dyadic_int8)
    HIPCHK(hipMemsetAsync(op->m.flag_dev, 0, 16, s));
    y355_launch_absmax(x_dev, n_in, op->m.flag_dev, s);
    HIPCHK(hipGetLastError());
    unsigned int bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, op->m.flag_dev, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float mx;
    memcpy(&mx, &bits, 4);
    if (!(mx > 0.f) || !std::isfinite(mx)) return 0;                              // all zero / not finite: not this route
    const int sa = (int)std::floor(std::log2((1.0f / mx) * 127.0f));
    if (sa < -64 || sa > 64) return 0;
    if (sa_in) *sa_in = sa;
    // (2) weights, integer epilogue, workspaces; (3) stage: int8 NHWC with halo + the dyadic verdict
    size_t in_bytes = 0;
    if (int rc = i8_prepare(op, batch, height, width, sa, s, &pl, &in_bytes)) return rc;
    hipLaunchKernelGGL(dyadic_to_nhwc_i8_kernel, dim3(grid_for(n_in)), dim3(256), 0, s, x_dev, (int8_t *)op->m.in_dev, batch, op->cin, height, width,
                       op->cpad, std::ldexp(1.0f, sa), op->m.flag_dev + 1);
    HIPCHK(hipGetLastError());
    unsigned int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, op->m.flag_dev + 1, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return 0;
    // (4) the convolution, (5) t' / 2^F' -> fp32 NCHW
    if (int rc = i8_launch(op, pl, batch, height, width, s)) return rc;
    hipLaunchKernelGGL(raw_to_nchw_f32_kernel, dim3(grid_for(n_out)), dim3(256), 0, s, (const long long *)op->m.out_dev, out_dev, batch, op->cout, pl.Ho,
                       pl.Wo, pl.cout_pad, std::ldexp(1.0f, -op->frac_bits));
    HIPCHK(hipGetLastError());
    *exact = 1;
    return 0;
}

// conv + bias + activation WITHOUT requantisation on caller data: t' (int64) and F' such that the reference's Conv2d_fuse
// output is exactly t' / 2^F' (utils/modules.py:20-29 on fake-quantized operands).  The input is int8 at the GIVEN exponent
// sa_in, so these forms enter below the exponent detection.  Host pointers, synchronous, on a temporary operator (owned).
static int i8_raw_host_form(y355_conv_op *op_, const int8_t *q_in, int batch, int height, int width, int sa_in, int64_t *out, int32_t *frac_bits) {
    OpOwner own{op_};
    y355_conv_op *op = own.op;
    ConvPlan pl;
    size_t in_bytes = 0;
    if (int rc = conv_out_size(op, batch, height, width, &pl)) return rc;
    if (int rc = i8_prepare(op, batch, height, width, sa_in, nullptr, &pl, &in_bytes)) return rc;
    const std::vector<int8_t> xin = nhwc_halo_i8(q_in, batch, op->cin, height, width, op->cpad, in_bytes);
    HIPCHK(hipMemcpy(op->m.in_dev, xin.data(), in_bytes, hipMemcpyHostToDevice));
    if (int rc = i8_launch(op, pl, batch, height, width, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    std::vector<long long> o((size_t)batch * pl.Ho * pl.Wo * pl.cout_pad);
    HIPCHK(hipMemcpy(o.data(), op->m.out_dev, sizeof(long long) * o.size(), hipMemcpyDeviceToHost));
    nhwc_to_nchw(o.data(), out, batch, op->cout, pl.Ho, pl.Wo, pl.cout_pad);
    *frac_bits = op->frac_bits;
    return 0;
}

extern "C" int y355_conv3x3_i8_raw(int device_id, const int8_t *q_in, const int8_t *q_w, const int32_t *q_b, int batch, int cin, int cout,
                                   int H, int W, int sa_in, int e_w, int e_b, int flags, int64_t *out, int32_t *frac_bits) {
    if (!q_in || !q_w || !q_b || !out || !frac_bits) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = gen16_shape(batch, cin, cout, H, W, flags)) return rc;
    y355_conv_op *op = nullptr;
    if (int rc = y355_conv_op_create_i8(device_id, q_w, q_b, cin, cout, e_w, e_b, flags, &op)) return rc;
    return i8_raw_host_form(op, q_in, batch, H, W, sa_in, out, frac_bits);
}

extern "C" int y355_conv_geom_i8_raw(int device_id, const int8_t *q_in, const int8_t *q_w, const int32_t *q_b, int batch, int cin, int cout,
                                     int height, int width, const y355_conv_geom *g, int sa_in, int e_w, int e_b, int flags, int64_t *out,
                                     int32_t *frac_bits) {
    if (!q_in || !q_w || !q_b || !out || !frac_bits || !g) return y355_fail(Y355_EINVAL, "null argument");
    if (cin < 1 || cout < 1) return y355_fail(Y355_EINVAL, "bad shape");
    int Ho = 0, Wo = 0;
    if (int rc = geom_out(g, batch, height, width, &Ho, &Wo)) return rc;
    y355_conv_op *op = nullptr;
    if (int rc = y355_conv_op_create_i8_geom(device_id, q_w, q_b, cin, cout, g, e_w, e_b, flags, &op)) return rc;
    return i8_raw_host_form(op, q_in, batch, height, width, sa_in, out, frac_bits);
}

// The fused layer on caller data (utils/modules.py Conv2d_fuse drop-in, unit tests): conv + bias + activation [+ 2x2 max-pool]
// requantised to sa_out.  Two passes: statistics (max |t'|), then the requantised one that stores and counts saturations.
extern "C" int y355_conv3x3_i8_fused(int device_id, const int8_t *q_in, const int8_t *q_w, const int32_t *q_b, int batch, int cin, int cout,
                                     int H, int W, int sa_in, int e_w, int e_b, int sa_out, int flags, int8_t *out, y355_layer_stats *stats) {
    if (!q_in || !q_w || !q_b || !out) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = gen16_shape(batch, cin, cout, H, W, flags)) return rc;
    const int pool = (flags & Y355_OP_POOL) ? 1 : 0;
    if (pool && ((H | W) & 1)) return y355_fail(Y355_EINVAL, "pooling needs even H, W");
    HIPCHK(hipSetDevice(device_id));
    if (int e = y355_prepare_kernels()) return e;
    int cpad = 0;
    const ConvKernelInfo &ki = *y355_conv_kernel(gen16_kernel(cin, pool, &cpad));
    const int cout_pad = round_up(cout, ki.bn), Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    Y355RqLayer q;
    if (int rc = y355_rq_fail(y355_rq_layer(cin, 9, sa_in, e_w, e_b, sa_out, true, geom_act(flags), 10, q_b, cout, cout_pad, 0, &q))) return rc;
    const size_t in_bytes = ((size_t)batch * (H + 2) * (W + 2) + 64) * cpad, out_elems = (size_t)batch * Ho * Wo * cout_pad;
    const std::vector<int8_t> xin = nhwc_halo_i8(q_in, batch, cin, H, W, cpad, in_bytes);
    std::vector<int8_t> packed(y355_packed_bytes(ki, cout_pad));
    y355_pack_weights(ki, q_w, cout, cin, cout_pad, packed.data());
    DevScope tmp;
    int8_t *d_in = nullptr, *d_w = nullptr, *d_out = nullptr;
    int *d_b = nullptr;
    long long *d_bw = nullptr;
    Counters *d_c = nullptr;
    if (int rc = y355_dev_get(tmp, &d_in, in_bytes)) return rc;
    if (int rc = y355_dev_get(tmp, &d_w, packed.size())) return rc;
    if (int rc = y355_dev_get(tmp, &d_out, out_elems + 64)) return rc;
    if (int rc = y355_dev_get(tmp, &d_b, (size_t)cout_pad)) return rc;
    if (int rc = y355_dev_get(tmp, &d_bw, (size_t)cout_pad)) return rc;
    if (int rc = y355_dev_get(tmp, &d_c, 1)) return rc;
    HIPCHK(hipMemcpy(d_in, xin.data(), in_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_w, packed.data(), packed.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_b, q.bias_t.data(), sizeof(int) * cout_pad, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_bw, q.bias_w.data(), sizeof(long long) * cout_pad, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0, out_elems + 64));
    Counters cz{}, cs{};
    for (int mode = 1; mode >= 0; --mode) {
        HIPCHK(hipMemset(d_c, 0, sizeof(Counters)));
        ConvParams p = gen16_params(ki, d_in, d_w, d_b, d_bw, d_c, batch, H, W, cout_pad, q.rq);
        p.out = d_out; p.mode = mode; p.guard = 1;
        ki.launch(p, p.tiles_x * p.tiles_y * p.nblk * batch, 0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(mode ? &cs : &cz, d_c, sizeof(Counters), hipMemcpyDeviceToHost));
    }
    std::vector<int8_t> o(out_elems);
    HIPCHK(hipMemcpy(o.data(), d_out, out_elems, hipMemcpyDeviceToHost));
    nhwc_to_nchw(o.data(), out, batch, cout, Ho, Wo, cout_pad);
    if (stats) {
        stats->absmax_t = (int64_t)cs.absmax;
        stats->frac_bits = q.frac_bits;
        stats->reserved = 0;
        stats->saturated = (int64_t)cz.sat;
        stats->guard = (int64_t)cz.guard;
    }
    return 0;
}
