// yolo355 -- cv2.resize(image, (W, H)) of BaseTransform (data/__init__.py:36) for uint8 HWC frames, INTER_LINEAR: OpenCV's 8-bit
// fixed-point bilinear (imgproc/resize.cpp: 11-bit coefficients, horizontal pass in int32, vertical pass
// (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2).  The coefficient tables are computed on the host with
// OpenCV's own float / double expressions, so the kernel only gathers and does integer arithmetic (y355_resize_px,
// y355_common.h: the stage of the q_bf engine's y355_forward_u8_resized and of y355_net_forward_u8, where the net's
// input op also runs it fused into its own load).
// Horizontal axis: OpenCV clamps the offset AND zeroes the fraction at both borders.  Vertical axis (`vertical`): it keeps
// floor(f) and the coefficient pair as they are and clips the two ROW INDICES instead (resizeGeneric_Invoker:
// `sy = clip(sy0 - ksize2 + 1 + k, 0, ssize.height)`), so a border row is blended with itself through two separately
// truncated products -- up to 1 LSB below the single-product form; the kernel does the same clipping.
#include "y355_common.h"

#include <algorithm>
#include <cmath>

static void linear_tables(int src, int dst, int *ofs, int *coef, bool vertical) {
    const double scale = (double)src / (double)dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int sx = (int)std::floor(f);
        f -= (float)sx;
        if (!vertical && sx < 0) { sx = 0; f = 0.f; }
        if (!vertical && sx >= src - 1) { sx = src - 1; f = 0.f; }
        ofs[d] = sx;
        const long c0 = std::lrintf((1.f - f) * 2048.f), c1 = std::lrintf(f * 2048.f);     // saturate_cast<short>: round half to even
        coef[2 * d] = (int)std::min(32767l, std::max(-32768l, c0));
        coef[2 * d + 1] = (int)std::min(32767l, std::max(-32768l, c1));
    }
}

void y355_resize_tables(int sh, int sw, int dh, int dw, int *tab) {
    linear_tables(sw, dw, tab, tab + dw, false);
    linear_tables(sh, dh, tab + 3 * dw, tab + 3 * dw + dh, true);
}

__global__ __launch_bounds__(256) void resize_u8_kernel(const uint8_t *src, uint8_t *dst, const int *tab, int sh, int sw, int dh, int dw) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * dw) return;
    int v[3];
    y355_resize_px(src + (size_t)b * sh * sw * 3, tab, sh, sw, dh, dw, i / dw, i % dw, v);
    uint8_t *d = dst + ((size_t)b * dh * dw + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (uint8_t)v[c];
}

void y355_launch_resize_u8(const uint8_t *src, uint8_t *dst, const int *tab, int B, int sh, int sw, int dh, int dw, hipStream_t s) {
    hipLaunchKernelGGL(resize_u8_kernel, dim3((dh * dw + 255) / 256, B), dim3(256), 0, s, src, dst, tab, sh, sw, dh, dw);
}
