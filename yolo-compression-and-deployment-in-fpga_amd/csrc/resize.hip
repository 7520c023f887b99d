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
// Frame lists (y355_net_forward_frames): the ragged stage at the end of this file builds the same tables on the device.
#include "../../include/yolo355.h"
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

// ---- a list of frames, each with its own pointer, size and row pitch (y355_net_forward_frames): every frame's tables are
// built on the device (no host table, no upload, nothing to keep alive between calls), then one launch resizes the list.
struct RsFrame {
    const uint8_t *src;
    long long pitch;        // bytes of one source row
    int sh, sw;
};
constexpr int kRsChunk = 64;                  // frames per launch: 64 x 24 bytes of kernel arguments
struct RsChunk {
    RsFrame f[kRsChunk];
};

// linear_tables on the device, one thread per table entry: the same double / float operations in the same order, every one
// rounded on its own (no fused multiply-add), so the entries are the host's bit for bit
__global__ __launch_bounds__(256) void resize_tables_kernel(RsChunk ch, int *tabs, int dh, int dw) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= dh + dw) return;
    const RsFrame &fr = ch.f[blockIdx.y];
    int *tab = tabs + (size_t)blockIdx.y * 3 * (dh + dw);
    const bool vertical = t >= dw;
    const int d = vertical ? t - dw : t, src = vertical ? fr.sh : fr.sw, dst = vertical ? dh : dw;
    int *ofs = vertical ? tab + 3 * dw : tab, *coef = vertical ? tab + 3 * dw + dh : tab + dw;
    const double scale = __ddiv_rn((double)src, (double)dst);
    float f = __double2float_rn(__dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5));
    int sx = (int)floorf(f);
    f = __fsub_rn(f, (float)sx);
    if (!vertical && sx < 0) { sx = 0; f = 0.f; }
    if (!vertical && sx >= src - 1) { sx = src - 1; f = 0.f; }
    ofs[d] = sx;
    const long c0 = lrintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f)), c1 = lrintf(__fmul_rn(f, 2048.f));
    coef[2 * d] = (int)min(32767l, max(-32768l, c0));
    coef[2 * d + 1] = (int)min(32767l, max(-32768l, c1));
}

// four consecutive pixels of one output row per thread (dw is a multiple of 4): 12 bytes, stored as three dwords when the
// destination is dword-aligned (DW).  y355_resize_px's arithmetic; the source is read byte by byte (no alignment assumed)
template <bool DW>
__global__ __launch_bounds__(256) void resize_frames_kernel(RsChunk ch, uint8_t *dst, const int *tabs, int dh, int dw) {
    const int gw = dw >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * gw) return;
    const int b = blockIdx.y, dy = i / gw, dx0 = (i - dy * gw) * 4;
    const RsFrame fr = ch.f[b];
    const int *tab = tabs + (size_t)b * 3 * (dh + dw);
    const int *xofs = tab, *xa = tab + dw, *yofs = tab + 3 * dw, *yb = tab + 3 * dw + dh;
    const int sy = yofs[dy], b0 = yb[2 * dy], b1 = yb[2 * dy + 1];
    const uint8_t *r0 = fr.src + (long long)min(max(sy, 0), fr.sh - 1) * fr.pitch;
    const uint8_t *r1 = fr.src + (long long)min(max(sy + 1, 0), fr.sh - 1) * fr.pitch;
    unsigned int w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int dx = dx0 + p;
        const int sx0 = xofs[dx] * 3, sx1 = min(xofs[dx] + 1, fr.sw - 1) * 3, a0 = xa[2 * dx], a1 = xa[2 * dx + 1];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d0 = (int)r0[sx0 + c] * a0 + (int)r0[sx1 + c] * a1;
            const int d1 = (int)r1[sx0 + c] * a0 + (int)r1[sx1 + c] * a1;
            const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
            const int k = p * 3 + c;
            w[k >> 2] |= (unsigned int)min(max(v, 0), 255) << (8 * (k & 3));
        }
    }
    uint8_t *o = dst + ((size_t)b * dh * dw + (size_t)dy * dw + dx0) * 3;
    if (DW) {
        unsigned int *o4 = (unsigned int *)o;
        o4[0] = w[0];
        o4[1] = w[1];
        o4[2] = w[2];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

void y355_launch_resize_frames(const y355_frame *frames, int n, uint8_t *dst, int *tabs, int dh, int dw, hipStream_t s) {
    const bool dword = ((uintptr_t)dst & 3) == 0;
    for (int i0 = 0; i0 < n; i0 += kRsChunk) {
        const int m = std::min(kRsChunk, n - i0);
        RsChunk ch{};
        for (int k = 0; k < m; ++k) {
            const y355_frame &f = frames[i0 + k];
            ch.f[k] = RsFrame{f.data_dev, f.row_bytes ? (long long)f.row_bytes : 3ll * f.width, f.height, f.width};
        }
        int *tab = tabs + (size_t)i0 * 3 * (dh + dw);
        uint8_t *out = dst + (size_t)i0 * dh * dw * 3;
        hipLaunchKernelGGL(resize_tables_kernel, dim3((dh + dw + 255) / 256, m), dim3(256), 0, s, ch, tab, dh, dw);
        const dim3 grid((dh * (dw >> 2) + 255) / 256, m);
        if (dword) hipLaunchKernelGGL(resize_frames_kernel<true>, grid, dim3(256), 0, s, ch, out, tab, dh, dw);
        else hipLaunchKernelGGL(resize_frames_kernel<false>, grid, dim3(256), 0, s, ch, out, tab, dh, dw);
    }
}

// ---- the stage's host state (FrameStage, y355_common.h)
void y355_stage_init(FrameStage &st, int H, int W, int max_batch, const DevMem &mem) {
    st = FrameStage{};
    st.H = H;
    st.W = W;
    st.max_batch = max_batch;
    st.own.mem = mem;
}

void y355_stage_destroy(FrameStage &st) {
    y355_dev_release_all(st.own);
    st.tab = st.tabs = nullptr;
    st.frames = nullptr;
    st.src_h = st.src_w = 0;
}

int y355_stage_set_normalization(FrameStage &st, const float *mean_bgr, const float *std_bgr) {
    for (int c = 0; c < 3; ++c)
        if (!(std_bgr[c] > 0.f)) return y355_fail(Y355_EINVAL, "std must be positive");
    for (int c = 0; c < 3; ++c) {
        st.norm.mean[c] = mean_bgr[2 - c];
        st.norm.sd[c] = std_bgr[2 - c];
    }
    return 0;
}

int y355_stage_need_frames(FrameStage &st) { return st.frames ? 0 : y355_dev_get(st.own, &st.frames, (size_t)st.max_batch * st.H * st.W * 3); }
int y355_stage_need_list(FrameStage &st) { return st.tabs ? 0 : y355_dev_get(st.own, &st.tabs, 3 * (size_t)(st.H + st.W) * st.max_batch); }

int y355_stage_tables_for(FrameStage &st, int src_h, int src_w, hipStream_t s) {
    std::vector<int> tab(3 * (size_t)(st.H + st.W));
    if (!st.tab)
        if (int rc = y355_dev_get(st.own, &st.tab, tab.size())) return rc;
    if (st.src_h == src_h && st.src_w == src_w) return 0;
    y355_resize_tables(src_h, src_w, st.H, st.W, tab.data());
    // (the upload waits for s: a previous forward may still read the old tables)
    if (int rc = st.own.mem.upload(st.tab, tab.data(), sizeof(int) * tab.size(), s)) {
        st.src_h = st.src_w = 0;        // the old tables may be partly overwritten
        return rc;
    }
    st.src_h = src_h;
    st.src_w = src_w;
    return 0;
}

int y355_frames_check(const y355_frame *frames, int batch, int max_batch) {
    if (!frames) return y355_fail(Y355_EINVAL, "null frame array");
    if (batch < 1 || batch > max_batch) return y355_fail(Y355_EINVAL, "batch out of range");
    for (int i = 0; i < batch; ++i) {
        const y355_frame &f = frames[i];
        if (!f.data_dev) return y355_fail(Y355_EINVAL, "null frame pointer");
        if (f.height < 1 || f.width < 1 || f.height > 16384 || f.width > 16384) return y355_fail(Y355_EINVAL, "bad frame size");
        if (f.row_bytes != 0 && f.row_bytes < 3 * (int64_t)f.width) return y355_fail(Y355_EINVAL, "row_bytes below width * 3");
    }
    return 0;
}
