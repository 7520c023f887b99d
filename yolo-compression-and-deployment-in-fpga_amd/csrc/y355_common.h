// yolo355 -- shared device/host declarations of libyolo355.so (gfx950 only).  The host-side pieces that need no kernel parameter
// struct -- y355_fail, HIPCHK, DevMem and its HIP form, DevOwner (users: HeadState, FrameStage, HandleCore, y355_apeval,
// y355_pipeline, and in the companion libraries y355_loss and y355_anchors) -- are y355_host.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_ext.h>
#include "y355_host.h"      // y355_fail, HIPCHK, DevMem / DevOwner: the host-side pieces the companion libraries share
#include "y355_requant.h"   // Requant, RequantG, ResQ and their host-side derivation: the fixed-point epilogue's constants
inline int y355_rq_fail(const Y355RqErr &e) { return e.code ? y355_fail(e.code, e.msg) : 0; }      // a refusal of y355_requant.h as a y355 error

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
#define Y355_STAMP_ROWS 4096      // rows of 32 stamps in the diagnostic builds' stamp buffer (y355_debug_stamps)

// launch; with both events given the launch records its own start / end timestamps into them (profile mode 2: the
// duration rocprofv3 reports for the kernel, without the gap to the neighbouring launches)
#define Y355_LAUNCH(kernel, grid, block, lds, stream, e0, e1, ...)                                                       \
    do {                                                                                                                 \
        if ((e0) && (e1)) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, (hipEvent_t)(e0), (hipEvent_t)(e1), 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                          \
    } while (0)

__device__ __forceinline__ int y355_rne_shift32(int x, int s) {            // s wave-uniform
    if (s <= 0) return x << (-s);
    return (x + (1 << (s - 1)) - 1 + ((x >> s) & 1)) >> s;
}
// q before clamping for a LeakyReLU slope neg_mul / 2^lk that is not a power of two, 32-bit (Requant::gen32)
// (t = acc * 2^shl + bias is the caller's: shl is rq.shl for a per-tensor epilogue, a per-lane value for a per-channel one)
__device__ __forceinline__ int y355_requant_gen32_t(int t, const Requant &rq) {
    const int qp = y355_rne_shift32(t, rq.sh - rq.lk);
    int qn;
    if (rq.split) {                                    // wave-uniform
        // t = 256 hi + lo (0 <= lo < 256):  t * neg_mul = 256 A + rem  with  A = hi * neg_mul + (lo * neg_mul >> 8),
        // rem = lo * neg_mul & 255.  RNE((256 A + rem) / 2^sh) = RNE of A / 2^(sh - 8) in which a non-zero rem turns an exact
        // tie into "above the tie": the usual half - 1 + lsb rounding add with lsb forced to 1
        const int hi = t >> 8, m2 = (t & 255) * rq.neg_mul;
        const int A = hi * rq.neg_mul + (m2 >> 8);
        const int s = rq.sh - 8;
        qn = (A + ((1 << (s - 1)) - 1) + ((((m2 & 255) + 255) >> 8) | ((A >> s) & 1))) >> s;
    } else {
        qn = y355_rne_shift32(t * rq.neg_mul, rq.sh);
    }
    return t >= 0 ? qp : qn;
}
__device__ __forceinline__ int y355_requant_gen32(int acc, int bias, const Requant &rq) {
    return y355_requant_gen32_t((acc << rq.shl) + bias, rq);
}
// Bias word of the 32-bit epilogues of y355_net's int8 convolutions (convg.hip NARROW, convr.hip): the pre-shifted bias fits
// 32 bits there, so the upper half of the 64-bit word carries the output channel's own accumulator shift shl[c] = F - sa_in -
// e_w[c] (per-channel weight exponents; all equal for a per-tensor layer).  One load per channel, as before; the shift amount
// is per lane, no longer wave-uniform.
__host__ __device__ __forceinline__ long long y355_pc_word(int shl, int bias) {
    return (long long)(((unsigned long long)(unsigned int)shl << 32) | (unsigned int)bias);
}
__device__ __forceinline__ int y355_pc_t(int acc, long long word) { return (acc << (int)(word >> 32)) + (int)word; }

// q before clamping, 32-bit, no branches (production kernels)
__device__ __forceinline__ int y355_requant_fast(int acc, int bias, const Requant &rq) {
    int t = (acc << rq.shl) + bias;
    t = max(t, t << rq.lk);
    const int rb = (int)__builtin_amdgcn_ubfe((unsigned int)t, (unsigned int)rq.sh_r, (unsigned int)rq.bw);
    return ((t << rq.sh_l) + rq.hm1 + rb) >> rq.sh_r;
}

struct Counters {
    unsigned long long absmax;   // max |t'| (stats mode)
    unsigned long long in_sat;   // layer 0 only: clamped input pixels
    unsigned long long sat;   // clamped outputs
    unsigned long long guard; // head-room violations
};

// engine.hip, for the other translation units
int y355_prepare_kernels();                          // one-time kernel attributes of the int8 engine's kernels; a y355 error code
int y355_cu_count(void);       // engine.hip: compute units of the current device (cached per device), 256 on an MI355X in SPX mode
int y355_zero_counters(Counters *c, int n, hipStream_t s);    // engine.hip: a kernel launch, not hipMemsetAsync; returns the launch status (hipError_t)

// Two sets of per-forward counters used alternately: the fused front end of forward i (the first launch of a step) zeroes the
// set forward i + 1 will count into, so the steady state has NO counter-reset launch (round 5: a one-wave kernel per step,
// 4.5 us of a 298 us one-stream step).  Every launch of a stream runs behind the previous one, so the set being zeroed is idle:
// forward i - 1 (its last user) is complete, forward i counts into the other one, and a host read of "the last forward's
// counters" happens before the next forward is enqueued.  A forward without the fused front end zeroes its own set by a launch.
struct CounterSets {
    Counters *base = nullptr;     // [2][n]
    int n = 0, cur = 0;
    bool clean[2] = {false, false};
    Counters *set(int i) const { return base + (size_t)i * n; }
    // start a forward: the set it counts into; *need_zero: not zeroed by the previous forward's front end
    Counters *begin(bool *need_zero) {
        cur ^= 1;
        *need_zero = !clean[cur];
        clean[cur] = false;
        return set(cur);
    }
    // this forward's front end zeroes the other set (call when that launch is enqueued)
    Counters *other_zeroed_by_front() {
        clean[cur ^ 1] = true;
        return set(cur ^ 1);
    }
};

struct ConvParams {
    const int8_t *in;     // int8 NHWC with halo  [B][H+2][W+2][CIN]
    int8_t *out;          // int8 NHWC [B][Ho+2h][Wo+2h][cstride]
    const int8_t *w;      // fragment-packed weights
    const int *bias_t;    // [cout_pad]
    const long long *bias_w;  // [cout_pad] 64-bit copy for the wide epilogue
    Counters *ctr;
    int8_t *sink;         // >= 4 KiB scratch for masked-out stores (keeps store counts static)
    long long *raw;       // statistics mode: optional dump of t' as [B][H][W][cstride] (operator API)
    unsigned long long *stamps;   // diagnostic builds only: per-workgroup s_memtime stamps (or null)
    int B, H, W;          // input feature-map size (unpadded)
    int cstride;          // channels of the output buffer
    int out_halo;         // 1: output buffer carries a zero halo
    int tiles_x, tiles_y, nblk;
    Requant rq;
    int mode;             // 0 run, 1 statistics only
    int guard;            // evaluate the head-room guard
    // host side only (ring launcher): when set, the launch records the kernel's own start / end timestamps into these
    // events (hipExtLaunchKernelGGL) -- the duration rocprofv3 reports, without the gap to the neighbouring launches
    void *ev_start, *ev_stop;
    int grid_limit;       // host side only: persistent workgroups of a ring launch (0 = one per CU), Y355_OPT_RING_WORKGROUPS
    int xcd_share_log2;   // ring kernels: work items that read one input are walked by workgroups of one XCD (set by the launcher)
};

struct Conv1Params {
    const float *x;       // fp32 NCHW [B][3][H][W]
    const uint8_t *x_u8;  // or (x == nullptr) camera frames uint8 HWC BGR [B][H][W][3], normalised on the fly
    float nmean[3], nstd[3];  // BaseTransform constants per RGB channel (data/__init__.py:50)
    int8_t *out;          // int8 NHWC16 with halo [B][H/2+2][W/2+2][16]
    int out_pb;           // bytes per output pixel (0 = 16; wider: the extra bytes stay untouched)
    const int8_t *w;      // 64 lanes x 16 B fragment
    const int *bias_t;    // [16]
    const long long *bias_w;
    const int *shl_c;     // [16] accumulator shift per output channel (per-channel weight exponents), or null: rq.shl
    Counters *ctr;
    int B, H, W;
    int tiles_x, tiles_y;
    float in_scale;       // 2^sa[0]
    Requant rq;
    int mode;
    int guard;
};

// fused front end (front.hip): network input -> conv1 + pool1 -> conv2 + pool2
struct FrontParams {
    const float *x;       // fp32 NCHW [B][3][H][W]
    const uint8_t *x_u8;  // or (x == nullptr) uint8 HWC BGR frames [B][H][W][3]
    float nmean[3], nstd[3];
    int8_t *out;          // conv2's pooled output: int8 NHWC32 with halo [B][H/4+2][W/4+2][32]
    const int8_t *wf;     // 16 KiB of weight fragments (y355_pack_front)
    const int *bias1;     // [16]
    const int *bias2;     // [32]
    Counters *ctr;        // [0] conv1, [1] conv2
    unsigned long long *zero_next;   // or null: zero_n 64-bit words the first workgroup clears (the NEXT forward's counters, CounterSets)
    int zero_n;
    int B, H, W;
    int tiles_x, tiles_y;
    float in_scale;       // 2^sa[0]
    float in_thr;         // set by the launcher: 127.5 / in_scale
    int step_x, step_y, step_b;   // set by the launcher: the grid size split as (tiles_x, tiles_y, batch) digits (front.hip's tile walk)
    Requant rq1, rq2;
    unsigned long long *stamps;   // diagnostic builds only (-DFRONT_DIAG=1)
    void *ev_start, *ev_stop;     // host side only: see ConvParams
};
// fused front end of the bf16 nets (frontb.hip): fp32 NCHW (or uint8 frames) -> conv(3 -> 16) + pool -> conv(16 -> 32) + pool -> bf16 NHWC
struct FrontBParams {
    const float *x;       // fp32 NCHW [B][3][H][W]
    const uint8_t *x_u8;  // or (x == nullptr) uint8 HWC BGR frames [B][H][W][3]
    float nmean[3], nstd[3];
    char *out;            // conv2's pooled output: bf16 NHWC with halo [B][H/4+2][W/4+2][out_pb bytes], channels 0..31
    int out_pb;           // bytes per output pixel (64)
    const char *wf;       // 32 KiB of weight fragments (y355_pack_frontb)
    const float *bias1;   // [16]
    const float *bias2;   // [32]
    int B, H, W;
    int tiles_x, tiles_y;
    float slope1, slope2; // LeakyReLU slopes of the two layers, each in [0, 1] (the kernel takes max(m, m * slope))
    int step_x, step_y, step_b;   // set by the launcher: the grid size split as (tiles_x, tiles_y, batch) digits (the tile walk)
};
void y355_frontb_tiles(int H, int W, int *tx, int *ty);
void y355_pack_frontb(const float *w1 /*[16][3][3][3] or null*/, const float *w2 /*[32][16][3][3] or null*/, char *dst /*32768*/);
void y355_launch_frontb(const FrontBParams &p, hipStream_t s);
void y355_front_tiles(int H, int W, int *tx, int *ty);
void y355_pack_front(const int8_t *q_w1, const int8_t *q_w2, int8_t *dst /*16384; a null tensor leaves its part zero*/);
bool y355_front_eligible(const Requant &rq1, const Requant &rq2);
void y355_launch_front(const FrontParams &p, hipStream_t s);

// fp32 -> bf16 bits on the host, round to nearest-even as the device's conversion (a NaN stays a quiet NaN): the weight packers
inline unsigned short y355_bf16_rne(float v) {
    unsigned int u;
    memcpy(&u, &v, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <typename T>
__device__ __forceinline__ T y355_rne_shift(T t, int sh) {
    if (sh > 0) {
        return (t + (((T)1 << (sh - 1)) - 1) + ((t >> sh) & 1)) >> sh;
    }
    return t * ((T)1 << (-sh));
}

template <typename T>
__device__ __forceinline__ T y355_pre(int acc, T bias, const Requant &rq) {
    T t = (T)acc * ((T)1 << rq.shl) + bias;
    if (rq.leaky) t = t >= 0 ? t * ((T)1 << rq.lk) : t * (T)rq.neg_mul;
    return t;
}

template <typename T> struct UnsignedOf { using type = unsigned int; };
template <> struct UnsignedOf<long long> { using type = unsigned long long; };
template <typename T>
__device__ __forceinline__ typename UnsignedOf<T>::type y355_uabs(T v) {
    return (typename UnsignedOf<T>::type)(v < 0 ? -v : v);
}

template <typename T>
__device__ __forceinline__ int y355_clamp8(T q) { return (int)min((T)127, max((T)-127, q)); }

// Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous chunk of tile ids
// so neighbouring tiles (shared halo rows, same weights) hit the same L2.  Bijective for any n.
__device__ __forceinline__ int y355_xcd_remap(int bid, int n) {
    const int q = n >> 3, r = n & 7, x = bid & 7, k = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

__device__ __forceinline__ unsigned int y355_wave_max_u32(unsigned int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned int)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long y355_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int lo = (unsigned int)__shfl_xor((int)(unsigned int)v, o, 64);
        const unsigned int hi = (unsigned int)__shfl_xor((int)(unsigned int)(v >> 32), o, 64);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// conv3_1 (32 -> 64 channels at a quarter of the input resolution) tile geometry, shared by the generic kernel
// (conv3x3.hip, always 4 waves: GWM x WN); the weight packing depends on WN
#ifndef Y355_C31_TH
#define Y355_C31_TH 13
#define Y355_C31_TW 52
#define Y355_C31_WM 4
#define Y355_C31_WN 2
#endif
#define Y355_C31_GWM (4 / Y355_C31_WN)

// ---- host-side launch table --------------------------------------------------------------
struct ConvKernelInfo {
    int cin, bn, th, tw, pool, wm, wn;
    int nt, ks;
    size_t lds_bytes;
    void (*launch)(const ConvParams &p, int nblocks, hipStream_t s);
    int (*prepare)(void);     // one-time hipFuncSetAttribute
};

// pack q_w[cout][cin][3][3] into the fragment order kernel `ki` streams (host buffers).
void y355_pack_weights(const ConvKernelInfo &ki, const int8_t *q_w, int cout, int cin,
                       int cout_pad, int8_t *dst);
size_t y355_packed_bytes(const ConvKernelInfo &ki, int cout_pad);
const ConvKernelInfo *y355_conv_kernel(int id);
enum {
    Y355_K_CONV2 = 0, Y355_K_CONV3_1, Y355_K_CONV3_2, Y355_K_CONV4_1, Y355_K_CONV4_2,
    Y355_K_CONV5, Y355_K_CONV67, Y355_K_PRED,
    Y355_K_GEN16, Y355_K_GEN32, Y355_K_GEN64, Y355_K_GEN128, Y355_K_GEN256,
    Y355_K_GEN16P, Y355_K_GEN32P, Y355_K_GEN64P, Y355_K_GEN128P, Y355_K_GEN256P,
    Y355_K_COUNT
};

// conv3_1 .. conv4_2 with the weights in registers and the pixels as the MFMA's B operand (convpx.hip); p.w = y355_pack_px layout
bool y355_launch_conv_px(int kid, const ConvParams &p, hipStream_t s);
int y355_prepare_conv_px(void);
size_t y355_px_packed_bytes(int kid);           // 0: the layer has no such kernel
bool y355_pack_px(int kid, const int8_t *q_w, int cout, int cin, int8_t *dst);
// conv3_1 -> conv3_2 + pool in one launch (pxpair.hip): conv3_1's map stays in LDS
struct PairParams {
    const int8_t *in;     // conv3_1's input: int8 NHWC32 with halo [B][H+2][W+2][32]
    int8_t *out;          // conv3_2's pooled output: int8 NHWC64 with halo [B][H/2+2][W/2+2][64]
    const int8_t *w1;     // conv3_1's weights, y355_pack_px(Y355_K_CONV3_1) layout
    const int8_t *w2;     // conv3_2's weights, y355_pack_px(Y355_K_CONV3_2) layout
    const int *bias1;     // [64]
    const int *bias2;     // [64]
    Counters *ctr1, *ctr2;
    Requant rq1, rq2;
    int B, H, W;          // conv3_1's map (= its input's size, unpadded)
    void *ev_start, *ev_stop;     // host side only: see ConvParams
    int grid_limit;       // host side only: persistent workgroups per launch (0 = one per CU)
    unsigned long long *stamps;   // diagnostic builds only (-DPAIR_DIAG=1)
};
bool y355_pair3_eligible(const Requant &rq1, const Requant &rq2, int H, int W);
bool y355_launch_pair3(const PairParams &p, hipStream_t s);      // false: not eligible, run the two layers' own launches
int y355_prepare_pair3(void);
// deep-prefetch ring kernels (conv3x3_ring.hip), layers with >= 64 input channels
bool y355_launch_conv_ring(int kid, const ConvParams &p, hipStream_t s);
int y355_prepare_conv_ring(void);

void y355_launch_conv1(const Conv1Params &p, hipStream_t s);
void y355_conv1_tiles(int H, int W, int *tx, int *ty);
void y355_pack_conv1(const int8_t *q_w /*[16][3][3][3]*/, int8_t *dst /*1024*/);


// One prediction map of the detection head.  Channel layout [A obj | A*C cls | A*4 txtytwth],
// anchor-major (models/slim_yolo_v2.py:330-341, models/tiny_yolo_v3.py:202-222).
struct HeadLevel {
    const int8_t *pred;   // [B][Hs][Ws][cstride] int8 (value = q * dq) ...
    const float *pred_f;  // ... or fp32 (bf16 nets; pred == nullptr)
    int cstride;
    int Hs, Ws;
    float stride;         // cx = (sigmoid(tx) + gx) * stride
    float dq;             // 2^-sa_pred
    float anchors[32];    // (w, h) of this level's A anchors
};
struct HeadParams {
    HeadLevel lev[3];     // anchor index n: level 0 first, n = cell * A + a inside a level
    int nlev;
    int A, C;             // anchors per level, classes
    float wh_mul;         // w = exp(tw) * aw * wh_mul   (16: anchors in grid units; 1: pixels)
    int Hb, Wb;           // bin grid of the candidate sort
    int group_by_area;    // 0: candidates grouped by anchor type (bins = level 0's grid); 1: by area octave (<= 16 x 16 bins)
    int pairs_wgs;        // workgroups per image of the NMS pair walk: 0 = default (2); 1 while several handles share the GPU
    int cls_groups;       // set by y355_launch_head_nms: 1 = the groups are the CLASSES (per-class NMS never pairs two classes), else 0
    float in_w, in_h;     // network input size in pixels
    float conf_thresh, nms_thresh;
    float *cand_box;      // [B][N][4]
    float *cand_score;    // [B][N]
    int *cand_cls;        // [B][N]
    int max_det;
    float *out_box;
    float *out_score;
    int *out_cls;
    int *out_count;
};
#define Y355_NMS_CAP 4096   // anchors per image the NMS workspace is sized for
#define Y355_HEAD_EDGE_CAP 28672   // suppressing pairs per image the NMS edge list holds (more: the sorted fallback walk)
#define Y355_HEAD_MAXA 16
#define Y355_HEAD_MAXG 32   // candidate groups of the NMS sort: anchor types, area octaves, or -- heads with 3 .. 32 classes -- the classes
#define Y355_NMS_MAX_CAP (16 * Y355_NMS_CAP)   // most anchors / candidates per image of any head: a rank fits 16 bits
#define Y355_NMS_MAX_CLASSES 256              // the large route sorts on 8 bits of the class (every head has A * (5 + C) <= 256)
// the loud failure of a forward in which more anchors of an image passed conf_thresh than the candidate capacity holds
inline std::string y355_head_overflow_message(int cap) {
    return "more than " + std::to_string(cap) + " anchors of an image pass conf_thresh: raise the threshold" +
           (cap < Y355_NMS_MAX_CAP ? std::string(cap > Y355_NMS_CAP ? " or the candidate capacity" : "") : std::string());
}
void y355_launch_absmax(const float *x, size_t n, unsigned int *out_bits, hipStream_t s);
// uint8 HWC BGR frames -> fp32 NCHW RGB, BaseTransform arithmetic (data/__init__.py:30-56, test.py:79)
void y355_launch_normalize_u8(const uint8_t *frames, float *x, int B, int H, int W, const float *mean_rgb, const float *std_rgb,
                              hipStream_t s);

// BaseTransform of one byte (data/__init__.py:43-45): ((u / 255) - mean) / std with the reference's fp32 operations in the
// reference's order.  Every uint8 input route builds its per-channel 256-entry table from this one expression.
__device__ __forceinline__ float y355_norm_u8(int u, float mean, float sd) {
    float t = (float)u;
    t /= 255.0f;
    t -= mean;
    t /= sd;
    return t;
}

// ---- cv2.resize(image, (W, H)) of BaseTransform (data/__init__.py:36) for uint8 HWC frames (resize.hip)
// coefficient tables of both axes, tab = [xofs dw | xa 2 dw | yofs dh | yb 2 dh] (3 (dh + dw) ints), computed on the host
void y355_resize_tables(int sh, int sw, int dh, int dw, int *tab);
// frames [B][sh][sw][3] -> [B][dh][dw][3], tab on the device
void y355_launch_resize_u8(const uint8_t *src, uint8_t *dst, const int *tab, int B, int sh, int sw, int dh, int dw, hipStream_t s);
// one output pixel (dy, dx) of that resize, three bytes in the frame's channel order: OpenCV's 8-bit fixed-point bilinear
// (imgproc/resize.cpp: 11-bit coefficients, horizontal pass in int32, vertical pass
// (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2), the two row indices clipped to the frame.
// s = the frame's first byte
__device__ __forceinline__ void y355_resize_px(const uint8_t *s, const int *tab, int sh, int sw, int dh, int dw, int dy, int dx,
                                               int out[3]) {
    const int *xofs = tab, *xa = tab + dw, *yofs = tab + 3 * dw, *yb = tab + 3 * dw + dh;
    const int sx0 = xofs[dx], sx1 = min(sx0 + 1, sw - 1), a0 = xa[2 * dx], a1 = xa[2 * dx + 1];
    const int sy0 = min(max(yofs[dy], 0), sh - 1), sy1 = min(max(yofs[dy] + 1, 0), sh - 1), b0 = yb[2 * dy], b1 = yb[2 * dy + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int d0 = (int)s[((size_t)sy0 * sw + sx0) * 3 + c] * a0 + (int)s[((size_t)sy0 * sw + sx1) * 3 + c] * a1;
        const int d1 = (int)s[((size_t)sy1 * sw + sx0) * 3 + c] * a0 + (int)s[((size_t)sy1 * sw + sx1) * 3 + c] * a1;
        const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
        out[c] = min(max(v, 0), 255);
    }
}
// a list of n frames (y355_frame of include/yolo355.h: own pointer, size and row pitch each, any alignment) -> dst [n][dh][dw][3]
// (dst 4-byte aligned: whole dwords are stored; otherwise bytes), the same arithmetic with the taps addressed through the
// pitch.  tabs [n][3 (dh + dw)] on the device: every frame's tables, built by a kernel of this launch (bit-identical to
// y355_resize_tables).  The descriptors travel by value as kernel arguments, 64 frames per launch: `frames` is read here only
struct y355_frame;
void y355_launch_resize_frames(const y355_frame *frames, int n, uint8_t *dst, int *tabs, int dh, int dw, hipStream_t s);

// ---- the uint8 frame stage's host state, one per handle (y355_engine, y355_net; resize.hip): BaseTransform's constants and
// the buffers of the two resize routes, each allocated when its route first needs it
struct NormU8 { float mean[3], sd[3]; };        // BaseTransform constants per RGB channel (data/__init__.py:50 lists them in BGR order)
struct FrameStage {
    NormU8 norm{{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};
    int H = 0, W = 0, max_batch = 0;            // the network size every frame is resized to
    int *tab = nullptr;             // same-size frames: [xofs W | xa 2W | yofs H | yb 2H] for sources of src_h x src_w (0: none yet)
    int src_h = 0, src_w = 0;
    uint8_t *frames = nullptr;      // [max_batch][H][W][3]: the frames at the network size, where a forward reads them from here
    int *tabs = nullptr;            // frame lists: [max_batch][3 (H + W)], one set of tables per frame, built on the device; the
                                    // list route never touches tab / src_h / src_w
    DevOwner own;
};
void y355_stage_init(FrameStage &st, int H, int W, int max_batch, const DevMem &mem);
void y355_stage_destroy(FrameStage &st);
// mean / std in the reference's BGR order; a non-positive std fails (Y355_EINVAL) and leaves every channel as it was
int y355_stage_set_normalization(FrameStage &st, const float *mean_bgr, const float *std_bgr);
// st.tab holds the tables for same-size frames of src_h x src_w: rebuilt and uploaded (behind what s has in flight) only when
// the size differs from the cached one; a failed upload forgets the cached size
int y355_stage_tables_for(FrameStage &st, int src_h, int src_w, hipStream_t s);
int y355_stage_need_frames(FrameStage &st);     // st.frames
int y355_stage_need_list(FrameStage &st);       // st.tabs
// the rules of a frame list (y355_frame of include/yolo355.h), in this order: the array, the batch, then per frame its pointer,
// its size (1 .. 16384 each way) and its row pitch
int y355_frames_check(const y355_frame *frames, int batch, int max_batch);

// ---- element-wise ops of the y355_net graphs (netops.hip): bf selects the bf16 form, else int8
struct NetMap { char *dev; int H, W, pb; };     // NHWC tensor with a one-pixel halo, [B][H + 2][W + 2][pb bytes]
void y355_launch_pool(bool bf, const NetMap &in, const NetMap &out, int B, int cbytes, int stride, hipStream_t s);      // 2x2 max, first cbytes of a pixel
// bilinear x2 (align_corners) of C channels into byte out_off of out's pixels; int8: times rescale, and only where y355_upsample_i8_ok
void y355_launch_upsample(bool bf, const NetMap &in, const NetMap &out, int B, int C, int out_off, float rescale, hipStream_t s);
bool y355_upsample_i8_ok(const NetMap &in, const NetMap &out, int B, int C, int out_off);
// reorg(stride) of C channels into byte out_off of out's pixels; int8: rescaled by 2^d, clamps counted into ctr
void y355_launch_reorg(bool bf, const NetMap &in, const NetMap &out, int B, int C, int out_off, int stride, int d, Counters *ctr,
                       hipStream_t s);
void y355_launch_spp(bool bf, const NetMap &t, int B, int C, hipStream_t s);          // in place: [x | pool5 | pool9 | pool13], C channels each
// network input: fp32 NCHW x, or (u8 != null) uint8 HWC BGR frames [B][sh][sw][3], resized in the load when tab != null; int8:
// q = clamp(RNE(v * in_scale)), clamps counted into ctr
void y355_launch_input(bool bf, const float *x, const uint8_t *u8, const int *tab, int sh, int sw, const NormU8 &nm, const NetMap &out,
                       int B, float in_scale, Counters *ctr, hipStream_t s);
// maxima, atomicMax into *out (bits of a non-negative fp32, or an unsigned int for absmax_i8): all n_elems bf16 values of a
// buffer; |blend| of the int8 bilinear x2 before its rescale; |q| of the first C channels; the normalised frames as the input reads them
void y355_launch_absmax_bf16(const char *t, size_t n_elems, unsigned int *out_bits, hipStream_t s);
void y355_launch_upsample_i8_max(const NetMap &in, int B, int C, unsigned int *out_bits, hipStream_t s);
void y355_launch_absmax_i8(const NetMap &in, int B, int C, unsigned int *out, hipStream_t s);
void y355_launch_absmax_u8(const uint8_t *frames, const int *tab, int B, int sh, int sw, int H, int W, const NormU8 &nm,
                           unsigned int *out_bits, hipStream_t s);
// the evaluators' `bboxes *= [[w, h, w, h]]` of every image, in place (engine.hip); wh [B][2]
void y355_launch_scale_boxes(float *boxes, const int32_t *count, const float *wh, int batch, int max_det, hipStream_t s);

// ---- generic chunked conv (convg.hip): bf16 nets and the int8 layers conv3x3.hip cannot hold (RequantG, ResQ: y355_requant.h) --
struct ConvGParams {
    const char *in;           // NHWC with halo, in_pb bytes per pixel
    char *out;                // NHWC, out_pb bytes per pixel
    const char *w;            // fragment-packed weights (y355_convg_pack)
    const float *bias_f;      // bf16: [cout_pad]
    const long long *bias_w;  // int8: [cout_pad] pre-shifted; rq.narrow: y355_pc_word(shl[c], bias[c])
    Counters *ctr;            // int8: saturation counter (or null)
    int B, H, W;
    int in_pb, nchunks;       // bytes per input pixel; chunks of CHB bytes consumed
    int out_pb, out_off;      // bytes per output pixel of the buffer; byte offset of this conv's channel 0
    int out_halo, tiles_x, tiles_y, nblk;
    int taps;                 // 9 (3x3, pad 1) or 1 (1x1)
    float slope;              // bf16: y = x >= 0 ? x : slope * x
    int out_f32;              // bf16: store fp32 (prediction layers)
    RequantG rq;
    // residual added after the activation (backbone/darknet.py:36 `module(x) + x`), same layout as `out` (halo, pixel
    // pitch res_pb, byte offset res_off of channel 0); null = none.  bf16: added in fp32; int8: ResQ rr below
    const char *res;
    int res_pb, res_off;
    int grid_limit;           // host side only: persistent workgroups of a convr.hip launch (0 = one per CU), Y355_NET_OPT_WORKGROUPS
    int xcd_share_log2;       // convr.hip: work items that read one input are walked by workgroups of one XCD (set by the launcher)
    ResQ rr;                  // int8 with `res`: the residual's exponent shifts
    // per-channel weight exponents (appended: the fields above keep their kernel-argument offsets)
    const int *shl_w;         // int8, 64-bit epilogue (!rq.narrow): [cout_pad] accumulator shift of every output channel
    int pc;                   // int8: 1 = the shifts differ between channels (convg.hip and pw_i8_kernel take their per-lane-shift instantiation)
};

struct Conv1FParams {
    const float *x;       // fp32 NCHW [B][3][H][W]
    const uint8_t *x_u8;  // or (x == nullptr) camera frames uint8 HWC BGR [B][H][W][3], normalised on the fly
    float nmean[3], nstd[3];  // BaseTransform constants per RGB channel (data/__init__.py:50)
    char *out;            // bf16 NHWC16 with halo [B][H/2+2][W/2+2][16]
    const char *w;        // two 1 KiB fragments
    const float *bias;    // [16]
    int B, H, W, tiles_x, tiles_y;
    float slope;
};

struct ConvGInfo {
    int bf, chb, bn, th, tw, pool, wm, wn, nt;
    int stride;               // 1, or 2 (3x3 / pad 1 / stride 2: backbone/darknet.py:124-141)
    size_t lds_bytes;
    void (*launch)(const ConvGParams &p, int nblocks, hipStream_t s);
    int (*prepare)(void);
    // int8: statistics mode -- max |t'| (residual layers: |u|) over the un-pooled outputs into p.ctr->absmax, nothing stored;
    // p.bias_w plain 64-bit biases, p.shl_w when p.pc (y355_net_calibrate)
    void (*launch_stat)(const ConvGParams &p, int nblocks, hipStream_t s);
};
#define Y355_G_COUNT 11
const ConvGInfo *y355_convg_kernel(int bf, int id);
int y355_prepare_convg(void);
int y355_convg_select(int in_pb, int cout, int pool, int H, int W, int stride = 1, int batch_hint = 0);
int y355_convg_ksteps(const ConvGInfo &ki, int in_pb, int taps);
size_t y355_convg_packed_bytes(const ConvGInfo &ki, int in_pb, int taps, int cout_pad);
void y355_convg_pack(const ConvGInfo &ki, const float *w_f, const int8_t *w_q, int cout, int cin, int ksize,
                     int in_pb, int cout_pad, char *dst);
// thin 3x3 layers of the bf16 nets with the weights in registers (convpxb.hip): id from select (-1: none), weights fp32 [cout][cin][3][3]
int y355_prepare_convpxb(void);
int y355_convpxb_select(int in_pb, int cout, int pool);
size_t y355_convpxb_packed_bytes(int id);
bool y355_convpxb_pack(int id, const float *w, int cout, int cin, char *dst);
bool y355_launch_convpxb(int id, const ConvGParams &p, hipStream_t s);      // false: not available for this launch
// 3x3 layers of the generic nets on the LDS-DMA ring discipline (convr.hip); weights in y355_convg_pack order for (bn, wn, nt) below
struct Y355ConvRInfo { int bf, cinb, bn, th, tw, pool, wn, nt; };
int y355_prepare_convr(int device);
const Y355ConvRInfo *y355_convr_info(int rid);
int y355_convr_select(int bf, int in_pb, int cout_pad, int pool, int H, int W);
bool y355_launch_convr(int rid, const ConvGParams &p, int device, hipStream_t s);
bool y355_launch_pw_i8(const ConvGParams &p, hipStream_t s);        // 1x1, int8, 32-bit epilogue; weights packed for (bn 64, wn 1, nt 4)
void y355_conv1f_tiles(int H, int W, int *tx, int *ty);
void y355_launch_conv1f(const Conv1FParams &p, hipStream_t s);
void y355_pack_conv1f(const float *w, char *dst);
// General-geometry implicit-GEMM convolution (convgeom.hip): any kernel size, stride, dilation and four pads.
// GEMM rows = output pixels of the whole batch (m = (b * Ho + oy) * Wo + ox), columns = output channels, K = taps x 64-byte
// chunks of one input pixel.  Input NHWC with a one-pixel halo (the staging kernels of ops.hip), in_pb bytes per pixel;
// taps that fall in the padding are zero by a predicate, never by a read.
struct ConvGeomParams {
    const char *in;           // [B][H + 2][W + 2][in_pb]
    const char *w;            // y355_convgeom_pack order
    const float *bias_f;      // bf16: [cout_pad]
    const long long *bias_w;  // int8: [cout_pad] pre-shifted (q_b << (F - e_b))
    const char *res;          // bf16: residual, same layout as out (or null)
    char *out;                // bf16: [B][Ho + 2][Wo + 2][out_pb] (bf16 or fp32 channels)
    long long *raw;           // int8: t' [M][cout_pad]
    int B, H, W, Ho, Wo, M;
    int in_pb, nchunk;        // bytes per input pixel (multiple of 64), 64-byte chunks per pixel
    int kh, kw, sh, sw, dh, dw, pt, pl;
    int nblk, cout_pad, out_pb, out_f32;
    float slope;              // bf16: y = x >= 0 ? x : slope * x
    int shl, lk, neg_mul;     // int8: t = acc * 2^shl + bias; t' = t >= 0 ? t * 2^lk : t * neg_mul
};
struct ConvGeomInfo { int bm, bn, wm, wn, mt, nt; size_t lds_bytes; };
#define Y355_GEOM_COUNT 3
const ConvGeomInfo *y355_convgeom_info(int id);
int y355_convgeom_select(int M, int cout, int cu);
int y355_prepare_convgeom(void);
size_t y355_convgeom_packed_bytes(int id, int in_pb, int taps, int cout_pad);
void y355_convgeom_pack(int id, int bf, const float *w_f, const int8_t *w_q, int cout, int cin, int taps, int in_pb, int cout_pad,
                        char *dst);
void y355_launch_convgeom(int id, int bf, const ConvGeomParams &p, hipStream_t s);
