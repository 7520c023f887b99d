// yolo355_qtrain -- one quantisation-aware fine-tuning step of the BN-folded SlimYOLOv2 on the GPU (gfx950): the forward of the
// deployed int8 network as a fake quantisation in fp32, bit for bit, the straight-through backward and the SGD step of
// train.hip with the weights and biases quantised again after it; C ABI in include/yolo355_qtrain.h, linked into
// libyolo355_qtrain.so on its own.  The arithmetic contract is DESIGN.md section 6o.
//
// The kernels.  train_core.h's convolution with the epilogues M_QFWD, M_QFWD_POOL, M_QPRED (quantise at the output's tracker,
// the state byte S_k, the tracker's max|v| and clipped count) and M_QDGRAD, M_QDGRAD_UNPOOL (slope and clip mask from S_{k-1});
// its weight-gradient, reduce and SGD kernels unchanged, on the quantised operands.  Here:
//   qtrain_input_kernel    A_0 = fq(x): NCHW fp32 -> NHWC bf16, 3 channels padded to 8, tracker 0's statistics
//   qtrain_dpred_kernel    G_10 = rb(dP * [not clipped]): NCHW fp32 -> NHWC bf16 through S_10, channels padded with zeros
//   qtrain_range_kernel    max|W_k| and max|b_k| of the twenty tensors, as the bits of a non-negative float through atomicMax
//   qtrain_requant_kernel  e = the exponent field of fl32(127 / m); Wq_k into the forward pack and the data-gradient pack, bq_k,
//                          the exponents themselves
// Integer atomics alone (maxima and counts, exact in any order): the same bits from run to run.
//
// The handle's common state, the create rules, the common device memory and the bodies of the entry points yolo355_train.h has
// too are train_host.h's; this file owns the quantiser's kernels, state, memory and entry points and the two passes' loops.
#include "../../include/yolo355_qtrain.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
#include <cmath>
static_assert(Y355_QTRAIN_OK == Y355_OK && Y355_QTRAIN_EINVAL == Y355_EINVAL && Y355_QTRAIN_EHIP == Y355_EHIP && Y355_QTRAIN_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_qtrain_last_error's text
#ifndef Y355_HOSTCHECK                                   // (qtrain_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

#define TRAIN_FAMILY "y355_qtrain"
#include "train_core.h"
#include "train_host.h"
static_assert(NL == Y355_QTRAIN_LAYERS, "train_core.h's layer table");
static_assert(Y355_QTRAIN_ACT == T_ACT && Y355_QTRAIN_IDX == T_IDX && Y355_QTRAIN_GRAD == T_GRAD, "train_host.h's tensor kinds");
static_assert(Y355_QTRAIN_S_POS == Q_POS && Y355_QTRAIN_S_NEG == Q_NEG && Y355_QTRAIN_S_CLIP == Q_CLIP, "train_core.h's state byte");
constexpr int NT = Y355_QTRAIN_TRACKERS;

// floor(log2(fl32(127 / m))) of a tensor's m = max|T|, exactly: the exponent field of the quotient.  m = 0 (and a NaN): 0;
// a quotient that overflows (m below 2^-121, the denormals among them): 127.  The quotient is never denormal (m <= FLT_MAX
// gives 127 / m >= 2^-122).
__host__ __device__ inline int qtrain_exponent(float m) {
    if (!(m > 0.f)) return 0;
    const float s = 127.0f / m;
    const int f = (int)((__builtin_bit_cast(unsigned int, s) >> 23) & 0xff);
    return f == 0xff ? 127 : f - 127;
}

// ---------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void qtrain_input_kernel(const float *__restrict__ x, bf16_t *__restrict__ a0, size_t npix, size_t hw, float qs, float qi,
                                                           unsigned int *__restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned int vmax = 0, nclip = 0;
    if (p < npix) {
        const size_t b = p / hw, yx = p - b * hw;
        const float *s = x + b * 3 * hw + yx;
        bf16_t h[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = s[c * hw];
            vmax = max(vmax, __builtin_bit_cast(unsigned int, fabsf(v)));
            bool clipped;
            h[c] = rb_(quant_(v, qs, clipped) * qi);
            nclip += clipped ? 1u : 0u;
        }
        uint4 u;
        u.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
        u.y = (unsigned)h[2];
        u.z = 0;
        u.w = 0;
        *(uint4 *)(a0 + p * 8) = u;
    }
    wave_stats_(vmax, nclip, stats);
}

__global__ __launch_bounds__(256) void qtrain_dpred_kernel(const float *__restrict__ dp, const unsigned char *__restrict__ s10, bf16_t *__restrict__ g,
                                                           size_t n, int cout, int coutp_log2, size_t hw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t p = i >> coutp_log2;
    const int c = (int)(i & (((size_t)1 << coutp_log2) - 1));
    const size_t b = p / hw, yx = p - b * hw;
    g[i] = (c < cout && !(s10[i] & Q_CLIP)) ? rb_(dp[(b * cout + c) * hw + yx]) : (bf16_t)0;
}

// tensor 2 k + (bias) of parameter i, k = 0..9
__device__ __forceinline__ int tensor_of_(const NetDesc &d, size_t i, int &k) {
    k = 0;
    while (k < NL - 1 && i >= d.L[k + 1].woff) ++k;
    return 2 * k + (i >= d.L[k].boff ? 1 : 0);
}

__global__ __launch_bounds__(256) void qtrain_range_kernel(const NetDesc d, const float *__restrict__ p, unsigned int *__restrict__ range) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int k, id = -1;
    unsigned int bits = 0;
    if (i < d.total) {
        id = tensor_of_(d, i, k);
        bits = __builtin_bit_cast(unsigned int, fabsf(p[i]));
    }
    if (__all(id == __shfl(id, 0))) {                         // the wave lies inside one tensor (or past the end): one atomic
        if (id < 0) return;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) bits = max(bits, (unsigned int)__shfl_xor((int)bits, m));
        if ((threadIdx.x & 63) == 0 && bits > __hip_atomic_load(range + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(range + id, bits);
    } else if (id >= 0) {                                     // (a maximum already reached needs no atomic, as in wave_stats_)
        atomicMax(range + id, bits);
    }
}

struct QuantDesc {
    size_t qb[NL];                   // of bq_k in the bias array
};

__global__ __launch_bounds__(256) void qtrain_requant_kernel(const NetDesc d, const QuantDesc qd, const float *__restrict__ p,
                                                             const unsigned int *__restrict__ range, bf16_t *__restrict__ packs, float *__restrict__ bq,
                                                             int *__restrict__ wexp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d.total) return;
    int k;
    const int id = tensor_of_(d, i, k);
    const LayerDesc &L = d.L[k];
    const int e = qtrain_exponent(__builtin_bit_cast(float, range[id]));
    const float r = rintf(ldexpf(p[i], e));
    const float v = ldexpf(fminf(fmaxf(r, -127.f), 127.f) + 0.0f, -e);         // (+ 0: the integer 0 has no sign)
    if (i == L.woff || i == L.boff) wexp[id] = e;
    if (i >= L.boff) {
        bq[qd.qb[k] + (i - L.boff)] = v;
        return;
    }
    const size_t el = i - L.woff;
    const int co = (int)(el / ((size_t)L.cin * 9)), rem = (int)(el - (size_t)co * L.cin * 9), ci = rem / 9, tap = rem % 9;
    const bf16_t h = rb_(v);                                  // exact: seven bits and a sign
    packs[L.wf_off + pack_index(co, L.ksf, tap * L.cinp + ci)] = h;
    if (k > 0) packs[L.wd_off + pack_index(ci, L.ksd, (8 - tap) * L.coutp + co)] = h;       // rotated by 180 degrees, (co, ci) transposed
}

// ---------------------------------------------------------------------------------------------------------- the handle
struct QDev {                        // the quantiser's device memory, the owner's too: qtrain_buffers resets it in one assignment
    float *bq = nullptr;             // bq_1 .. bq_10
    unsigned int *wrange = nullptr;  // [20] bits of max|W_k|, max|b_k|
    int *wexp = nullptr;             // [20] (e_w, e_b)
    unsigned int *stats = nullptr;   // [11][2] bits of max|v|, clipped count
    unsigned char *state[NL + 1] = {};       // S_1 .. S_10 (index k); a pooled layer's is idx[k]
};
struct y355_qtrain : TrainCore, QDev {
    int e_a[NT] = {};
    bool have_exp = false;
    QuantDesc qd{};
    size_t qb_total = 0;
};

// The seams of qtrain_host_check.cpp, which does not see the struct.  y355_qtrain_create in two parts: train_host.h's rules and
// host state with the offsets of the quantised biases on top, ...
int qtrain_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_qtrain **out) {
    if (int rc = core_open(max_h, max_w, num_classes, num_anchors, max_batch, mem, out)) return rc;
    y355_qtrain *h = *out;
    for (int k = 0; k < NL; ++k) {
        h->qd.qb[k] = h->qb_total;
        h->qb_total += h->d.L[k].cout;
    }
    return Y355_QTRAIN_OK;
}
// ... and all of its device memory (on the current device) or none of it: the quantiser's arrays follow the parameters, S_k of a
// layer without a pool follows G_k (a pooled layer's is I_k)
int qtrain_buffers(y355_qtrain *h) {
    DevOwner &o = h->own;
    const int rc = core_buffers(
        h,
        [&] {
            int r = y355_dev_get(o, &h->bq, h->qb_total, true);
            r = r ? r : y355_dev_get(o, &h->wrange, 2 * NL, true);
            r = r ? r : y355_dev_get(o, &h->wexp, 2 * NL, true);
            return r ? r : y355_dev_get(o, &h->stats, 2 * NT, true);
        },
        [&](int k, size_t n) { return kPool[k - 1] ? 0 : y355_dev_get(o, &h->state[k], n, true); });
    if (rc) {
        static_cast<QDev &>(*h) = QDev{};
        return rc;
    }
    for (int k = 1; k <= NL; ++k)
        if (kPool[k - 1]) h->state[k] = h->idx[k];
    return rc;
}
DevOwner &qtrain_owner(y355_qtrain *h) { return h->own; }
void qtrain_free(y355_qtrain *h) { core_free(h); }
void qtrain_state(const y355_qtrain *h, int *hw_batch) {     // core_state's four, then whether the exponents are set
    core_state(h, hw_batch);
    hw_batch[4] = h->have_exp ? 1 : 0;
}
int qtrain_exponent_host(float m) { return qtrain_exponent(m); }

// S_t, t = 1..10: the tensor kind yolo355_train.h does not have, on A_t's grid (P's for t = 10), one byte an element
static OwnTensor q_tensor(const TrainCore *hc, int kind, int t) {
    const y355_qtrain *h = static_cast<const y355_qtrain *>(hc);
    if (kind != Y355_QTRAIN_STATE || t < 1 || t > NL) return OwnTensor{nullptr, 0, false};
    return OwnTensor{h->state[t], h->d.L[t - 1].coutp, false, 1, t == NL ? kDiv[NL - 1] : act_div(t)};
}

// every tensor's range, then its exponent, its quantised values in the packs and the bias array
static hipError_t launch_requant(y355_qtrain *h, hipStream_t s) {
    if (const hipError_t e = hipMemsetAsync(h->wrange, 0, 2 * NL * sizeof(unsigned int), s)) return e;
    const dim3 grid((unsigned)((h->d.total + 255) / 256)), block(256);
    hipLaunchKernelGGL(qtrain_range_kernel, grid, block, 0, s, h->d, h->p, h->wrange);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(qtrain_requant_kernel, grid, block, 0, s, h->d, h->qd, h->p, h->wrange, h->packs, h->bq, h->wexp);
    return hipGetLastError();
}

// the arguments of layer k's forward convolution with the quantiser's on top
static ConvArgs q_forward_args(const y355_qtrain *h, int k, int batch, void *out) {
    ConvArgs a = forward_conv_args(h, k, batch, out, nullptr);
    a.bias = h->bq + h->qd.qb[k - 1];
    a.qs = std::ldexp(1.0f, h->e_a[k]);
    a.qi = std::ldexp(1.0f, -h->e_a[k]);
    a.state = h->state[k];
    a.stats = h->stats + 2 * k;
    return a;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_qtrain_last_error(void) { return g_err.c_str(); }

// what yolo355_train.h has too: train_host.h's bodies
int y355_qtrain_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_qtrain **out) {
    return core_create(max_h, max_w, num_classes, num_anchors, max_batch, out, qtrain_open, qtrain_buffers);
}
void y355_qtrain_destroy(y355_qtrain *h) { core_destroy(h); }
int y355_qtrain_set_size(y355_qtrain *h, int32_t height, int32_t width) { return core_set_size(h, height, width); }
int y355_qtrain_layer_shape(const y355_qtrain *h, int32_t k, int32_t *shape) { return core_layer_shape(h, k, shape); }
int y355_qtrain_get_layer(y355_qtrain *h, int32_t k, float *w, float *b) { return core_get_layer(h, k, w, b); }
int y355_qtrain_get_grad(y355_qtrain *h, int32_t k, float *dw, float *db) { return core_get_grad(h, k, dw, db); }
int y355_qtrain_get_momentum(y355_qtrain *h, int32_t k, float *mw, float *mb) { return core_get_momentum(h, k, mw, mb); }
int y355_qtrain_get_packed(y355_qtrain *h, int32_t k, uint16_t *w_bf16) { return core_get_packed(h, k, w_bf16); }
int y355_qtrain_pred(y355_qtrain *h, void **out) { return core_pred(h, out); }
int y355_qtrain_wgrad_plan(const y355_qtrain *h, int32_t k, int32_t batch, int32_t *out) { return core_wgrad_plan(h, k, batch, out); }
int y355_qtrain_tensor_shape(const y355_qtrain *h, int32_t kind, int32_t t, int32_t *shape) { return core_tensor_shape(h, kind, t, shape, q_tensor); }
int y355_qtrain_get_tensor(y355_qtrain *h, int32_t kind, int32_t t, void *out) { return core_get_tensor(h, kind, t, out, q_tensor); }

int y355_qtrain_load_layer(y355_qtrain *h, int32_t k, const float *w, const float *b) {
    if (int rc = core_load_layer(h, k, w, b)) return rc;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_requant(h, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return Y355_QTRAIN_OK;
}

int y355_qtrain_sgd_step(y355_qtrain *h, float lr, float momentum, float weight_decay, void *stream) {
    return core_sgd_step(h, lr, momentum, weight_decay, stream, [=](int) { return launch_requant(h, (hipStream_t)stream); });
}

int y355_qtrain_set_act_exponents(y355_qtrain *h, const int32_t *e_a) {
    if (!h || !e_a) return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_set_act_exponents: null argument");
    for (int t = 0; t < NT; ++t)
        if (e_a[t] < -Y355_QTRAIN_MAX_ACT_EXPONENT || e_a[t] > Y355_QTRAIN_MAX_ACT_EXPONENT)
            return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_set_act_exponents: an exponent beyond +-96");
    for (int t = 0; t < NT; ++t) h->e_a[t] = e_a[t];
    h->have_exp = true;
    return Y355_QTRAIN_OK;
}

int y355_qtrain_get_act_exponents(const y355_qtrain *h, int32_t *e_a) {
    if (!h || !e_a) return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_get_act_exponents: null argument");
    if (!h->have_exp) return y355_fail(Y355_QTRAIN_ENOTREADY, "y355_qtrain_get_act_exponents: the activation exponents are not set");
    for (int t = 0; t < NT; ++t) e_a[t] = h->e_a[t];
    return Y355_QTRAIN_OK;
}

int y355_qtrain_get_act_stats(y355_qtrain *h, float *max_abs, int64_t *clipped) {
    if (!h) return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_get_act_stats: null handle");
    if (h->batch == 0) return y355_fail(Y355_QTRAIN_ENOTREADY, "y355_qtrain_get_act_stats: no forward pass has run at this size");
    unsigned int st[2 * NT];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(st, h->stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int t = 0; t < NT; ++t) {
        if (max_abs) max_abs[t] = __builtin_bit_cast(float, st[2 * t]);
        if (clipped) clipped[t] = (int64_t)st[2 * t + 1];
    }
    return Y355_QTRAIN_OK;
}

int y355_qtrain_get_weight_exponents(y355_qtrain *h, int32_t *out) {
    if (!h || !out) return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_get_weight_exponents: null argument");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, h->wexp, 2 * NL * sizeof(int32_t), hipMemcpyDeviceToHost));
    return Y355_QTRAIN_OK;
}

int y355_qtrain_get_qbias(y355_qtrain *h, int32_t k, float *bq) {
    if (int rc = layer_arg("y355_qtrain_get_qbias", h, k)) return rc;
    if (!bq) return y355_fail(Y355_QTRAIN_EINVAL, "y355_qtrain_get_qbias: null argument");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(bq, h->bq + h->qd.qb[k - 1], (size_t)h->d.L[k - 1].cout * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_QTRAIN_OK;
}

int y355_qtrain_forward(y355_qtrain *h, const void *x_dev, int32_t batch, void *stream) {
    if (int rc = forward_args(h, x_dev, batch)) return rc;
    if (!h->have_exp) return y355_fail(Y355_QTRAIN_ENOTREADY, "y355_qtrain_forward: the activation exponents are not set");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->batch = 0;                                             // no finished forward until the end
    h->have_grad = false;
    HIPCHK(hipMemsetAsync(h->stats, 0, 2 * NT * sizeof(unsigned int), s));
    const size_t npix = (size_t)batch * h->H * h->W;
    hipLaunchKernelGGL(qtrain_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const float *)x_dev, h->act[0], npix,
                       (size_t)h->H * h->W, std::ldexp(1.0f, h->e_a[0]), std::ldexp(1.0f, -h->e_a[0]), h->stats);
    HIPCHK(hipGetLastError());
    for (int k = 1; k < NL; ++k) {
        const LayerDesc &L = h->d.L[k - 1];
        const ConvArgs a = q_forward_args(h, k, batch, h->act[k]);
        HIPCHK(kPool[k - 1] ? launch_conv<M_QFWD_POOL>(a, L.ct, (L.cout + 15) / 16, s) : launch_conv<M_QFWD>(a, L.ct, (L.cout + 15) / 16, s));
    }
    const LayerDesc &L = h->d.L[NL - 1];
    ConvArgs a = q_forward_args(h, NL, batch, h->pred);
    a.outc = L.coutp;                                         // of S_10
    HIPCHK(launch_conv<M_QPRED>(a, L.ct, (L.cout + 15) / 16, s));
    h->batch = batch;
    return Y355_QTRAIN_OK;
}

int y355_qtrain_backward(y355_qtrain *h, const void *dpred_dev, void *stream) {
    if (int rc = backward_args(h, dpred_dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->have_grad = false;
    {
        const LayerDesc &L = h->d.L[NL - 1];
        const size_t hw = (size_t)(h->H / 16) * (h->W / 16), n = (size_t)h->batch * hw * L.coutp;
        hipLaunchKernelGGL(qtrain_dpred_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)dpred_dev, h->state[NL], h->grad[NL], n,
                           L.cout, ilog2_(L.coutp), hw);
        HIPCHK(hipGetLastError());
    }
    for (int k = NL; k >= 1; --k) {
        HIPCHK(launch_wgrad(h, k, s));
        if (k == 1) break;                                    // the gradient with respect to the image is not computed
        const LayerDesc &L = h->d.L[k - 1];
        ConvArgs a = dgrad_conv_args(h, k, h->grad[k - 1]);
        a.state_prev = h->state[k - 1];
        HIPCHK(kPool[k - 2] ? launch_conv<M_QDGRAD_UNPOOL>(a, L.dct, L.cin / 16, s) : launch_conv<M_QDGRAD>(a, L.dct, L.cin / 16, s));
    }
    h->have_grad = true;
    return Y355_QTRAIN_OK;
}

}  // extern "C"
