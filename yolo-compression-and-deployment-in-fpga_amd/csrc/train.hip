// yolo355_train -- one fine-tuning step of the BN-folded SlimYOLOv2 on the GPU (gfx950): forward with what the backward
// needs, data and weight gradients of the ten 3x3 convolutions, SGD; C ABI in include/yolo355_train.h, linked into
// libyolo355_train.so on its own (nothing of libyolo355.so is used).  The arithmetic contract is DESIGN.md section 6m.
//
// Layouts.  Activations A_t, pool positions I_t and gradients G_t are NHWC (a pixel's channels are contiguous), so a lane's
// MFMA fragment of eight consecutive input channels of one tap is one 16-byte load.  The GEMM index of a convolution is
// k = tap * cinp + ci (cinp a power of two >= 8), cut into k-steps of 32; weights are packed per (16-row tile, k-step) as
// the 64 x 16 bytes of the A operand (lane (g, i): row i, k = 8 g .. 8 g + 7).
//
// The kernels (train_core.h, which bntrain.hip compiles too):
//   train_input_kernel  A_0 = rb(x): NCHW fp32 -> NHWC bf16, 3 channels padded to 8
//   train_conv_kernel    implicit GEMM, rows = output channels (packed weights), columns = pixels (gathered from NHWC with
//                        zero padding), four column sets per wave: four runs of 16 pixels, or the four positions of 16
//                        pooling windows.  Epilogues: bias + LeakyReLU (+ 2x2 pool with I_k) -> bf16; bias -> fp32 NCHW (P);
//                        data gradient: times the slope mask of A_{k-1}, rb, written through I_{k-1} (all four positions).
//   train_dpred_kernel   G_10 = rb(dP): NCHW fp32 -> NHWC bf16, channels padded with zeros
//   train_wgrad_kernel   dW_k and db_k: rows = output channels of G_k, columns = 16 input channels of A_{k-1} for each of
//                        the nine taps, summed over a run of pixels; one wave per (tile, run), partial sums to a workspace
//   train_reduce_kernel  adds the runs in a fixed order (four interleaved chains, then their sum): no atomics
//   train_sgd_kernel     the update of every parameter and the bf16 packs of the forward and of the data gradient
#include "../../include/yolo355_train.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_TRAIN_OK == Y355_OK && Y355_TRAIN_EINVAL == Y355_EINVAL && Y355_TRAIN_EHIP == Y355_EHIP && Y355_TRAIN_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_train_last_error's text
#ifndef Y355_HOSTCHECK                                   // (train_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

#include "train_core.h"
static_assert(NL == Y355_TRAIN_LAYERS, "train_core.h's layer table");

// ---------------------------------------------------------------------------------------------------------- the handle
struct y355_train {
    DevOwner own;
    int device_id = 0;
    int max_h = 0, max_w = 0, max_batch = 0, num_classes = 0, num_anchors = 0;
    int H = 0, W = 0;
    int batch = 0;                   // of the last forward at this size (0: none)
    bool have_grad = false;          // a backward since the last forward
    long long steps = 0;
    NetDesc d;
    size_t pack_total = 0, ws_total = 0;
    float *p = nullptr, *g = nullptr, *m = nullptr;
    bf16_t *packs = nullptr;
    bf16_t *act[NL] = {};            // A_0 .. A_9
    unsigned char *idx[NL] = {};     // I_t, t = 1, 2, 4, 6 (index t)
    bf16_t *grad[NL + 1] = {};       // G_1 .. G_10 (index k)
    float *pred = nullptr, *ws = nullptr;
};

// channels and grid divisor of A_t
static int act_c(const y355_train *h, int t) { return t == 0 ? 8 : h->d.L[t - 1].cout; }
static int act_div(int t) { return t == 0 ? 1 : kDiv[t - 1] * (kPool[t - 1] ? 2 : 1); }

// y355_train_create in two parts, as train_host_check.cpp runs them on the CPU: the rules and the host state (no device
// call), ...
int train_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_train **out) {
    if (!out) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_create: null argument");
    *out = nullptr;
    if (max_h < 16 || max_w < 16 || max_h % 16 || max_w % 16 || max_h > 4096 || max_w > 4096)
        return y355_fail(Y355_TRAIN_EINVAL, "y355_train_create: max_h and max_w must be multiples of 16 in 16..4096");
    if (num_classes < 1 || num_classes > 200) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_create: num_classes must be 1..200");
    if (num_anchors < 1 || num_anchors > 16) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_create: num_anchors must be 1..16");
    if (max_batch < 1 || max_batch > 1024) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_create: max_batch must be 1..1024");
    y355_train *h = new y355_train;
    h->own = DevOwner{mem, {}};
    h->max_h = h->H = max_h;
    h->max_w = h->W = max_w;
    h->max_batch = max_batch;
    h->num_classes = num_classes;
    h->num_anchors = num_anchors;
    size_t off = 0, poff = 0;
    for (int k = 0; k < NL; ++k) {
        LayerDesc &L = h->d.L[k];
        L.cin = kCin[k];
        L.cinp = k == 0 ? 8 : kCin[k];
        L.cout = k == NL - 1 ? num_anchors * (5 + num_classes) : kCout[k];
        L.coutp = k == NL - 1 ? pow2_at_least(L.cout, 32) : L.cout;
        L.ct = tiles_per_wave(L.cout);
        L.ksf = (9 * L.cinp + 31) / 32;
        L.ksd = 9 * L.coutp / 32;
        L.dct = tiles_per_wave(L.cin);
        L.woff = off;
        off += (size_t)L.cout * L.cin * 9;
        L.boff = off;
        off += L.cout;
        const int tf = ((L.cout + 15) / 16 + L.ct - 1) / L.ct * L.ct;
        L.wf_off = poff;
        poff += (size_t)tf * L.ksf * 512;
        L.wd_off = poff;
        if (k > 0) poff += (size_t)(L.cin / 16) * L.ksd * 512;
        h->ws_total = std::max(h->ws_total, (size_t)wgrad_max_runs(L) * wgrad_stride(L));
    }
    h->d.total = off;
    h->pack_total = poff;
    *out = h;
    return Y355_TRAIN_OK;
}
// ... and all of its device memory (on the current device), or none of it
int train_buffers(y355_train *h) {
    DevOwner &o = h->own;
    const size_t mark = y355_dev_mark(o);
    const size_t B = h->max_batch;
    int rc = y355_dev_get_all<true>(o, h->d.total, &h->p, &h->g, &h->m);
    rc = rc ? rc : y355_dev_get(o, &h->packs, h->pack_total, true);
    rc = rc ? rc : y355_dev_get(o, &h->ws, h->ws_total, true);
    for (int t = 0; t < NL && !rc; ++t) {
        const size_t n = B * (h->max_h / act_div(t)) * (h->max_w / act_div(t)) * act_c(h, t);
        rc = y355_dev_get(o, &h->act[t], n, true);
        if (!rc && t >= 1 && kPool[t - 1]) rc = y355_dev_get(o, &h->idx[t], n, true);
    }
    for (int k = 1; k <= NL && !rc; ++k)
        rc = y355_dev_get(o, &h->grad[k], B * (h->max_h / kDiv[k - 1]) * (h->max_w / kDiv[k - 1]) * h->d.L[k - 1].coutp, true);
    rc = rc ? rc : y355_dev_get(o, &h->pred, B * h->d.L[NL - 1].cout * (h->max_h / 16) * (h->max_w / 16), true);
    if (rc) {
        y355_dev_rollback(o, mark);
        h->p = h->g = h->m = h->ws = h->pred = nullptr;
        h->packs = nullptr;
        for (int t = 0; t < NL; ++t) {
            h->act[t] = nullptr;
            h->idx[t] = nullptr;
            h->grad[t + 1] = nullptr;
        }
    }
    return rc;
}
DevOwner &train_owner(y355_train *h) { return h->own; }      // (train_host_check.cpp does not see the struct)
void train_free(y355_train *h) {
    y355_dev_release_all(h->own);
    delete h;
}
void train_state(const y355_train *h, int *hw_batch) {       // H, W, batch of the last forward, have_grad: for the host check
    hw_batch[0] = h->H;
    hw_batch[1] = h->W;
    hw_batch[2] = h->batch;
    hw_batch[3] = h->have_grad ? 1 : 0;
}

static int layer_arg(const char *who, const y355_train *h, int k) {
    if (!h) return y355_fail(Y355_TRAIN_EINVAL, std::string(who) + ": null handle");
    if (k < 1 || k > NL) return y355_fail(Y355_TRAIN_EINVAL, std::string(who) + ": layer index must be 1..10");
    return 0;
}


static hipError_t launch_pack(y355_train *h, float lr, float momentum, float wd, int first, int update, hipStream_t s) {
    hipLaunchKernelGGL(train_sgd_kernel, dim3((unsigned)((h->d.total + 255) / 256)), dim3(256), 0, s, h->d, h->p, h->g, h->m, h->packs, lr, momentum,
                       wd, first, update);
    return hipGetLastError();
}

// [B, h, w, c] of a tensor at the current size; 0 on a kind / index that does not exist
static bool tensor_dims(const y355_train *h, int kind, int t, int *shape) {
    int div, c;
    if (kind == Y355_TRAIN_ACT && t >= 0 && t <= 9) {
        div = act_div(t);
        c = act_c(h, t);
    } else if (kind == Y355_TRAIN_IDX && t >= 1 && t <= 9 && kPool[t - 1]) {
        div = act_div(t);
        c = act_c(h, t);
    } else if (kind == Y355_TRAIN_GRAD && t >= 1 && t <= NL) {
        div = kDiv[t - 1];
        c = h->d.L[t - 1].coutp;
    } else {
        return false;
    }
    shape[0] = h->batch;
    shape[1] = h->H / div;
    shape[2] = h->W / div;
    shape[3] = c;
    return true;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_train_last_error(void) { return g_err.c_str(); }

int y355_train_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_train **out) {
    if (int rc = train_open(max_h, max_w, num_classes, num_anchors, max_batch, y355_hip_mem(), out)) return rc;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    (*out)->device_id = dev;
    const int rc = e != hipSuccess ? y355_fail(Y355_TRAIN_EHIP, std::string("y355_train_create: ") + hipGetErrorString(e)) : train_buffers(*out);
    if (rc) {
        train_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_train_destroy(y355_train *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->device_id);
    train_free(h);
}

int y355_train_set_size(y355_train *h, int32_t height, int32_t width) {
    if (!h) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_set_size: null handle");
    if (height < 16 || width < 16 || height % 16 || width % 16)
        return y355_fail(Y355_TRAIN_EINVAL, "y355_train_set_size: height and width must be multiples of 16");
    if (height > h->max_h || width > h->max_w) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_set_size: size beyond the handle's maximum");
    if (height != h->H || width != h->W) {
        h->H = height;
        h->W = width;
        h->batch = 0;                                         // the stored tensors are of another size
        h->have_grad = false;
    }
    return Y355_TRAIN_OK;
}

int y355_train_layer_shape(const y355_train *h, int32_t k, int32_t *shape) {
    if (int rc = layer_arg("y355_train_layer_shape", h, k)) return rc;
    if (!shape) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_layer_shape: null argument");
    shape[0] = h->d.L[k - 1].cout;
    shape[1] = h->d.L[k - 1].cin;
    return Y355_TRAIN_OK;
}

int y355_train_load_layer(y355_train *h, int32_t k, const float *w, const float *b) {
    if (int rc = layer_arg("y355_train_load_layer", h, k)) return rc;
    if (!w || !b) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_load_layer: null argument");
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->p + L.woff, w, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->p + L.boff, b, (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(launch_pack(h, 0.f, 0.f, 0.f, 0, 0, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return Y355_TRAIN_OK;
}

static int get_pair(const char *who, y355_train *h, int k, const float *src, float *w, float *b) {
    if (int rc = layer_arg(who, h, k)) return rc;
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    if (w) HIPCHK(hipMemcpy(w, src + L.woff, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b, src + L.boff, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_TRAIN_OK;
}

int y355_train_get_layer(y355_train *h, int32_t k, float *w, float *b) { return get_pair("y355_train_get_layer", h, k, h ? h->p : nullptr, w, b); }

int y355_train_get_grad(y355_train *h, int32_t k, float *dw, float *db) {
    if (int rc = layer_arg("y355_train_get_grad", h, k)) return rc;
    if (!h->have_grad) return y355_fail(Y355_TRAIN_ENOTREADY, "y355_train_get_grad: no backward pass has run");
    return get_pair("y355_train_get_grad", h, k, h->g, dw, db);
}

int y355_train_get_momentum(y355_train *h, int32_t k, float *mw, float *mb) {
    return get_pair("y355_train_get_momentum", h, k, h ? h->m : nullptr, mw, mb);
}

int y355_train_get_packed(y355_train *h, int32_t k, uint16_t *w_bf16) {
    if (int rc = layer_arg("y355_train_get_packed", h, k)) return rc;
    if (!w_bf16) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_get_packed: null argument");
    const LayerDesc &L = h->d.L[k - 1];
    const int tf = ((L.cout + 15) / 16 + L.ct - 1) / L.ct * L.ct;
    std::vector<bf16_t> pk((size_t)tf * L.ksf * 512);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pk.data(), h->packs + L.wf_off, pk.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
    for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                const int kidx = tap * L.cinp + ci;
                w_bf16[((size_t)co * L.cin + ci) * 9 + tap] =
                    pk[((((size_t)(co >> 4) * L.ksf + (kidx >> 5)) * 64 + ((kidx >> 3) & 3) * 16 + (co & 15)) << 3) + (kidx & 7)];
            }
    return Y355_TRAIN_OK;
}

int y355_train_forward(y355_train *h, const void *x_dev, int32_t batch, void *stream) {
    if (!h || !x_dev) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_forward: null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_forward: batch must be 1..max_batch");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->batch = 0;
    h->have_grad = false;
    const size_t npix = (size_t)batch * h->H * h->W;
    hipLaunchKernelGGL(train_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const float *)x_dev, h->act[0], npix,
                       (size_t)h->H * h->W);
    HIPCHK(hipGetLastError());
    for (int k = 1; k <= NL; ++k) {
        const LayerDesc &L = h->d.L[k - 1];
        ConvArgs a{};
        a.in = h->act[k - 1];
        a.w = h->packs + L.wf_off;
        a.bias = h->p + L.boff;
        a.cinp_log2 = ilog2_(L.cinp);
        a.ks = L.ksf;
        a.B = batch;
        a.H = h->H / kDiv[k - 1];
        a.W = h->W / kDiv[k - 1];
        a.cout = L.cout;
        a.outc = L.cout;
        const int tiles = (L.cout + 15) / 16;
        if (k == NL) {
            a.out = h->pred;
            HIPCHK(launch_conv<M_PRED>(a, L.ct, tiles, s));
        } else if (kPool[k - 1]) {
            a.out = h->act[k];
            a.idx = h->idx[k];
            HIPCHK(launch_conv<M_FWD_POOL>(a, L.ct, tiles, s));
        } else {
            a.out = h->act[k];
            HIPCHK(launch_conv<M_FWD>(a, L.ct, tiles, s));
        }
    }
    h->batch = batch;
    return Y355_TRAIN_OK;
}

int y355_train_pred(y355_train *h, void **out) {
    if (!h || !out) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_pred: null argument");
    *out = h->pred;
    return Y355_TRAIN_OK;
}

int y355_train_backward(y355_train *h, const void *dpred_dev, void *stream) {
    if (!h || !dpred_dev) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_backward: null argument");
    if (h->batch == 0) return y355_fail(Y355_TRAIN_ENOTREADY, "y355_train_backward: no forward pass has run at this size");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->have_grad = false;
    const int B = h->batch;
    {
        const LayerDesc &L = h->d.L[NL - 1];
        const size_t hw = (size_t)(h->H / 16) * (h->W / 16), n = (size_t)B * hw * L.coutp;
        hipLaunchKernelGGL(train_dpred_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)dpred_dev, h->grad[NL], n, L.cout,
                           ilog2_(L.coutp), hw);
        HIPCHK(hipGetLastError());
    }
    for (int k = NL; k >= 1; --k) {
        const LayerDesc &L = h->d.L[k - 1];
        const int H = h->H / kDiv[k - 1], W = h->W / kDiv[k - 1];
        WgradArgs wa{};
        wa.g = h->grad[k];
        wa.act = h->act[k - 1];
        wa.ws = h->ws;
        wa.ws_stride = wgrad_stride(L);
        const WgradPlan plan = wgrad_plan(L, B, H, W);
        const int runs = plan.runs;
        wa.npix = plan.npix;
        wa.chunk = plan.chunk;
        wa.H = H;
        wa.W = W;
        wa.cinp = L.cinp;
        wa.coutp = L.coutp;
        wa.cout = L.cout;
        const int mt = wgrad_mt(L);
        const dim3 grid((unsigned)((L.cinp + 15) / 16), (unsigned)((L.cout + 16 * mt - 1) / (16 * mt)), (unsigned)runs), block(64);
        if (mt == 1) hipLaunchKernelGGL((train_wgrad_kernel<1>), grid, block, 0, s, wa);
        else if (mt == 2) hipLaunchKernelGGL((train_wgrad_kernel<2>), grid, block, 0, s, wa);
        else hipLaunchKernelGGL((train_wgrad_kernel<4>), grid, block, 0, s, wa);
        HIPCHK(hipGetLastError());
        const size_t n = (size_t)L.cout * L.cin * 9 + L.cout;
        hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->ws, wa.ws_stride, runs, L.cin, L.cinp, L.cout,
                           h->g + L.woff, h->g + L.boff);
        HIPCHK(hipGetLastError());
        if (k == 1) break;                                    // the gradient with respect to the image is not computed
        ConvArgs a{};
        a.in = h->grad[k];
        a.w = h->packs + L.wd_off;
        a.cinp_log2 = ilog2_(L.coutp);
        a.ks = L.ksd;
        a.B = B;
        a.H = H;
        a.W = W;
        a.cout = L.cin;
        a.outc = L.cin;
        a.out = h->grad[k - 1];
        a.act_prev = h->act[k - 1];
        if (kPool[k - 2]) {
            a.idx_prev = h->idx[k - 1];
            HIPCHK(launch_conv<M_DGRAD_UNPOOL>(a, L.dct, L.cin / 16, s));
        } else {
            HIPCHK(launch_conv<M_DGRAD>(a, L.dct, L.cin / 16, s));
        }
    }
    h->have_grad = true;
    return Y355_TRAIN_OK;
}

int y355_train_wgrad_plan(const y355_train *h, int32_t k, int32_t batch, int32_t *out) {
    if (int rc = layer_arg("y355_train_wgrad_plan", h, k)) return rc;
    if (!out) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_wgrad_plan: null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_wgrad_plan: batch must be 1..max_batch");
    const WgradPlan p = wgrad_plan(h->d.L[k - 1], batch, h->H / kDiv[k - 1], h->W / kDiv[k - 1]);
    if (p.npix > (size_t)INT32_MAX) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_wgrad_plan: more than 2^31 - 1 pixels");
    out[0] = (int32_t)p.npix;
    out[1] = p.max_runs;
    out[2] = p.runs;
    out[3] = (int32_t)p.chunk;
    return Y355_TRAIN_OK;
}

int y355_train_sgd_step(y355_train *h, float lr, float momentum, float weight_decay, void *stream) {
    if (!h) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_sgd_step: null handle");
    if (!(lr == lr) || !(momentum == momentum) || !(weight_decay == weight_decay))
        return y355_fail(Y355_TRAIN_EINVAL, "y355_train_sgd_step: lr, momentum and weight_decay must be numbers");
    if (!h->have_grad) return y355_fail(Y355_TRAIN_ENOTREADY, "y355_train_sgd_step: no backward pass has run");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_pack(h, lr, momentum, weight_decay, h->steps == 0 ? 1 : 0, 1, (hipStream_t)stream));
    ++h->steps;
    return Y355_TRAIN_OK;
}

int y355_train_tensor_shape(const y355_train *h, int32_t kind, int32_t t, int32_t *shape) {
    if (!h || !shape) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_tensor_shape: null argument");
    if (!tensor_dims(h, kind, t, shape)) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_tensor_shape: no such tensor");
    return Y355_TRAIN_OK;
}

int y355_train_get_tensor(y355_train *h, int32_t kind, int32_t t, void *out) {
    if (!h || !out) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_get_tensor: null argument");
    int shape[4];
    if (!tensor_dims(h, kind, t, shape)) return y355_fail(Y355_TRAIN_EINVAL, "y355_train_get_tensor: no such tensor");
    if (h->batch == 0) return y355_fail(Y355_TRAIN_ENOTREADY, "y355_train_get_tensor: no forward pass has run at this size");
    if (kind == Y355_TRAIN_GRAD && !h->have_grad) return y355_fail(Y355_TRAIN_ENOTREADY, "y355_train_get_tensor: no backward pass has run");
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * shape[3];
    const void *src = kind == Y355_TRAIN_ACT ? (const void *)h->act[t] : kind == Y355_TRAIN_IDX ? (const void *)h->idx[t] : (const void *)h->grad[t];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, src, n * (kind == Y355_TRAIN_IDX ? 1 : 2), hipMemcpyDeviceToHost));
    return Y355_TRAIN_OK;
}

}  // extern "C"
