// The host side the training libraries share (train.hip; bntrain.hip, section 6n; qtrain.hip, section 6o:
// it has an input, a dP and a data-gradient launch of its own, so those here are marked as possibly unused), on the kernels
// of train_core.h: the handle's common state, the create rules with the layer table, the common device memory, the bodies of
// the entry points both headers declare, and the launches of a layer that both passes make.  Each library compiles its own copy
// (everything here is static, under the including file's hidden visibility) after
//     #define TRAIN_FAMILY "y355_train"        (or "y355_bntrain": the prefix of the entry points in every error text)
//     #include "train_core.h"
// What only bntrain.hip needs comes in as an argument: the last layer an index may name, the tensor kinds of its own, the
// second launch of the SGD step, its device memory between and inside the common requests.
#ifndef Y355_TRAIN_HOST_H
#define Y355_TRAIN_HOST_H
#ifndef TRAIN_FAMILY
#error "define TRAIN_FAMILY before including train_host.h"
#endif
#define TRAIN_FN(name) TRAIN_FAMILY "_" name

enum { T_ACT = 0, T_IDX = 1, T_GRAD = 2 };       // the tensor kinds both headers have (each library asserts its header's numbers)

// ---------------------------------------------------------------------------------------------------------- the handle
struct TrainDev {                    // the common device memory, all of it TrainCore::own's: core_rollback resets it in one assignment
    float *p = nullptr, *g = nullptr, *m = nullptr;
    bf16_t *packs = nullptr;
    bf16_t *act[NL] = {};            // A_0 .. A_9
    unsigned char *idx[NL] = {};     // I_t, t = 1, 2, 4, 6 (index t)
    bf16_t *grad[NL + 1] = {};       // G_1 .. G_10 (index k)
    float *pred = nullptr, *ws = nullptr;
};
struct TrainCore : TrainDev {
    DevOwner own;
    int device_id = 0;
    int max_h = 0, max_w = 0, max_batch = 0, num_classes = 0, num_anchors = 0;
    int H = 0, W = 0;
    int batch = 0;                   // of the last forward at this size (0: none)
    bool have_grad = false;          // a backward since the last forward
    long long steps = 0;
    NetDesc d;
    size_t pack_total = 0, ws_total = 0;
};

// channels and grid divisor of A_t
static int act_c(const TrainCore *h, int t) { return t == 0 ? 8 : h->d.L[t - 1].cout; }
static int act_div(int t) { return t == 0 ? 1 : kDiv[t - 1] * (kPool[t - 1] ? 2 : 1); }

// <family>_create in two parts, as the host checks run them on the CPU: the rules and the host state of a new H (no device
// call), ...
template <class H>
static int core_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, H **out) {
    if (!out) return y355_fail(Y355_EINVAL, TRAIN_FN("create") ": null argument");
    *out = nullptr;
    if (max_h < 16 || max_w < 16 || max_h % 16 || max_w % 16 || max_h > 4096 || max_w > 4096)
        return y355_fail(Y355_EINVAL, TRAIN_FN("create") ": max_h and max_w must be multiples of 16 in 16..4096");
    if (num_classes < 1 || num_classes > 200) return y355_fail(Y355_EINVAL, TRAIN_FN("create") ": num_classes must be 1..200");
    if (num_anchors < 1 || num_anchors > 16) return y355_fail(Y355_EINVAL, TRAIN_FN("create") ": num_anchors must be 1..16");
    if (max_batch < 1 || max_batch > 1024) return y355_fail(Y355_EINVAL, TRAIN_FN("create") ": max_batch must be 1..1024");
    H *h = new H;
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
        L.wf_off = poff;
        poff += forward_pack_size(L);
        L.wd_off = poff;
        if (k > 0) poff += (size_t)(L.cin / 16) * L.ksd * 512;
        h->ws_total = std::max(h->ws_total, (size_t)wgrad_max_runs(L) * wgrad_stride(L));
    }
    h->d.total = off;
    h->pack_total = poff;
    *out = h;
    return Y355_OK;
}

static void core_rollback(TrainCore *h, size_t mark) {
    y355_dev_rollback(h->own, mark);
    static_cast<TrainDev &>(*h) = TrainDev{};
}
// ... and all of the common device memory (on the current device), or none of it.  The order of the requests is part of the
// contract (the host checks count them and read blocks by their index; it also places the blocks), so the including library's
// own ones keep their places: own_params() asks for what follows the parameters, own_grid(k, n) for what follows G_k, of the n
// elements of layer k's pre-pool grid at coutp channels.  A failure of either is a failure of the whole: the caller nulls its own.
template <class OwnParams, class OwnGrid>
static int core_buffers(TrainCore *h, OwnParams own_params, OwnGrid own_grid) {
    DevOwner &o = h->own;
    const size_t mark = y355_dev_mark(o);
    const size_t B = h->max_batch;
    int rc = y355_dev_get_all<true>(o, h->d.total, &h->p, &h->g, &h->m);
    rc = rc ? rc : own_params();
    rc = rc ? rc : y355_dev_get(o, &h->packs, h->pack_total, true);
    rc = rc ? rc : y355_dev_get(o, &h->ws, h->ws_total, true);
    for (int t = 0; t < NL && !rc; ++t) {
        const size_t n = B * (h->max_h / act_div(t)) * (h->max_w / act_div(t)) * act_c(h, t);
        rc = y355_dev_get(o, &h->act[t], n, true);
        if (!rc && t >= 1 && kPool[t - 1]) rc = y355_dev_get(o, &h->idx[t], n, true);
    }
    for (int k = 1; k <= NL && !rc; ++k) {
        const size_t n = B * (h->max_h / kDiv[k - 1]) * (h->max_w / kDiv[k - 1]) * h->d.L[k - 1].coutp;
        rc = y355_dev_get(o, &h->grad[k], n, true);
        rc = rc ? rc : own_grid(k, n);
    }
    rc = rc ? rc : y355_dev_get(o, &h->pred, B * h->d.L[NL - 1].cout * (h->max_h / 16) * (h->max_w / 16), true);
    if (rc) core_rollback(h, mark);
    return rc;
}
template <class H>
static void core_free(H *h) {
    y355_dev_release_all(h->own);
    delete h;
}
static void core_state(const TrainCore *h, int *hw_batch) {   // H, W, batch of the last forward, have_grad: for the host checks
    hw_batch[0] = h->H;
    hw_batch[1] = h->W;
    hw_batch[2] = h->batch;
    hw_batch[3] = h->have_grad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------- entry points
// layer index k of an entry point `who`: 1..NL, or 1..last for what exists on fewer layers
static int layer_arg(const char *who, const TrainCore *h, int k, int last = NL) {
    if (!h) return y355_fail(Y355_EINVAL, std::string(who) + ": null handle");
    if (k < 1 || k > last) return y355_fail(Y355_EINVAL, std::string(who) + (last == NL ? ": layer index must be 1..10" : ": layer index must be 1..9"));
    return 0;
}

static hipError_t launch_pack(TrainCore *h, float lr, float momentum, float wd, int first, int update, hipStream_t s) {
    hipLaunchKernelGGL(train_sgd_kernel, dim3((unsigned)((h->d.total + 255) / 256)), dim3(256), 0, s, h->d, h->p, h->g, h->m, h->packs, lr, momentum,
                       wd, first, update);
    return hipGetLastError();
}

template <class H>
static int core_create(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, H **out,
                       int (*open)(int, int, int, int, int, const DevMem &, H **), int (*buffers)(H *)) {
    if (int rc = open(max_h, max_w, num_classes, num_anchors, max_batch, y355_hip_mem(), out)) return rc;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    (*out)->device_id = dev;
    const int rc = e != hipSuccess ? y355_fail(Y355_EHIP, std::string(TRAIN_FN("create") ": ") + hipGetErrorString(e)) : buffers(*out);
    if (rc) {
        core_free(*out);
        *out = nullptr;
    }
    return rc;
}

template <class H>
static void core_destroy(H *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->device_id);
    core_free(h);
}

static int core_set_size(TrainCore *h, int height, int width) {
    if (!h) return y355_fail(Y355_EINVAL, TRAIN_FN("set_size") ": null handle");
    if (height < 16 || width < 16 || height % 16 || width % 16)
        return y355_fail(Y355_EINVAL, TRAIN_FN("set_size") ": height and width must be multiples of 16");
    if (height > h->max_h || width > h->max_w) return y355_fail(Y355_EINVAL, TRAIN_FN("set_size") ": size beyond the handle's maximum");
    if (height != h->H || width != h->W) {
        h->H = height;
        h->W = width;
        h->batch = 0;                                         // the stored tensors are of another size
        h->have_grad = false;
    }
    return Y355_OK;
}

static int core_layer_shape(const TrainCore *h, int k, int32_t *shape) {
    if (int rc = layer_arg(TRAIN_FN("layer_shape"), h, k)) return rc;
    if (!shape) return y355_fail(Y355_EINVAL, TRAIN_FN("layer_shape") ": null argument");
    shape[0] = h->d.L[k - 1].cout;
    shape[1] = h->d.L[k - 1].cin;
    return Y355_OK;
}

static int core_load_layer(TrainCore *h, int k, const float *w, const float *b) {
    if (int rc = layer_arg(TRAIN_FN("load_layer"), h, k)) return rc;
    if (!w || !b) return y355_fail(Y355_EINVAL, TRAIN_FN("load_layer") ": null argument");
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->p + L.woff, w, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->p + L.boff, b, (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(launch_pack(h, 0.f, 0.f, 0.f, 0, 0, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return Y355_OK;
}

// W_k and b_k of one of the flat arrays (parameters, gradients, momenta) to the host pointers that are not null
static int get_pair(const char *who, TrainCore *h, int k, const float *src, float *w, float *b) {
    if (int rc = layer_arg(who, h, k)) return rc;
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    if (w) HIPCHK(hipMemcpy(w, src + L.woff, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b, src + L.boff, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_OK;
}
static int core_get_layer(TrainCore *h, int k, float *w, float *b) { return get_pair(TRAIN_FN("get_layer"), h, k, h ? h->p : nullptr, w, b); }
static int core_get_momentum(TrainCore *h, int k, float *mw, float *mb) { return get_pair(TRAIN_FN("get_momentum"), h, k, h ? h->m : nullptr, mw, mb); }
static int core_get_grad(TrainCore *h, int k, float *dw, float *db) {
    if (int rc = layer_arg(TRAIN_FN("get_grad"), h, k)) return rc;
    if (!h->have_grad) return y355_fail(Y355_ENOTREADY, TRAIN_FN("get_grad") ": no backward pass has run");
    return get_pair(TRAIN_FN("get_grad"), h, k, h->g, dw, db);
}

static int core_get_packed(TrainCore *h, int k, uint16_t *w_bf16) {
    if (int rc = layer_arg(TRAIN_FN("get_packed"), h, k)) return rc;
    if (!w_bf16) return y355_fail(Y355_EINVAL, TRAIN_FN("get_packed") ": null argument");
    const LayerDesc &L = h->d.L[k - 1];
    std::vector<bf16_t> pk(forward_pack_size(L));
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pk.data(), h->packs + L.wf_off, pk.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
    for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) w_bf16[((size_t)co * L.cin + ci) * 9 + tap] = pk[pack_index(co, L.ksf, tap * L.cinp + ci)];
    return Y355_OK;
}

static int core_pred(TrainCore *h, void **out) {
    if (!h || !out) return y355_fail(Y355_EINVAL, TRAIN_FN("pred") ": null argument");
    *out = h->pred;
    return Y355_OK;
}

static int core_wgrad_plan(const TrainCore *h, int k, int batch, int32_t *out) {
    if (int rc = layer_arg(TRAIN_FN("wgrad_plan"), h, k)) return rc;
    if (!out) return y355_fail(Y355_EINVAL, TRAIN_FN("wgrad_plan") ": null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_EINVAL, TRAIN_FN("wgrad_plan") ": batch must be 1..max_batch");
    const WgradPlan p = wgrad_plan(h->d.L[k - 1], batch, h->H / kDiv[k - 1], h->W / kDiv[k - 1]);
    if (p.npix > (size_t)INT32_MAX) return y355_fail(Y355_EINVAL, TRAIN_FN("wgrad_plan") ": more than 2^31 - 1 pixels");
    out[0] = (int32_t)p.npix;
    out[1] = p.max_runs;
    out[2] = p.runs;
    out[3] = (int32_t)p.chunk;
    return Y355_OK;
}

// own_launch(first): the including library's update of what train_sgd_kernel does not hold, on the same stream
template <class OwnLaunch>
static int core_sgd_step(TrainCore *h, float lr, float momentum, float weight_decay, void *stream, OwnLaunch own_launch) {
    if (!h) return y355_fail(Y355_EINVAL, TRAIN_FN("sgd_step") ": null handle");
    if (!(lr == lr) || !(momentum == momentum) || !(weight_decay == weight_decay))
        return y355_fail(Y355_EINVAL, TRAIN_FN("sgd_step") ": lr, momentum and weight_decay must be numbers");
    if (!h->have_grad) return y355_fail(Y355_ENOTREADY, TRAIN_FN("sgd_step") ": no backward pass has run");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    const int first = h->steps == 0 ? 1 : 0;
    HIPCHK(launch_pack(h, lr, momentum, weight_decay, first, 1, (hipStream_t)stream));
    HIPCHK(own_launch(first));
    ++h->steps;
    return Y355_OK;
}

// A tensor kind of the including library's own, on the pre-pool grid of layer t: its device memory, its channels (0: no such
// tensor) and whether only a backward fills it; the bytes of an element, and the divisor of its grid where it is another.
struct OwnTensor {
    const void *src;
    int c;
    bool of_backward;
    int elem = 2;
    int div = 0;
};
typedef OwnTensor (*OwnTensorFn)(const TrainCore *h, int kind, int t);

// [B, h, w, c] of a tensor at the current size, its memory, whether it needs a backward and the bytes of an element; false on
// a kind / index that does not exist
static bool tensor_dims(const TrainCore *h, int kind, int t, OwnTensorFn own, int *shape, const void **src = nullptr, bool *of_backward = nullptr,
                        int *elem = nullptr) {
    int div;
    OwnTensor o{nullptr, 0, false};
    if ((kind == T_ACT && t >= 0 && t <= 9) || (kind == T_IDX && t >= 1 && t <= 9 && kPool[t - 1])) {
        div = act_div(t);
        o = OwnTensor{kind == T_ACT ? (const void *)h->act[t] : (const void *)h->idx[t], act_c(h, t), false, kind == T_IDX ? 1 : 2};
    } else if (kind == T_GRAD && t >= 1 && t <= NL) {
        div = kDiv[t - 1];
        o = OwnTensor{h->grad[t], h->d.L[t - 1].coutp, true};
    } else if (own && (o = own(h, kind, t)).c) {
        div = o.div ? o.div : kDiv[t - 1];
    } else {
        return false;
    }
    shape[0] = h->batch;
    shape[1] = h->H / div;
    shape[2] = h->W / div;
    shape[3] = o.c;
    if (src) *src = o.src;
    if (of_backward) *of_backward = o.of_backward;
    if (elem) *elem = o.elem;
    return true;
}

static int core_tensor_shape(const TrainCore *h, int kind, int t, int32_t *shape, OwnTensorFn own = nullptr) {
    if (!h || !shape) return y355_fail(Y355_EINVAL, TRAIN_FN("tensor_shape") ": null argument");
    if (!tensor_dims(h, kind, t, own, shape)) return y355_fail(Y355_EINVAL, TRAIN_FN("tensor_shape") ": no such tensor");
    return Y355_OK;
}

static int core_get_tensor(TrainCore *h, int kind, int t, void *out, OwnTensorFn own = nullptr) {
    if (!h || !out) return y355_fail(Y355_EINVAL, TRAIN_FN("get_tensor") ": null argument");
    int shape[4];
    const void *src;
    bool of_backward;
    int elem;
    if (!tensor_dims(h, kind, t, own, shape, &src, &of_backward, &elem)) return y355_fail(Y355_EINVAL, TRAIN_FN("get_tensor") ": no such tensor");
    if (h->batch == 0) return y355_fail(Y355_ENOTREADY, TRAIN_FN("get_tensor") ": no forward pass has run at this size");
    if (of_backward && !h->have_grad) return y355_fail(Y355_ENOTREADY, TRAIN_FN("get_tensor") ": no backward pass has run");
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * shape[3];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, src, n * elem, hipMemcpyDeviceToHost));
    return Y355_OK;
}

// ---------------------------------------------------------------------------------------------------------- the passes
// The arguments of <family>_forward (a library's own rules follow them), ...
static int forward_args(const TrainCore *h, const void *x_dev, int batch) {
    if (!h || !x_dev) return y355_fail(Y355_EINVAL, TRAIN_FN("forward") ": null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_EINVAL, TRAIN_FN("forward") ": batch must be 1..max_batch");
    return 0;
}
// ... its first launch, A_0 = rb(x): from here on the handle holds no finished forward until the caller sets h->batch, ...
[[maybe_unused]] static hipError_t launch_input(TrainCore *h, const void *x_dev, int batch, hipStream_t s) {
    h->batch = 0;
    h->have_grad = false;
    const size_t npix = (size_t)batch * h->H * h->W;
    hipLaunchKernelGGL(train_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const float *)x_dev, h->act[0], npix,
                       (size_t)h->H * h->W);
    return hipGetLastError();
}
// ... and the convolution of layer k on A_{k-1} into out (idx: I_k of M_FWD_POOL): its arguments, and its launch with epilogue
// MODE (a library with epilogues of its own fills in the rest of the arguments and calls launch_conv itself)
static ConvArgs forward_conv_args(const TrainCore *h, int k, int batch, void *out, unsigned char *idx) {
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
    a.out = out;
    a.idx = idx;
    return a;
}
template <int MODE>
static hipError_t launch_forward(const TrainCore *h, int k, int batch, void *out, unsigned char *idx, hipStream_t s) {
    const LayerDesc &L = h->d.L[k - 1];
    return launch_conv<MODE>(forward_conv_args(h, k, batch, out, idx), L.ct, (L.cout + 15) / 16, s);
}

// The arguments of <family>_backward, ...
static int backward_args(const TrainCore *h, const void *dpred_dev) {
    if (!h || !dpred_dev) return y355_fail(Y355_EINVAL, TRAIN_FN("backward") ": null argument");
    if (h->batch == 0) return y355_fail(Y355_ENOTREADY, TRAIN_FN("backward") ": no forward pass has run at this size");
    return 0;
}
// ... its first launch, G_10 = rb(dP): from here on the handle holds no finished backward until the caller sets h->have_grad, ...
[[maybe_unused]] static hipError_t launch_dpred(TrainCore *h, const void *dpred_dev, hipStream_t s) {
    h->have_grad = false;
    const LayerDesc &L = h->d.L[NL - 1];
    const size_t hw = (size_t)(h->H / 16) * (h->W / 16), n = (size_t)h->batch * hw * L.coutp;
    hipLaunchKernelGGL(train_dpred_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)dpred_dev, h->grad[NL], n, L.cout,
                       ilog2_(L.coutp), hw);
    return hipGetLastError();
}
// ... dW_k and db_k from G_k and A_{k-1}: the runs of the plan, then their sum, ...
static hipError_t launch_wgrad(const TrainCore *h, int k, hipStream_t s) {
    const LayerDesc &L = h->d.L[k - 1];
    const int H = h->H / kDiv[k - 1], W = h->W / kDiv[k - 1];
    const WgradPlan plan = wgrad_plan(L, h->batch, H, W);
    WgradArgs wa{};
    wa.g = h->grad[k];
    wa.act = h->act[k - 1];
    wa.ws = h->ws;
    wa.ws_stride = wgrad_stride(L);
    wa.npix = plan.npix;
    wa.chunk = plan.chunk;
    wa.H = H;
    wa.W = W;
    wa.cinp = L.cinp;
    wa.coutp = L.coutp;
    wa.cout = L.cout;
    const int mt = wgrad_mt(L);
    const dim3 grid((unsigned)((L.cinp + 15) / 16), (unsigned)((L.cout + 16 * mt - 1) / (16 * mt)), (unsigned)plan.runs), block(64);
    if (mt == 1) hipLaunchKernelGGL((train_wgrad_kernel<1>), grid, block, 0, s, wa);
    else if (mt == 2) hipLaunchKernelGGL((train_wgrad_kernel<2>), grid, block, 0, s, wa);
    else hipLaunchKernelGGL((train_wgrad_kernel<4>), grid, block, 0, s, wa);
    if (const hipError_t e = hipGetLastError()) return e;
    const size_t n = (size_t)L.cout * L.cin * 9 + L.cout;
    hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->ws, wa.ws_stride, plan.runs, L.cin, L.cinp, L.cout,
                       h->g + L.woff, h->g + L.boff);
    return hipGetLastError();
}
// ... and the data gradient of layer k = 2..10 from G_k, through A_{k-1}'s slope mask and I_{k-1}, into dst on layer k - 1's grid
static ConvArgs dgrad_conv_args(const TrainCore *h, int k, bf16_t *dst) {
    const LayerDesc &L = h->d.L[k - 1];
    ConvArgs a{};
    a.in = h->grad[k];
    a.w = h->packs + L.wd_off;
    a.cinp_log2 = ilog2_(L.coutp);
    a.ks = L.ksd;
    a.B = h->batch;
    a.H = h->H / kDiv[k - 1];
    a.W = h->W / kDiv[k - 1];
    a.cout = L.cin;
    a.outc = L.cin;
    a.out = dst;
    a.act_prev = h->act[k - 1];
    return a;
}
[[maybe_unused]] static hipError_t launch_dgrad(const TrainCore *h, int k, bf16_t *dst, hipStream_t s) {
    const LayerDesc &L = h->d.L[k - 1];
    ConvArgs a = dgrad_conv_args(h, k, dst);
    if (!kPool[k - 2]) return launch_conv<M_DGRAD>(a, L.dct, L.cin / 16, s);
    a.idx_prev = h->idx[k - 1];
    return launch_conv<M_DGRAD_UNPOOL>(a, L.dct, L.cin / 16, s);
}
#endif
