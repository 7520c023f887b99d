// yolo355_grad -- the four training losses together with their gradient with respect to the prediction maps on the GPU
// (gfx950); C ABI in include/yolo355_grad.h, linked into libyolo355_grad.so on its own (nothing of libyolo355.so or
// libyolo355_loss.so is used).  The loss arithmetic, assign_kernel and loss_finish_kernel are loss_core.h's, which loss.hip
// compiles too: the value returned here is y355_loss_compute's bit for bit.
//
//   grad_terms_kernel   the walk of loss_terms_kernel (item i = base[level] + a * HW + cell: consecutive lanes on consecutive
//                       cells of one NCHW channel, so every read and every write of a channel is coalesced), the same terms
//                       and sums, and per anchor its 5 + C gradient channels, written by the one thread that owns the anchor:
//                       no atomics, every element written exactly once
//   grad_flat_kernel    the same on the flat tensors tools.loss itself takes
// <VALUE, GRAD>: terms and sums / gradient channels, either or both.  CMAX: the softmax needs an anchor's class logits twice
// (maximum and sum, then the quotient); for C <= CMAX they stay in registers between the two, above it they are read again.
//
// The upstream gradients are four floats on the device, read by the kernel: a backward pass never waits for the host.
#include "../../include/yolo355_grad.h"
#pragma GCC visibility push(hidden)
#include "loss_core.h"
static_assert(Y355_GRAD_OK == Y355_OK && Y355_GRAD_EINVAL == Y355_EINVAL && Y355_GRAD_EHIP == Y355_EHIP && Y355_GRAD_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

#ifndef Y355_GRAD_CREG
#define Y355_GRAD_CREG 24        // class logits kept in registers up to this C (measured against 0, 20 and 32)
#endif

static thread_local std::string g_err;                  // y355_grad_last_error's text
#ifndef Y355_HOSTCHECK                                   // (grad_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

struct y355_grad : LossState {};

struct GradPtrs {
    float *p[MAXL];
};
// k_conf, k_cls, k_box: (the group's upstream + total_loss's) / batch, each computed once in fp32 and applied last
struct GradK {
    float conf, cls, box;
};
__device__ __forceinline__ GradK grad_k_(const float *__restrict__ up, int batch) {
    const float u_conf = up ? up[0] : 0.0f, u_cls = up ? up[1] : 0.0f, u_box = up ? up[2] : 0.0f, u_tot = up ? up[3] : 1.0f;
    const float fb = (float)batch;
    GradK k;
    k.conf = (u_conf + u_tot) / fb;
    k.cls = (u_cls + u_tot) / fb;
    k.box = (u_box + u_tot) / fb;
    return k;
}

// One anchor: its five terms into acc (VALUE) and its gradient channels (GRAD): g_conf, g_cls[c * gcs], g_box[j * gbs].
// x(c): the class logits, as cls_stat_<CMAX> takes them.
template <bool VALUE, bool GRAD, int CMAX, typename Logit>
__device__ __forceinline__ void anchor_pass_(float conf, Logit x, int C, float tx, float ty, float tw, float th, float iou, float t_obj,
                                             float t_cls, float t_tx, float t_ty, float t_tw, float t_th, float t_wt, float obj_w,
                                             float noobj_w, const GradK &k, double *acc, float *g_conf, float *g_cls, size_t gcs,
                                             float *g_box, size_t gbs) {
    const ClsStat st = cls_stat_<CMAX>(x, C, t_cls);
    if constexpr (VALUE) {
        float term[5];
        loss_terms_(conf, st, tx, ty, tw, th, iou, t_obj, t_tx, t_ty, t_tw, t_th, t_wt, term);
        for (int j = 0; j < 5; ++j) acc[j] += (double)term[j];
    }
    if constexpr (GRAD) {
        const float s = sigmoidf_(conf);
        const float pos = t_obj == 1.0f ? 1.0f : 0.0f, neg = t_obj == 0.0f ? 1.0f : 0.0f, mask = t_wt > 0.0f ? 1.0f : 0.0f;
        *g_conf = (((obj_w * pos) * (2.0f * (s - iou)) + (noobj_w * neg) * (2.0f * s)) * (s * (1.0f - s))) * k.conf;
        if constexpr (CMAX == 0) {
            for (int c = 0; c < C; ++c)
                g_cls[(size_t)c * gcs] = (((expf(x(c) - st.m) / st.se) - (c == st.kc ? 1.0f : 0.0f)) * mask) * k.cls;
        } else {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) g_cls[(size_t)c * gcs] = (((expf(x(c) - st.m) / st.se) - (c == st.kc ? 1.0f : 0.0f)) * mask) * k.cls;
        }
        g_box[0] = (((sigmoidf_(tx) - t_tx) * t_wt) * mask) * k.box;
        g_box[gbs] = (((sigmoidf_(ty) - t_ty) * t_wt) * mask) * k.box;
        g_box[2 * gbs] = (((2.0f * (tw - t_tw)) * t_wt) * mask) * k.box;
        g_box[3 * gbs] = (((2.0f * (th - t_th)) * t_wt) * mask) * k.box;
    }
}

template <bool VALUE, bool GRAD, int CMAX>
__global__ __launch_bounds__(LOSS_THREADS) void grad_terms_kernel(const LossDev p, const PredPtrs pp, const float *__restrict__ target,
                                                                  const float *__restrict__ up, float obj_w, float noobj_w, const GradPtrs gp,
                                                                  double *__restrict__ partial) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int b = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
    const int A = p.A, C = p.C;
    const GradK k = grad_k_(up, (int)gridDim.y);
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * LOSS_THREADS + tid; i < p.N; i += nblk * LOSS_THREADS) {
        const AnchorAt q = anchor_at_(p, i);
        const size_t HW = q.HW;
        const size_t at = (size_t)b * A * (5 + C) * HW + q.cell;                 // of the image's map, this cell
        const size_t o_conf = at + (size_t)q.a * HW, o_cls = at + (size_t)(A + q.a * C) * HW, o_box = at + (size_t)(A * (1 + C) + q.a * 4) * HW;
        const float *pm = pp.p[q.lv];
        const float *t = target + ((size_t)b * p.N + p.base[q.lv] + (size_t)q.cell * A + q.a) * NF;
        const float conf = pm[o_conf];
        const float *pc = pm + o_cls, *pb = pm + o_box;
        const float tx = pb[0], ty = pb[HW], tw = pb[2 * HW], th = pb[3 * HW];
        const float iou = anchor_iou_(p, q, tx, ty, tw, th, t);
        float *g = GRAD ? gp.p[q.lv] : nullptr;
        if constexpr (CMAX > 0) {
            float x[CMAX];                                                        // constant indices only: registers
#pragma unroll
            for (int c = 0; c < CMAX; ++c) x[c] = c < C ? pc[(size_t)c * HW] : 0.0f;
            anchor_pass_<VALUE, GRAD, CMAX>(conf, [&x](int c) { return x[c]; }, C, tx, ty, tw, th, iou, t[0], t[1], t[2], t[3], t[4], t[5], t[6],
                                            obj_w, noobj_w, k, acc, g + o_conf, g + o_cls, HW, g + o_box, HW);
        } else {
            anchor_pass_<VALUE, GRAD, 0>(conf, [pc, HW](int c) { return pc[(size_t)c * HW]; }, C, tx, ty, tw, th, iou, t[0], t[1], t[2], t[3], t[4],
                                         t[5], t[6], obj_w, noobj_w, k, acc, g + o_conf, g + o_cls, HW, g + o_box, HW);
        }
    }
    if constexpr (VALUE) block_partial(acc, s_part, partial + ((size_t)b * nblk + blockIdx.x) * 5);
}

// conf [B][N], cls [B][N][C], txtytwth [B][N][4], label [B][N][8] = iou, obj, cls, tx, ty, tw, th, weight; the gradients in the
// layouts of the first three
template <bool VALUE, bool GRAD>
__global__ __launch_bounds__(LOSS_THREADS) void grad_flat_kernel(const float *__restrict__ conf, const float *__restrict__ cls,
                                                                 const float *__restrict__ box, const float *__restrict__ label, int N, int C,
                                                                 const float *__restrict__ up, float obj_w, float noobj_w, float *__restrict__ g_conf,
                                                                 float *__restrict__ g_cls, float *__restrict__ g_box, double *__restrict__ partial) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int b = blockIdx.y, nblk = gridDim.x;
    const GradK k = grad_k_(up, (int)gridDim.y);
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = blockIdx.x * LOSS_THREADS + threadIdx.x; n < N; n += nblk * LOSS_THREADS) {
        const size_t i = (size_t)b * N + n;
        const float *L = label + i * 8, *pb = box + i * 4, *pc = cls + i * C;
        anchor_pass_<VALUE, GRAD, 0>(conf[i], [pc](int c) { return pc[c]; }, C, pb[0], pb[1], pb[2], pb[3], L[0], L[1], L[2], L[3], L[4], L[5], L[6],
                                     L[7], obj_w, noobj_w, k, acc, GRAD ? g_conf + i : nullptr, GRAD ? g_cls + i * C : nullptr, 1,
                                     GRAD ? g_box + i * 4 : nullptr, 1);
    }
    if constexpr (VALUE) block_partial(acc, s_part, partial + ((size_t)b * nblk + blockIdx.x) * 5);
}

// ---------------------------------------------------------------------------------------------------------- the handle
// y355_grad_create in two parts, as grad_host_check.cpp runs them on the CPU: the rules of a configuration and the host state
// (no device call; the handle gets its device memory from mem), ...
int grad_open(const y355_loss_config *cfg, const DevMem &mem, y355_grad **out) {
    if (!cfg || !out) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_create: null argument");
    *out = nullptr;
    y355_grad st;
    if (int rc = loss_rules(*cfg, mem, &st)) return rc;
    *out = new y355_grad(st);
    return Y355_GRAD_OK;
}
// ... and all of its device memory (on the current device), or none of it
int grad_buffers(y355_grad *h) { return loss_state_buffers(h); }
DevOwner &grad_owner(y355_grad *h) { return h->own; }      // (grad_host_check.cpp does not see the struct)
void grad_free(y355_grad *h) {
    y355_dev_release_all(h->own);
    delete h;
}

// one terms-and-gradient launch of the map form on s (the caller has set the device)
template <bool VALUE, bool GRAD>
static hipError_t launch_terms(const y355_grad *h, const PredPtrs &pp, const float *target, int batch, const void *upstream_dev,
                               const GradPtrs &gp, hipStream_t s) {
    const dim3 grid(h->nblk, batch), block(LOSS_THREADS);
    const float obj_w = (float)h->cfg.obj_weight, noobj_w = (float)h->cfg.noobj_weight;
    const float *up = (const float *)upstream_dev;
    if (GRAD && Y355_GRAD_CREG > 0 && h->dev.C <= Y355_GRAD_CREG)
        hipLaunchKernelGGL((grad_terms_kernel<VALUE, GRAD, GRAD ? Y355_GRAD_CREG : 0>), grid, block, 0, s, h->dev, pp, target, up, obj_w, noobj_w, gp,
                           h->partial);
    else
        hipLaunchKernelGGL((grad_terms_kernel<VALUE, GRAD, 0>), grid, block, 0, s, h->dev, pp, target, up, obj_w, noobj_w, gp, h->partial);
    return hipGetLastError();
}

// the checks forward_backward and backward share, before any HIP call
static int map_args(const std::string &who, const y355_grad *h, const void *const *pred_dev, const void *target_dev, int32_t batch,
                    void *const *grad_dev, PredPtrs *pp, GradPtrs *gp, const float **target) {
    if (batch < 1 || batch > h->cfg.max_batch) return y355_fail(Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    *pp = PredPtrs{};
    *gp = GradPtrs{};
    for (int l = 0; l < h->dev.nlev; ++l) {
        if (!pred_dev[l]) return y355_fail(Y355_GRAD_EINVAL, who + ": null prediction map");
        if (grad_dev && !grad_dev[l]) return y355_fail(Y355_GRAD_EINVAL, who + ": null gradient map");
        pp->p[l] = (const float *)pred_dev[l];
        gp->p[l] = grad_dev ? (float *)grad_dev[l] : nullptr;
    }
    return loss_pick_target(who, h, target_dev, batch, target);
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_grad_last_error(void) { return g_err.c_str(); }

int y355_grad_create(const y355_loss_config *cfg, y355_grad **out) {
    if (int rc = grad_open(cfg, y355_hip_mem(), out)) return rc;
    DeviceGuard g;
    const hipError_t e = g.set(cfg->device_id);
    const int rc = e != hipSuccess ? y355_fail(Y355_GRAD_EHIP, std::string("y355_grad_create: ") + hipGetErrorString(e)) : grad_buffers(*out);
    if (rc) {
        grad_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_grad_destroy(y355_grad *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->cfg.device_id);
    grad_free(h);
}

int y355_grad_num_anchors_total(const y355_grad *h) { return h ? h->dev.N : y355_fail(Y355_GRAD_EINVAL, "null handle"); }

int y355_grad_set_labels(y355_grad *h, const int32_t *offsets, const double *labels, int32_t batch) {
    if (!h || !offsets) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_set_labels: null argument");
    return loss_set_labels("y355_grad_set_labels", h, offsets, labels, batch);
}

int y355_grad_targets_dev(y355_grad *h, int32_t batch, const void **out) {
    if (!h || !out) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_targets_dev: null argument");
    *out = nullptr;
    if (h->labels_batch == 0) return y355_fail(Y355_GRAD_ENOTREADY, "y355_grad_targets_dev: no labels set");
    if (batch < 1 || batch > h->labels_batch) return y355_fail(Y355_GRAD_EINVAL, "batch must be 1..the batch of y355_grad_set_labels");
    *out = h->target;
    return Y355_GRAD_OK;
}

int y355_grad_forward_backward(y355_grad *h, const void *const *pred_dev, const void *target_dev, int32_t batch, const void *upstream_dev,
                               void *const *grad_dev, void *stream, double *out, double *per_image) {
    if (!h || !pred_dev || !out) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_forward_backward: null argument");
    PredPtrs pp;
    GradPtrs gp;
    const float *target = nullptr;
    if (int rc = map_args("y355_grad_forward_backward", h, pred_dev, target_dev, batch, grad_dev, &pp, &gp, &target)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    HIPCHK((grad_dev ? launch_terms<true, true>(h, pp, target, batch, upstream_dev, gp, s)
                     : launch_terms<true, false>(h, pp, target, batch, upstream_dev, gp, s)));
    HIPCHK(loss_finish(h->partial, h->nblk, batch, h->cfg.obj_weight, h->cfg.noobj_weight, h->per_image, h->out, s, out, per_image));
    return Y355_GRAD_OK;
}

int y355_grad_backward(y355_grad *h, const void *const *pred_dev, const void *target_dev, int32_t batch, const void *upstream_dev,
                       void *const *grad_dev, void *stream) {
    if (!h || !pred_dev || !grad_dev) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_backward: null argument");
    PredPtrs pp;
    GradPtrs gp;
    const float *target = nullptr;
    if (int rc = map_args("y355_grad_backward", h, pred_dev, target_dev, batch, grad_dev, &pp, &gp, &target)) return rc;
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    HIPCHK((launch_terms<false, true>(h, pp, target, batch, upstream_dev, gp, (hipStream_t)stream)));
    return Y355_GRAD_OK;
}

int y355_grad_flat(int32_t device_id, const void *conf_dev, const void *cls_dev, const void *txtytwth_dev, const void *label_dev, int32_t batch,
                   int32_t num_anchors_total, int32_t num_classes, double obj_weight, double noobj_weight, const void *upstream_dev,
                   void *g_conf_dev, void *g_cls_dev, void *g_txtytwth_dev, void *stream, double *out, double *per_image) {
    if (device_id < 0 || !conf_dev || !cls_dev || !txtytwth_dev || !label_dev) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: null argument");
    const int ng = (g_conf_dev ? 1 : 0) + (g_cls_dev ? 1 : 0) + (g_txtytwth_dev ? 1 : 0);
    if (ng != 0 && ng != 3) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: give all three gradient tensors or none");
    if (!out && ng == 0) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: neither out nor gradient tensors");
    if (!out && per_image) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: per_image without out");
    if (batch < 1 || batch > 65535 || num_anchors_total < 1 || num_classes < 1 || num_classes > 4096)
        return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: batch must be 1..65535, num_anchors_total >= 1, num_classes 1..4096");
    if (!std::isfinite(obj_weight) || !std::isfinite(noobj_weight)) return y355_fail(Y355_GRAD_EINVAL, "y355_grad_flat: weights must be finite");
    const int nblk = loss_nblk(num_anchors_total);
    const dim3 grid(nblk, batch), block(LOSS_THREADS);
    const float *conf = (const float *)conf_dev, *cls = (const float *)cls_dev, *box = (const float *)txtytwth_dev, *label = (const float *)label_dev;
    const float *up = (const float *)upstream_dev;
    float *gc = (float *)g_conf_dev, *gk = (float *)g_cls_dev, *gb = (float *)g_txtytwth_dev;
    const float obj_w = (float)obj_weight, noobj_w = (float)noobj_weight;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(device_id));
    if (!out) {                                                   // the gradient alone: no workspace, nothing to wait for
        hipLaunchKernelGGL((grad_flat_kernel<false, true>), grid, block, 0, s, conf, cls, box, label, num_anchors_total, num_classes, up, obj_w,
                           noobj_w, gc, gk, gb, (double *)nullptr);
        HIPCHK(hipGetLastError());
        return Y355_GRAD_OK;
    }
    double *ws = nullptr;                                         // partial [batch][nblk][5], per_image [batch][5], out [4]
    const size_t n_part = (size_t)batch * nblk * 5, n_img = (size_t)batch * 5;
    DevOwner own{y355_hip_mem(), {}};                             // no handle: the workspace lives for this call
    if (int rc = y355_dev_get(own, &ws, n_part + n_img + 4)) return rc;
    if (ng)
        hipLaunchKernelGGL((grad_flat_kernel<true, true>), grid, block, 0, s, conf, cls, box, label, num_anchors_total, num_classes, up, obj_w,
                           noobj_w, gc, gk, gb, ws);
    else
        hipLaunchKernelGGL((grad_flat_kernel<true, false>), grid, block, 0, s, conf, cls, box, label, num_anchors_total, num_classes, up, obj_w,
                           noobj_w, gc, gk, gb, ws);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = loss_finish(ws, nblk, batch, obj_weight, noobj_weight, ws + n_part, ws + n_part + n_img, s, out, per_image);
    y355_dev_release_all(own);                                    // every path from the allocation comes through here
    if (e != hipSuccess) return y355_fail(Y355_GRAD_EHIP, std::string("y355_grad_flat: ") + hipGetErrorString(e));
    return Y355_GRAD_OK;
}

}  // extern "C"
