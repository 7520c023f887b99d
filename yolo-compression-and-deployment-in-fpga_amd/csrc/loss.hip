// yolo355_loss -- the reference's training targets and the forward value of its losses on the GPU (gfx950); C ABI in
// include/yolo355_loss.h, linked into libyolo355_loss.so on its own (nothing of libyolo355.so is used).
//
//   assign_kernel       tools.gt_creator / tools.multi_gt_creator (tools.py:132-374): one wave per image walks the image's
//                       labels in list order; lane i owns anchor i of the A * levels anchors.  A slot (level, cell, anchor)
//                       is only ever written by the lane of its anchor, so the writes of successive labels to one slot are
//                       stores of ONE thread in program order: "a later write wins" needs no atomics and no sorting.
//   loss_terms_kernel   decode_boxes + tools.iou_score + the per-anchor terms of tools.loss ('mse', tools.py:377-435) in the
//                       reference's fp32 operations, masks applied by multiplication; float64 sums per lane, then per wave,
//                       then per workgroup, one partial per workgroup
//   loss_flat_kernel    the same terms on the flat tensors tools.loss itself takes (the drop-in of that signature)
//   loss_finish_kernel  the partials of an image in workgroup order, then the batch means in image order
// No floating-point atomics anywhere: every sum has one fixed order.  The arithmetic, assign_kernel and loss_finish_kernel
// live in loss_core.h, which libyolo355_grad.so (grad.hip) compiles too.
//
// Host side: y355_host.h's pieces (error return, HIPCHK, DeviceGuard, DevOwner).  Everything but the entry points of the public
// header is hidden, so that this library's y355_fail and error text stay its own in a process that also holds libyolo355.so.
#include "../../include/yolo355_loss.h"
#pragma GCC visibility push(hidden)
#include "loss_core.h"
static_assert(Y355_LOSS_OK == Y355_OK && Y355_LOSS_EINVAL == Y355_EINVAL && Y355_LOSS_EHIP == Y355_EHIP && Y355_LOSS_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_loss_last_error's text
#ifndef Y355_HOSTCHECK                                   // (host_state_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

struct y355_loss : LossState {};

// ---------------------------------------------------------------------------------------------------------- loss
__global__ __launch_bounds__(LOSS_THREADS) void loss_terms_kernel(const LossDev p, const PredPtrs pp, const float *__restrict__ target,
                                                                  double *__restrict__ partial) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int b = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
    const int A = p.A, C = p.C;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = blockIdx.x * LOSS_THREADS + tid; i < p.N; i += nblk * LOSS_THREADS) {
        const AnchorAt q = anchor_at_(p, i);
        const size_t HW = q.HW;
        const float *pm = pp.p[q.lv] + (size_t)b * A * (5 + C) * HW + q.cell;
        const float *t = target + ((size_t)b * p.N + p.base[q.lv] + (size_t)q.cell * A + q.a) * NF;
        const float conf = pm[(size_t)q.a * HW];
        const float *pc = pm + (size_t)(A + q.a * C) * HW, *pb = pm + (size_t)(A * (1 + C) + q.a * 4) * HW;
        const float tx = pb[0], ty = pb[HW], tw = pb[2 * HW], th = pb[3 * HW];
        const float iou = anchor_iou_(p, q, tx, ty, tw, th, t);
        const ClsStat st = cls_stat_<0>([pc, HW](int c) { return pc[(size_t)c * HW]; }, C, t[1]);
        float term[5];
        loss_terms_(conf, st, tx, ty, tw, th, iou, t[0], t[2], t[3], t[4], t[5], t[6], term);
        for (int k = 0; k < 5; ++k) acc[k] += (double)term[k];
    }
    block_partial(acc, s_part, partial + ((size_t)b * nblk + blockIdx.x) * 5);
}

// tools.loss on the reference's own flat tensors: conf [B][N], cls [B][N][C], txtytwth [B][N][4], label [B][N][8] = iou, obj, cls,
// tx, ty, tw, th, weight.  Same terms, same three-step sums.
__global__ __launch_bounds__(LOSS_THREADS) void loss_flat_kernel(const float *__restrict__ conf, const float *__restrict__ cls,
                                                                 const float *__restrict__ box, const float *__restrict__ label, int N, int C,
                                                                 double *__restrict__ partial) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int b = blockIdx.y, nblk = gridDim.x;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = blockIdx.x * LOSS_THREADS + threadIdx.x; n < N; n += nblk * LOSS_THREADS) {
        const size_t i = (size_t)b * N + n;
        const float *L = label + i * 8, *pb = box + i * 4, *pc = cls + i * C;
        const ClsStat st = cls_stat_<0>([pc](int c) { return pc[c]; }, C, L[2]);
        float term[5];
        loss_terms_(conf[i], st, pb[0], pb[1], pb[2], pb[3], L[0], L[1], L[3], L[4], L[5], L[6], L[7], term);
        for (int k = 0; k < 5; ++k) acc[k] += (double)term[k];
    }
    block_partial(acc, s_part, partial + ((size_t)b * nblk + blockIdx.x) * 5);
}

__global__ __launch_bounds__(LOSS_THREADS) void iou_score_kernel(const float *__restrict__ a, const float *__restrict__ g, long long n,
                                                                 float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= n) return;
    out[i] = iou_score_(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], g[4 * i], g[4 * i + 1], g[4 * i + 2], g[4 * i + 3]);
}

// ---------------------------------------------------------------------------------------------------------- the handle
// y355_loss_create in two parts, as host_state_check.cpp runs them on the CPU: the rules of a configuration and the host state
// (no device call; the handle gets its device memory from mem), ...
int loss_open(const y355_loss_config *cfg, const DevMem &mem, y355_loss **out) {
    if (!cfg || !out) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_create: null argument");
    *out = nullptr;
    y355_loss st;
    if (int rc = loss_rules(*cfg, mem, &st)) return rc;
    *out = new y355_loss(st);
    return Y355_LOSS_OK;
}
// ... and all of its device memory (on the current device), or none of it
int loss_buffers(y355_loss *h) { return loss_state_buffers(h); }
DevOwner &loss_owner(y355_loss *h) { return h->own; }      // (host_state_check.cpp does not see the struct)
void loss_free(y355_loss *h) {
    y355_dev_release_all(h->own);
    delete h;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_loss_last_error(void) { return g_err.c_str(); }

int y355_loss_default_config(y355_loss_config *cfg) {
    if (!cfg) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_default_config: null config");
    *cfg = y355_loss_config{};
    cfg->num_levels = 1;
    cfg->wh_mul = 1.0f;
    cfg->ignore_thresh = 0.5;
    cfg->obj_weight = 5.0;
    cfg->noobj_weight = 1.0;
    cfg->max_batch = 1;
    cfg->max_labels_per_image = 64;
    return Y355_LOSS_OK;
}

int y355_loss_create(const y355_loss_config *cfg, y355_loss **out) {
    if (int rc = loss_open(cfg, y355_hip_mem(), out)) return rc;
    DeviceGuard g;
    const hipError_t e = g.set(cfg->device_id);
    const int rc = e != hipSuccess ? y355_fail(Y355_LOSS_EHIP, std::string("y355_loss_create: ") + hipGetErrorString(e)) : loss_buffers(*out);
    if (rc) {
        loss_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_loss_destroy(y355_loss *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->cfg.device_id);
    loss_free(h);
}

int y355_loss_num_anchors_total(const y355_loss *h) { return h ? h->dev.N : y355_fail(Y355_LOSS_EINVAL, "null handle"); }

int y355_loss_set_labels(y355_loss *h, const int32_t *offsets, const double *labels, int32_t batch) {
    if (!h || !offsets) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_set_labels: null argument");
    return loss_set_labels("y355_loss_set_labels", h, offsets, labels, batch);
}

int y355_loss_get_targets(y355_loss *h, int32_t batch, float *dst_host) {
    if (!h || !dst_host) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_get_targets: null argument");
    if (h->labels_batch == 0) return y355_fail(Y355_LOSS_ENOTREADY, "y355_loss_get_targets: no labels set");
    if (batch < 1 || batch > h->labels_batch) return y355_fail(Y355_LOSS_EINVAL, "batch must be 1..the batch of y355_loss_set_labels");
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    HIPCHK(hipMemcpy(dst_host, h->target, (size_t)batch * h->dev.N * NF * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_LOSS_OK;
}

int y355_loss_compute(y355_loss *h, const void *const *pred_dev, const void *target_dev, int32_t batch, void *stream, double *out,
                      double *per_image) {
    if (!h || !pred_dev || !out) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_compute: null argument");
    if (batch < 1 || batch > h->cfg.max_batch) return y355_fail(Y355_LOSS_EINVAL, "batch must be 1..max_batch");
    PredPtrs pp{};
    for (int l = 0; l < h->dev.nlev; ++l) {
        if (!pred_dev[l]) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_compute: null prediction map");
        pp.p[l] = (const float *)pred_dev[l];
    }
    const float *target = nullptr;
    if (int rc = loss_pick_target("y355_loss_compute", h, target_dev, batch, &target)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    hipLaunchKernelGGL(loss_terms_kernel, dim3(h->nblk, batch), dim3(LOSS_THREADS), 0, s, h->dev, pp, target, h->partial);
    HIPCHK(hipGetLastError());
    HIPCHK(loss_finish(h->partial, h->nblk, batch, h->cfg.obj_weight, h->cfg.noobj_weight, h->per_image, h->out, s, out, per_image));
    return Y355_LOSS_OK;
}

int y355_loss_iou_score(int32_t device_id, const void *boxes_a_dev, const void *boxes_b_dev, int64_t n, void *out_dev, void *stream) {
    if (device_id < 0 || n < 0 || n > (1LL << 31) * (long long)LOSS_THREADS) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_iou_score: bad device or n");
    if (n == 0) return Y355_LOSS_OK;
    if (!boxes_a_dev || !boxes_b_dev || !out_dev) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_iou_score: null argument");
    DeviceGuard g;
    HIPCHK(g.set(device_id));
    hipLaunchKernelGGL(iou_score_kernel, dim3((unsigned)((n + LOSS_THREADS - 1) / LOSS_THREADS)), dim3(LOSS_THREADS), 0, (hipStream_t)stream,
                       (const float *)boxes_a_dev, (const float *)boxes_b_dev, (long long)n, (float *)out_dev);
    HIPCHK(hipGetLastError());
    return Y355_LOSS_OK;
}

int y355_loss_flat(int32_t device_id, const void *conf_dev, const void *cls_dev, const void *txtytwth_dev, const void *label_dev,
                   int32_t batch, int32_t num_anchors_total, int32_t num_classes, double obj_weight, double noobj_weight, void *stream,
                   double *out, double *per_image) {
    if (device_id < 0 || !conf_dev || !cls_dev || !txtytwth_dev || !label_dev || !out) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_flat: null argument");
    if (batch < 1 || batch > 65535 || num_anchors_total < 1 || num_classes < 1 || num_classes > 4096)
        return y355_fail(Y355_LOSS_EINVAL, "y355_loss_flat: batch must be 1..65535, num_anchors_total >= 1, num_classes 1..4096");
    if (!std::isfinite(obj_weight) || !std::isfinite(noobj_weight)) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_flat: weights must be finite");
    const int nblk = loss_nblk(num_anchors_total);
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(device_id));
    double *ws = nullptr;                                         // partial [batch][nblk][5], per_image [batch][5], out [4]
    const size_t n_part = (size_t)batch * nblk * 5, n_img = (size_t)batch * 5;
    DevOwner own{y355_hip_mem(), {}};                             // no handle: the workspace lives for this call
    if (int rc = y355_dev_get(own, &ws, n_part + n_img + 4)) return rc;
    hipLaunchKernelGGL(loss_flat_kernel, dim3(nblk, batch), dim3(LOSS_THREADS), 0, s, (const float *)conf_dev, (const float *)cls_dev,
                       (const float *)txtytwth_dev, (const float *)label_dev, num_anchors_total, num_classes, ws);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = loss_finish(ws, nblk, batch, obj_weight, noobj_weight, ws + n_part, ws + n_part + n_img, s, out, per_image);
    y355_dev_release_all(own);                                    // every path from the allocation comes through here
    if (e != hipSuccess) return y355_fail(Y355_LOSS_EHIP, std::string("y355_loss_flat: ") + hipGetErrorString(e));
    return Y355_LOSS_OK;
}

}  // extern "C"
