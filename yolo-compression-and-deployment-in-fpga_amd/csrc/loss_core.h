// The loss arithmetic both training libraries compile: libyolo355_loss.so (loss.hip, the value) and libyolo355_grad.so
// (grad.hip, the value and its gradient).  One home for the target assignment, the decode, the IoU that serves as the
// objectness label, the per-anchor terms, the three-step sums, the finish kernel, the rules of a configuration and the host
// side of a label upload -- so that the value the gradient library returns is the loss library's, bit for bit.
//
// Included once per library, inside its `#pragma GCC visibility push(hidden)`: every kernel and function here stays the
// including library's own.  Error texts name the entry point through `who`.
#pragma once
#include <math.h>

#include "../../include/yolo355_loss.h"
#include "y355_host.h"

#define MAXL Y355_LOSS_MAX_LEVELS
#define MAXA Y355_LOSS_MAX_ANCHORS
#define NF Y355_LOSS_TARGET_FIELDS
#define LOSS_THREADS 256
#define LOSS_WAVES (LOSS_THREADS / 64)
#define LOSS_MAX_WGS 32          // workgroups per image of the terms kernels: a function of N only, never of the batch

struct LossDev {
    int nlev, A, C, N, grid_units;
    int hs[MAXL], ws[MAXL], base[MAXL + 1];     // base[l]: first anchor index of level l; base[nlev] = N
    float stride[MAXL], anchors[2 * MAXL * MAXA];
    double stride_d[MAXL], anchors_d[2 * MAXL * MAXA];
    float in_h, in_w, wh_mul;
    double in_h_d, in_w_d, ignore_thresh;
};
struct PredPtrs {
    const float *p[MAXL];
};

// What a handle of either library holds: the configuration, its device form, and the six device arrays of a batch.
struct LossState {
    y355_loss_config cfg;
    LossDev dev;
    int nblk = 0;
    int labels_batch = 0;             // batch of the last set_labels, 0: none
    float *target = nullptr;          // [max_batch][N][11]
    double *labels = nullptr;         // [max_batch * max_labels][5]
    int *offsets = nullptr;           // [max_batch + 1]
    double *partial = nullptr;        // [max_batch][nblk][5]
    double *per_image = nullptr;      // [max_batch][5]
    double *out = nullptr;            // [4]
    DevOwner own;                     // of the six arrays above
};

// ---------------------------------------------------------------------------------------------------------- targets
__global__ __launch_bounds__(64) void assign_kernel(const LossDev p, const int *__restrict__ offsets, const double *__restrict__ labels,
                                                    float *__restrict__ target) {
    __shared__ double s_iou[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int nA = p.nlev * p.A;
    const bool mine = lane < nA;
    const int lv = mine ? lane / p.A : 0, a = lane - lv * p.A;
    const double aw = mine ? p.anchors_d[2 * lane] : 1.0, ah = mine ? p.anchors_d[2 * lane + 1] : 1.0;
    const double w = p.in_w_d, h = p.in_h_d;
    float *tb = target + (size_t)b * p.N * NF;
    const int k1 = offsets[b + 1];
    for (int k = offsets[b]; k < k1; ++k) {                       // list order: the order of writes is part of the result
        const double xmin = labels[5 * (size_t)k], ymin = labels[5 * (size_t)k + 1], xmax = labels[5 * (size_t)k + 2],
                     ymax = labels[5 * (size_t)k + 3], cls = labels[5 * (size_t)k + 4];
        const double c_x = (xmax + xmin) / 2 * w, c_y = (ymax + ymin) / 2 * h;
        const double box_w = (xmax - xmin) * w, box_h = (ymax - ymin) * h;
        if (box_w < 1. || box_h < 1.) continue;                   // same for every lane
        const double bw = p.grid_units ? box_w / p.stride_d[0] : box_w, bh = p.grid_units ? box_h / p.stride_d[0] : box_h;
        // tools.compute_iou, both boxes centred at the origin
        const double i_w = fmin(0.0 + bw / 2, 0.0 + aw / 2) - fmax(0.0 - bw / 2, 0.0 - aw / 2);
        const double i_h = fmin(0.0 + bh / 2, 0.0 + ah / 2) - fmax(0.0 - bh / 2, 0.0 - ah / 2);
        const double s_i = i_h * i_w;
        const double iou = s_i / (bw * bh + aw * ah - s_i + 1e-20);
        s_iou[lane] = mine ? iou : -1.0;
        __syncthreads();
        int best = 0;
        double bv = s_iou[0];
        for (int i = 1; i < nA; ++i)                              // np.argmax: the first maximum
            if (s_iou[i] > bv) { bv = s_iou[i]; best = i; }
        __syncthreads();
        if (!mine || !(lane == best || iou > p.ignore_thresh)) continue;
        const double s = p.stride_d[lv];
        const double c_x_s = c_x / s, c_y_s = c_y / s;
        const int gx = (int)c_x_s, gy = (int)c_y_s;
        if (gx < 0 || gy < 0 || gx >= p.ws[lv] || gy >= p.hs[lv]) continue;      // outside the grid: dropped, both kinds
        float *t = tb + ((size_t)p.base[lv] + ((size_t)gy * p.ws[lv] + gx) * p.A + a) * NF;
        if (lane == best) {
            t[0] = 1.0f;
            t[1] = (float)cls;
            t[2] = (float)(c_x_s - gx);
            t[3] = (float)(c_y_s - gy);
            t[4] = (float)log(bw / aw);
            t[5] = (float)log(bh / ah);
            t[6] = (float)(2.0 - (box_w / w) * (box_h / h));
            t[7] = (float)xmin;
            t[8] = (float)ymin;
            t[9] = (float)xmax;
            t[10] = (float)ymax;
        } else {
            t[0] = -1.0f;
            t[6] = -1.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// torch.max / torch.min hand a NaN on; fmaxf / fminf drop it
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }
__device__ __forceinline__ float min_nan(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                     // lane 0 holds the sum
}

// tools.iou_score (:377-389) of one pair of boxes
__device__ __forceinline__ float iou_score_(float x1, float y1, float x2, float y2, float g0, float g1, float g2, float g3) {
    const float tlx = max_nan(x1, g0), tly = max_nan(y1, g1), brx = min_nan(x2, g2), bry = min_nan(y2, g3);
    const float area_a = (x2 - x1) * (y2 - y1), area_b = (g2 - g0) * (g3 - g1);
    const float en = (tlx < brx ? 1.0f : 0.0f) * (tly < bry ? 1.0f : 0.0f);
    const float area_i = ((brx - tlx) * (bry - tly)) * en;
    return area_i / (area_a + area_b - area_i);
}

// Item i of an image's N anchors in the order of the terms kernels, i = base[level] + a * HW + cell: consecutive lanes walk
// consecutive cells of one channel of the NCHW map.
struct AnchorAt {
    int lv, HW, a, cell, gx, gy;
};
__device__ __forceinline__ AnchorAt anchor_at_(const LossDev &p, int i) {
    AnchorAt q;
    q.lv = (p.nlev > 1 && i >= p.base[1] ? 1 : 0) + (p.nlev > 2 && i >= p.base[2] ? 1 : 0);
    q.HW = p.hs[q.lv] * p.ws[q.lv];
    const int r = i - p.base[q.lv];
    q.a = r / q.HW;
    q.cell = r - q.a * q.HW;
    q.gy = q.cell / p.ws[q.lv];
    q.gx = q.cell - q.gy * p.ws[q.lv];
    return q;
}

// The objectness label of an anchor: decode_boxes / [w, h, w, h], no clamp (the arithmetic of decode_kernel in head_nms.hip),
// then tools.iou_score against the target's box t[7..10].  The reference takes it under no_grad: a constant of the gradient.
__device__ __forceinline__ float anchor_iou_(const LossDev &p, const AnchorAt &q, float tx, float ty, float tw, float th, const float *t) {
    const float cx = (sigmoidf_(tx) + (float)q.gx) * p.stride[q.lv];
    const float cy = (sigmoidf_(ty) + (float)q.gy) * p.stride[q.lv];
    const float bw = (expf(tw) * p.anchors[2 * (q.lv * p.A + q.a)]) * p.wh_mul;
    const float bh = (expf(th) * p.anchors[2 * (q.lv * p.A + q.a) + 1]) * p.wh_mul;
    const float x1 = (cx - bw / 2) / p.in_w, y1 = (cy - bh / 2) / p.in_h;
    const float x2 = (cx + bw / 2) / p.in_w, y2 = (cy + bh / 2) / p.in_h;
    return iou_score_(x1, y1, x2, y2, t[7], t[8], t[9], t[10]);
}

// What the cross entropy of an anchor needs of its class logits x(0) .. x(C - 1): the maximum, the sum of exp(x - max), the
// target class clamped into the map (a caller's target may hold anything: never read outside it) and its logit.
// CMAX == 0: x is read C times per pass, at run-time indices.  CMAX > 0 (C <= CMAX): the loops are unrolled to CMAX steps and
// every index is a constant, so that x may be a register array.  The operations and their order are the same.
struct ClsStat {
    float m, se, xk;
    int kc;
};
template <int CMAX, typename Logit>
__device__ __forceinline__ ClsStat cls_stat_(Logit x, int C, float t_cls) {
    ClsStat s;
    int kc = (int)t_cls;
    kc = kc < 0 ? 0 : (kc >= C ? C - 1 : kc);
    s.kc = kc;
    float m = x(0), se = 0.0f;
    if constexpr (CMAX == 0) {
        for (int c = 1; c < C; ++c) m = fmaxf(m, x(c));
        for (int c = 0; c < C; ++c) se += expf(x(c) - m);
        s.xk = x(kc);
    } else {
        float xk = x(0);
#pragma unroll
        for (int c = 1; c < CMAX; ++c)
            if (c < C) {
                m = fmaxf(m, x(c));
                xk = c == kc ? x(c) : xk;
            }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) se += expf(x(c) - m);
        s.xk = xk;
    }
    s.m = m;
    s.se = se;
    return s;
}

// The five terms of one anchor, tools.loss (:392-435) with MSELoss (:27-42): masks by multiplication, so a non-finite term at
// a masked anchor poisons the sum as it does there.  st: cls_stat_ of the anchor's class logits.
__device__ __forceinline__ void loss_terms_(float conf, const ClsStat &st, float tx, float ty, float tw, float th, float iou, float t_obj,
                                            float t_tx, float t_ty, float t_tw, float t_th, float t_wt, float *term) {
    const float pconf = sigmoidf_(conf);
    const float d = pconf - iou;
    term[0] = (t_obj == 1.0f ? 1.0f : 0.0f) * (d * d);
    term[1] = (t_obj == 0.0f ? 1.0f : 0.0f) * (pconf * pconf);
    const float mask = t_wt > 0.0f ? 1.0f : 0.0f;
    term[2] = (logf(st.se) - (st.xk - st.m)) * mask;
    const float bx = (1.0f - t_tx) * tx + (fmaxf(-tx, 0.0f) + log1pf(expf(-fabsf(tx))));
    const float by = (1.0f - t_ty) * ty + (fmaxf(-ty, 0.0f) + log1pf(expf(-fabsf(ty))));
    term[3] = ((bx + by) * t_wt) * mask;
    const float ew = tw - t_tw, eh = th - t_th;
    term[4] = ((ew * ew + eh * eh) * t_wt) * mask;
}

// lane sums -> wave sums -> the workgroup's partial [5]
__device__ __forceinline__ void block_partial(const double *acc, double (*s_part)[5], double *dst) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        double v = s_part[0][threadIdx.x];
        for (int wv = 1; wv < LOSS_WAVES; ++wv) v += s_part[wv][threadIdx.x];
        dst[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const double *__restrict__ partial, int nblk, int batch, double obj_w,
                                                                   double noobj_w, double *per_image, double *out) {
    __shared__ double s_mean[5];
    for (int i = threadIdx.x; i < batch * 5; i += LOSS_THREADS) {          // (image, part): the image's workgroups in order
        const int b = i / 5, k = i - b * 5;
        double v = 0.0;
        for (int j = 0; j < nblk; ++j) v += partial[((size_t)b * nblk + j) * 5 + k];
        per_image[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5) {                                                 // batch mean, images in order
        double v = 0.0;
        for (int b = 0; b < batch; ++b) v += per_image[b * 5 + threadIdx.x];
        s_mean[threadIdx.x] = v / batch;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double conf = obj_w * s_mean[0] + noobj_w * s_mean[1];
        const double box = s_mean[3] + s_mean[4];
        out[0] = conf;
        out[1] = s_mean[2];
        out[2] = box;
        out[3] = conf + s_mean[2] + box;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// workgroups per image of a terms kernel
inline int loss_nblk(long long N) {
    const long long n = (N + LOSS_THREADS - 1) / LOSS_THREADS;
    return (int)(n > LOSS_MAX_WGS ? LOSS_MAX_WGS : n);
}

// The rules of a configuration and, when it passes, the host state it gives (no device call): cfg, dev, nblk and the owner's
// allocator.
inline int loss_rules(const y355_loss_config &c, const DevMem &mem, LossState *st) {
    if (c.device_id < 0) return y355_fail(Y355_LOSS_EINVAL, "device_id < 0");
    if (c.num_levels < 1 || c.num_levels > MAXL) return y355_fail(Y355_LOSS_EINVAL, "num_levels must be 1..3");
    if (c.num_anchors < 1 || c.num_anchors > MAXA) return y355_fail(Y355_LOSS_EINVAL, "num_anchors must be 1..16 per level");
    if (c.num_classes < 1 || c.num_classes > 4096) return y355_fail(Y355_LOSS_EINVAL, "num_classes must be 1..4096");
    if (c.in_h < 1 || c.in_w < 1 || c.in_h > 65536 || c.in_w > 65536) return y355_fail(Y355_LOSS_EINVAL, "in_h / in_w must be 1..65536");
    if (!(c.wh_mul > 0.0f) || !std::isfinite(c.wh_mul)) return y355_fail(Y355_LOSS_EINVAL, "wh_mul must be finite and > 0");
    if (c.anchors_in_grid_units && c.num_levels != 1)
        return y355_fail(Y355_LOSS_EINVAL, "anchors_in_grid_units is gt_creator's form: one level only");
    if (!std::isfinite(c.ignore_thresh) || !std::isfinite(c.obj_weight) || !std::isfinite(c.noobj_weight))
        return y355_fail(Y355_LOSS_EINVAL, "ignore_thresh / obj_weight / noobj_weight must be finite");
    if (c.max_batch < 1 || c.max_batch > 65535) return y355_fail(Y355_LOSS_EINVAL, "max_batch must be 1..65535");
    if (c.max_labels_per_image < 1 || c.max_labels_per_image > (1 << 20)) return y355_fail(Y355_LOSS_EINVAL, "max_labels_per_image must be 1..2^20");
    long long N = 0;
    for (int l = 0; l < c.num_levels; ++l) {
        if (c.hs[l] < 1 || c.ws[l] < 1 || c.hs[l] > 4096 || c.ws[l] > 4096) return y355_fail(Y355_LOSS_EINVAL, "hs / ws must be 1..4096");
        if (c.stride[l] < 1) return y355_fail(Y355_LOSS_EINVAL, "stride must be >= 1");
        N += (long long)c.hs[l] * c.ws[l] * c.num_anchors;
    }
    for (int i = 0; i < 2 * c.num_levels * c.num_anchors; ++i)
        if (!(c.anchors[i] > 0.0) || !std::isfinite(c.anchors[i])) return y355_fail(Y355_LOSS_EINVAL, "anchor sizes must be finite and > 0");
    if (N * (5 + (long long)c.num_classes) > 0x7fffffffLL) return y355_fail(Y355_LOSS_EINVAL, "prediction maps of an image exceed 2^31 elements");
    if ((long long)c.max_batch * c.max_labels_per_image > (1LL << 26)) return y355_fail(Y355_LOSS_EINVAL, "max_batch * max_labels_per_image exceeds 2^26");

    st->cfg = c;
    st->own.mem = mem;
    LossDev &d = st->dev;
    d = LossDev{};
    d.nlev = c.num_levels; d.A = c.num_anchors; d.C = c.num_classes; d.N = (int)N; d.grid_units = c.anchors_in_grid_units ? 1 : 0;
    int base = 0;
    for (int l = 0; l < c.num_levels; ++l) {
        d.hs[l] = c.hs[l]; d.ws[l] = c.ws[l]; d.base[l] = base;
        d.stride[l] = (float)c.stride[l]; d.stride_d[l] = (double)c.stride[l];
        base += c.hs[l] * c.ws[l] * c.num_anchors;
    }
    for (int l = c.num_levels; l <= MAXL; ++l) d.base[l] = base;
    for (int i = 0; i < 2 * c.num_levels * c.num_anchors; ++i) { d.anchors_d[i] = c.anchors[i]; d.anchors[i] = (float)c.anchors[i]; }
    d.in_h = (float)c.in_h; d.in_w = (float)c.in_w; d.in_h_d = c.in_h; d.in_w_d = c.in_w;
    d.wh_mul = c.wh_mul; d.ignore_thresh = c.ignore_thresh;
    st->nblk = loss_nblk(N);
    return Y355_LOSS_OK;
}

// all of a state's device memory (on the current device), or none of it
inline int loss_state_buffers(LossState *st) {
    const size_t mb = (size_t)st->cfg.max_batch;
    DevOwner &o = st->own;
    int rc = y355_dev_get(o, &st->target, mb * st->dev.N * NF);
    rc = rc ? rc : y355_dev_get(o, &st->labels, mb * st->cfg.max_labels_per_image * 5);
    rc = rc ? rc : y355_dev_get(o, &st->offsets, mb + 1);
    rc = rc ? rc : y355_dev_get(o, &st->partial, mb * st->nblk * 5);
    rc = rc ? rc : y355_dev_get(o, &st->per_image, mb * 5);
    rc = rc ? rc : y355_dev_get(o, &st->out, 4);
    if (rc) y355_dev_release_all(o);
    return rc;
}

// y355_*_set_labels behind its null check: the label rules on the host, then the upload and the target assignment.  Synchronous.
inline int loss_set_labels(const std::string &who, LossState *st, const int32_t *offsets, const double *labels, int32_t batch) {
    if (batch < 1 || batch > st->cfg.max_batch) return y355_fail(Y355_LOSS_EINVAL, "batch must be 1..max_batch");
    if (offsets[0] != 0) return y355_fail(Y355_LOSS_EINVAL, "offsets[0] must be 0");
    for (int b = 0; b < batch; ++b) {
        const long long n = (long long)offsets[b + 1] - offsets[b];
        if (n < 0) return y355_fail(Y355_LOSS_EINVAL, "offsets must not decrease");
        if (n > st->cfg.max_labels_per_image)
            return y355_fail(Y355_LOSS_EINVAL, "image " + std::to_string(b) + " has " + std::to_string(n) + " labels, max_labels_per_image is " +
                                              std::to_string(st->cfg.max_labels_per_image));
    }
    const int n = offsets[batch];
    if (n > 0 && !labels) return y355_fail(Y355_LOSS_EINVAL, who + ": null labels");
    std::vector<double> host((size_t)n * 5);
    for (int k = 0; k < n; ++k) {
        const double *L = labels + 5 * (size_t)k;
        for (int j = 0; j < 5; ++j)
            if (!std::isfinite(L[j])) return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": non-finite value");
        for (int j = 0; j < 4; ++j)
            if (L[j] < 0.0 || L[j] > 1.0) return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": coordinate outside [0, 1]");
        if (L[4] < 0.0 || L[4] >= (double)st->cfg.num_classes)
            return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": class outside 0.." + std::to_string(st->cfg.num_classes - 1));
        for (int j = 0; j < 4; ++j) host[5 * (size_t)k + j] = L[j];
        host[5 * (size_t)k + 4] = (double)(int)L[4];              // int(gt_label[-1])
    }
    st->labels_batch = 0;
    DeviceGuard g;
    HIPCHK(g.set(st->cfg.device_id));
    HIPCHK(hipMemcpy(st->offsets, offsets, ((size_t)batch + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n > 0) HIPCHK(hipMemcpy(st->labels, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(st->target, 0, (size_t)batch * st->dev.N * NF * sizeof(float), nullptr));
    hipLaunchKernelGGL(assign_kernel, dim3(batch), dim3(64), 0, nullptr, st->dev, st->offsets, st->labels, st->target);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    st->labels_batch = batch;
    return Y355_LOSS_OK;
}

// the target a compute call reads: the caller's, or the handle's own when its labels were set for this batch
inline int loss_pick_target(const std::string &who, const LossState *st, const void *target_dev, int32_t batch, const float **target) {
    if (!target_dev) {
        if (st->labels_batch == 0) return y355_fail(Y355_LOSS_ENOTREADY, who + ": no labels set and no target given");
        if (st->labels_batch != batch)
            return y355_fail(Y355_LOSS_ENOTREADY, who + ": labels were set for a batch of " + std::to_string(st->labels_batch) + ", not " +
                                                 std::to_string(batch));
    }
    *target = target_dev ? (const float *)target_dev : st->target;
    return Y355_LOSS_OK;
}

// After a terms kernel on s: the finish kernel over partial [batch][nblk][5], the four losses and (per_image != NULL) the parts
// to the host; returns when s has finished.  The caller has set the device.
inline hipError_t loss_finish(const double *partial, int nblk, int batch, double obj_w, double noobj_w, double *per_image_dev, double *out_dev,
                              hipStream_t s, double *out, double *per_image) {
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, partial, nblk, batch, obj_w, noobj_w, per_image_dev, out_dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, out_dev, 4 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && per_image) e = hipMemcpyAsync(per_image, per_image_dev, (size_t)batch * 5 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}
