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
// No floating-point atomics anywhere: every sum has one fixed order.
//
// Host side: y355_host.h's pieces (error return, HIPCHK, DeviceGuard, DevOwner).  Everything but the entry points of the public
// header is hidden, so that this library's y355_fail and error text stay its own in a process that also holds libyolo355.so.
#include <math.h>

#include "../../include/yolo355_loss.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_LOSS_OK == Y355_OK && Y355_LOSS_EINVAL == Y355_EINVAL && Y355_LOSS_EHIP == Y355_EHIP && Y355_LOSS_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

#define MAXL Y355_LOSS_MAX_LEVELS
#define MAXA Y355_LOSS_MAX_ANCHORS
#define NF Y355_LOSS_TARGET_FIELDS
#define LOSS_THREADS 256
#define LOSS_WAVES (LOSS_THREADS / 64)
#define LOSS_MAX_WGS 32          // workgroups per image of loss_terms_kernel: a function of N only, never of the batch

static thread_local std::string g_err;                  // y355_loss_last_error's text
#ifndef Y355_HOSTCHECK                                   // (host_state_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

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

struct y355_loss {
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

// The five terms of one anchor, tools.loss (:392-435) with MSELoss (:27-42): masks by multiplication, so a non-finite term at
// a masked anchor poisons the sum as it does there.  pc: the anchor's class logits, cs elements apart.
__device__ __forceinline__ void loss_terms_(float conf, const float *pc, size_t cs, int C, float tx, float ty, float tw, float th, float iou,
                                            float t_obj, float t_cls, float t_tx, float t_ty, float t_tw, float t_th, float t_wt,
                                            float *term) {
    const float pconf = sigmoidf_(conf);
    const float d = pconf - iou;
    term[0] = (t_obj == 1.0f ? 1.0f : 0.0f) * (d * d);
    term[1] = (t_obj == 0.0f ? 1.0f : 0.0f) * (pconf * pconf);
    const float mask = t_wt > 0.0f ? 1.0f : 0.0f;
    float m = pc[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, pc[(size_t)c * cs]);
    float se = 0.0f;
    for (int c = 0; c < C; ++c) se += expf(pc[(size_t)c * cs] - m);
    int kc = (int)t_cls;                                          // a caller's target may hold anything: never read outside the map
    kc = kc < 0 ? 0 : (kc >= C ? C - 1 : kc);
    term[2] = (logf(se) - (pc[(size_t)kc * cs] - m)) * mask;
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

__global__ __launch_bounds__(LOSS_THREADS) void loss_terms_kernel(const LossDev p, const PredPtrs pp, const float *__restrict__ target,
                                                                  double *__restrict__ partial) {
    __shared__ double s_part[LOSS_WAVES][5];
    const int b = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
    const int A = p.A, C = p.C;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // item i = base[level] + a * HW + cell: consecutive lanes read consecutive cells of one channel of the NCHW map
    for (int i = blockIdx.x * LOSS_THREADS + tid; i < p.N; i += nblk * LOSS_THREADS) {
        const int lv = (p.nlev > 1 && i >= p.base[1] ? 1 : 0) + (p.nlev > 2 && i >= p.base[2] ? 1 : 0);
        const int HW = p.hs[lv] * p.ws[lv], r = i - p.base[lv];
        const int a = r / HW, cell = r - a * HW;
        const int gy = cell / p.ws[lv], gx = cell - gy * p.ws[lv];
        const float *pm = pp.p[lv] + (size_t)b * A * (5 + C) * HW + cell;
        const float *t = target + ((size_t)b * p.N + p.base[lv] + (size_t)cell * A + a) * NF;
        const float conf = pm[(size_t)a * HW];
        const float *pc = pm + (size_t)(A + a * C) * HW, *pb = pm + (size_t)(A * (1 + C) + a * 4) * HW;
        const float tx = pb[0], ty = pb[HW], tw = pb[2 * (size_t)HW], th = pb[3 * (size_t)HW];
        // decode_boxes / [w, h, w, h], no clamp (the arithmetic of decode_kernel in head_nms.hip)
        const float cx = (sigmoidf_(tx) + (float)gx) * p.stride[lv];
        const float cy = (sigmoidf_(ty) + (float)gy) * p.stride[lv];
        const float bw = (expf(tw) * p.anchors[2 * (lv * A + a)]) * p.wh_mul;
        const float bh = (expf(th) * p.anchors[2 * (lv * A + a) + 1]) * p.wh_mul;
        const float x1 = (cx - bw / 2) / p.in_w, y1 = (cy - bh / 2) / p.in_h;
        const float x2 = (cx + bw / 2) / p.in_w, y2 = (cy + bh / 2) / p.in_h;
        const float iou = iou_score_(x1, y1, x2, y2, t[7], t[8], t[9], t[10]);
        float term[5];
        loss_terms_(conf, pc, HW, C, tx, ty, tw, th, iou, t[0], t[1], t[2], t[3], t[4], t[5], t[6], term);
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
        const float *L = label + i * 8, *pb = box + i * 4;
        float term[5];
        loss_terms_(conf[i], cls + i * C, 1, C, pb[0], pb[1], pb[2], pb[3], L[0], L[1], L[2], L[3], L[4], L[5], L[6], L[7], term);
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

// ---------------------------------------------------------------------------------------------------------- the handle
// y355_loss_create in two parts, as host_state_check.cpp runs them on the CPU: the rules of a configuration and the host state
// (no device call; the handle gets its device memory from mem), ...
int loss_open(const y355_loss_config *cfg, const DevMem &mem, y355_loss **out) {
    if (!cfg || !out) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_create: null argument");
    *out = nullptr;
    const y355_loss_config &c = *cfg;
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

    y355_loss *h = new y355_loss();
    h->cfg = c;
    h->own.mem = mem;
    LossDev &d = h->dev;
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
    h->nblk = (int)((N + LOSS_THREADS - 1) / LOSS_THREADS);
    if (h->nblk > LOSS_MAX_WGS) h->nblk = LOSS_MAX_WGS;
    *out = h;
    return Y355_LOSS_OK;
}
// ... and all of its device memory (on the current device), or none of it
int loss_buffers(y355_loss *h) {
    const size_t mb = (size_t)h->cfg.max_batch;
    DevOwner &o = h->own;
    int rc = y355_dev_get(o, &h->target, mb * h->dev.N * NF);
    rc = rc ? rc : y355_dev_get(o, &h->labels, mb * h->cfg.max_labels_per_image * 5);
    rc = rc ? rc : y355_dev_get(o, &h->offsets, mb + 1);
    rc = rc ? rc : y355_dev_get(o, &h->partial, mb * h->nblk * 5);
    rc = rc ? rc : y355_dev_get(o, &h->per_image, mb * 5);
    rc = rc ? rc : y355_dev_get(o, &h->out, 4);
    if (rc) y355_dev_release_all(o);
    return rc;
}
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
    if (batch < 1 || batch > h->cfg.max_batch) return y355_fail(Y355_LOSS_EINVAL, "batch must be 1..max_batch");
    if (offsets[0] != 0) return y355_fail(Y355_LOSS_EINVAL, "offsets[0] must be 0");
    for (int b = 0; b < batch; ++b) {
        const long long n = (long long)offsets[b + 1] - offsets[b];
        if (n < 0) return y355_fail(Y355_LOSS_EINVAL, "offsets must not decrease");
        if (n > h->cfg.max_labels_per_image)
            return y355_fail(Y355_LOSS_EINVAL, "image " + std::to_string(b) + " has " + std::to_string(n) + " labels, max_labels_per_image is " +
                                              std::to_string(h->cfg.max_labels_per_image));
    }
    const int n = offsets[batch];
    if (n > 0 && !labels) return y355_fail(Y355_LOSS_EINVAL, "y355_loss_set_labels: null labels");
    std::vector<double> host((size_t)n * 5);
    for (int k = 0; k < n; ++k) {
        const double *L = labels + 5 * (size_t)k;
        for (int j = 0; j < 5; ++j)
            if (!std::isfinite(L[j])) return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": non-finite value");
        for (int j = 0; j < 4; ++j)
            if (L[j] < 0.0 || L[j] > 1.0) return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": coordinate outside [0, 1]");
        if (L[4] < 0.0 || L[4] >= (double)h->cfg.num_classes)
            return y355_fail(Y355_LOSS_EINVAL, "label " + std::to_string(k) + ": class outside 0.." + std::to_string(h->cfg.num_classes - 1));
        for (int j = 0; j < 4; ++j) host[5 * (size_t)k + j] = L[j];
        host[5 * (size_t)k + 4] = (double)(int)L[4];              // int(gt_label[-1])
    }
    h->labels_batch = 0;
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    HIPCHK(hipMemcpy(h->offsets, offsets, ((size_t)batch + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (n > 0) HIPCHK(hipMemcpy(h->labels, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(h->target, 0, (size_t)batch * h->dev.N * NF * sizeof(float), nullptr));
    hipLaunchKernelGGL(assign_kernel, dim3(batch), dim3(64), 0, nullptr, h->dev, h->offsets, h->labels, h->target);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    h->labels_batch = batch;
    return Y355_LOSS_OK;
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
    if (!target_dev) {
        if (h->labels_batch == 0) return y355_fail(Y355_LOSS_ENOTREADY, "y355_loss_compute: no labels set and no target given");
        if (h->labels_batch != batch)
            return y355_fail(Y355_LOSS_ENOTREADY, "y355_loss_compute: labels were set for a batch of " + std::to_string(h->labels_batch) + ", not " +
                                                 std::to_string(batch));
    }
    const float *target = target_dev ? (const float *)target_dev : h->target;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->cfg.device_id));
    hipLaunchKernelGGL(loss_terms_kernel, dim3(h->nblk, batch), dim3(LOSS_THREADS), 0, s, h->dev, pp, target, h->partial);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, h->partial, h->nblk, batch, h->cfg.obj_weight,
                       h->cfg.noobj_weight, h->per_image, h->out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->out, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (per_image) HIPCHK(hipMemcpyAsync(per_image, h->per_image, (size_t)batch * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
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
    int nblk = (num_anchors_total + LOSS_THREADS - 1) / LOSS_THREADS;
    if (nblk > LOSS_MAX_WGS) nblk = LOSS_MAX_WGS;
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
    if (e == hipSuccess) {
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, s, ws, nblk, batch, obj_weight, noobj_weight, ws + n_part,
                           ws + n_part + n_img);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, ws + n_part + n_img, 4 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && per_image) e = hipMemcpyAsync(per_image, ws + n_part, n_img * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    y355_dev_release_all(own);                                    // every path from the allocation comes through here
    if (e != hipSuccess) return y355_fail(Y355_LOSS_EHIP, std::string("y355_loss_flat: ") + hipGetErrorString(e));
    return Y355_LOSS_OK;
}

}  // extern "C"
