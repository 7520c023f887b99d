// yolo355_anchors -- anchor boxes fitted to a data set on the GPU (gfx950): the reference's generate_ab_kmeans.py (k-means++ and
// Lloyd iterations under 1 - IoU, float64) with R restarts side by side; C ABI in include/yolo355_anchors.h, linked into
// libyolo355_anchors.so on its own (nothing of libyolo355.so is used).
//
//   init_kernel        the first centroid of every restart (k-means++) or all of them (given indices)
//   pp_dist_kernel     one workgroup per (chunk, restart): D = min over the chosen centroids of 1 - IoU, the chunk's total
//   pp_select_kernel   one workgroup per restart: the chunks' totals in order, thresh, the pick (the header states the scan)
//   assign_kernel      one workgroup per chunk of boxes, every box read once and held against all R * k centroids (LDS): argmin
//                      by the reference's rules, the groups, and per (restart, cluster) the chunk's partial (sum w, sum h,
//                      count) and loss
//   update_kernel      one workgroup per restart: the partials in chunk order, new centroids, loss, step count, stop rule
//   assign_kernel<true>, score_finish_kernel   the same arithmetic for one given anchor set: the IoU with the chosen anchor
//                      instead of the distance, then its mean and the counts
// Nothing is handed from one workgroup to another inside a launch: the kernel boundary orders assign -> update -> assign.  Both
// read done[r] first, so a finished restart costs nothing and keeps its result.  No floating-point atomics: every sum has one
// fixed order, written down in the header.
//
// Host side: y355_host.h's pieces (error return, HIPCHK, DeviceGuard, DevOwner).  Everything but the entry points of the public
// header is hidden, so that this library's y355_fail and error text stay its own in a process that also holds libyolo355.so.
#include <math.h>

#include "../../include/yolo355_anchors.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_ANCHORS_OK == Y355_OK && Y355_ANCHORS_EINVAL == Y355_EINVAL && Y355_ANCHORS_EHIP == Y355_EHIP &&
                  Y355_ANCHORS_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

#define CHUNK Y355_ANCHORS_CHUNK
#define MAXK Y355_ANCHORS_MAX_K
#define MAXR Y355_ANCHORS_MAX_RESTARTS
#define THREADS 256
#define WAVES (THREADS / 64)
#define PER_THREAD (CHUNK / THREADS)
#define NV (3 * MAXK + 1)          // values of a partial: (sum w, sum h, count) per cluster, then the loss
#define V_LOSS (3 * MAXK)
#define TILE 128                   // chunks staged in LDS per pass of a sum in chunk order
#define TILE_LD (TILE + 1)         // row pitch: thread v walks row v, the odd pitch spreads the rows over the banks
#define STAGE ((NV + THREADS / TILE - 1) / (THREADS / TILE))   // values a thread stages per tile
#define PP_TILE 1024
#define QUEUE_GROUP 8              // iterations queued between two reads of the done words
static_assert(PER_THREAD == 4 && CHUNK == THREADS * PER_THREAD, "the header documents four boxes per thread");

static thread_local std::string g_err;                  // y355_anchors_last_error's text
#ifndef Y355_HOSTCHECK                                   // (host_state_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

struct y355_anchors {
    int device_id = 0, max_restarts = 0, max_k = 0;
    int64_t max_boxes = 0;
    int n = 0, nchunks = 0, chunks_cap = 0;
    int fit_k = 0, fit_r = 0;          // 0: no fit made on the boxes held
    double *boxes = nullptr;           // [max_boxes][2]
    uint8_t *groups = nullptr;         // [max_restarts][max_boxes]
    uint8_t *score_idx = nullptr;      // [max_boxes]
    double *partial = nullptr;         // [max_restarts][NV][chunks_cap]
    double *cent = nullptr;            // [max_restarts][MAXK][2]
    double *init = nullptr;            // the same, as the iterations found it
    double *loss = nullptr, *old_loss = nullptr;   // [max_restarts]
    double *u = nullptr;               // [max_restarts][MAXK - 1]
    double *score_anchors = nullptr;   // [MAXK][2]: the anchor set of a y355_anchors_score
    double *score_out = nullptr;       // [1 + MAXK]: mean IoU, counts
    int *iters = nullptr, *done = nullptr, *nfound = nullptr, *first = nullptr;   // [max_restarts]
    int *counts = nullptr, *init_index = nullptr;  // [max_restarts][MAXK]
    int *flag = nullptr;               // [1]
    DevOwner own;                      // of every array above
};

// ------------------------------------------------------------------------------------------------------ device helpers
// iou(), generate_ab_kmeans.py:27-47, both boxes centred at 0
__device__ __forceinline__ double iou_(double w1, double h1, double w2, double h2) {
    const double S_1 = w1 * h1, S_2 = w2 * h2;
    const double xmin_1 = 0.0 - w1 / 2, ymin_1 = 0.0 - h1 / 2, xmax_1 = 0.0 + w1 / 2, ymax_1 = 0.0 + h1 / 2;
    const double xmin_2 = 0.0 - w2 / 2, ymin_2 = 0.0 - h2 / 2, xmax_2 = 0.0 + w2 / 2, ymax_2 = 0.0 + h2 / 2;
    const double I_w = fmin(xmax_1, xmax_2) - fmax(xmin_1, xmin_2);
    const double I_h = fmin(ymax_1, ymax_2) - fmax(ymin_1, ymin_2);
    if (I_w < 0 || I_h < 0) return 0.0;
    const double I = I_w * I_h;
    return I / (S_1 + S_2 - I);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                                     // lane 0 holds the sum
}

// Value v of one restart's partials, the chunks in order: the workgroup stages TILE chunks of every value, thread v adds them.
__device__ __forceinline__ void sum_chunks(const double *__restrict__ part, int pitch, int nchunks, int k, double *s_tile, double *s_sum) {
    const int tid = threadIdx.x;
    const bool mine = tid < 3 * k || tid == V_LOSS;
    double acc = 0.0;
    for (int base = 0; base < nchunks; base += TILE) {
        const int m = nchunks - base < TILE ? nchunks - base : TILE;
        // a thread stages one chunk of every other value; all its loads are issued before the first is used
        const int c0 = tid % TILE, v0 = tid / TILE;
        double tmp[STAGE];
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            const int v = v0 + i * (THREADS / TILE);
            tmp[i] = (v < 3 * k || v == V_LOSS) && c0 < m ? part[(size_t)v * pitch + base + c0] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < STAGE; ++i) {
            const int v = v0 + i * (THREADS / TILE);
            if (v < NV) s_tile[v * TILE_LD + c0] = tmp[i];
        }
        __syncthreads();
        if (mine) {
#pragma unroll 8
            for (int c = 0; c < m; ++c) acc += s_tile[tid * TILE_LD + c];     // in chunk order, whatever the unrolling
        }
        __syncthreads();
    }
    if (mine) s_sum[tid] = acc;
    __syncthreads();
}

// k-means++: D of the thread's four consecutive boxes of `chunk` against the m chosen centroids c[m][2]; l[j]: the thread's
// running sum, s_tot[thread]: its total.  A box past n adds +0.0.
__device__ __forceinline__ void pp_chunk(const double *__restrict__ boxes, int n, int chunk, const double *c, int m, double *l, double *s_tot) {
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = chunk * CHUNK + PER_THREAD * (int)threadIdx.x + j;
        double D = 0.0;
        if (i < n) {
            const double w = boxes[2 * (size_t)i], h = boxes[2 * (size_t)i + 1];
            double md = 1.0;
            for (int q = 0; q < m; ++q) {
                const double d = 1.0 - iou_(w, h, c[2 * q], c[2 * q + 1]);
                if (d < md) md = d;
            }
            D = md;
        }
        run += D;
        l[j] = run;
    }
    s_tot[threadIdx.x] = run;
}

// ------------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(THREADS) void check_boxes_kernel(const double *__restrict__ boxes, long long n2, int *flag) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n2) return;
    const double v = boxes[i];
    if (!(v > 0.0) || !(v <= 1.7976931348623157e308)) atomicOr(flag, 1);
}

__global__ __launch_bounds__(64) void init_kernel(const double *__restrict__ boxes, int k, int R, const int *__restrict__ first,
                                                  const int *__restrict__ init_index, int use_index, double *cent, int *nfound, int *iters,
                                                  int *done, int *counts, double *loss, double *old_loss) {
    const int r = threadIdx.x;
    if (r >= R) return;
    for (int c = 0; c < MAXK; ++c) {
        double w = 0.0, h = 0.0;
        if (use_index ? c < k : c == 0) {
            const int i = use_index ? init_index[r * MAXK + c] : first[r];
            w = boxes[2 * (size_t)i];
            h = boxes[2 * (size_t)i + 1];
        }
        cent[(r * MAXK + c) * 2] = w;
        cent[(r * MAXK + c) * 2 + 1] = h;
        counts[r * MAXK + c] = 0;
    }
    nfound[r] = use_index ? k : 1;
    iters[r] = 0;
    done[r] = 0;
    loss[r] = 0.0;
    old_loss[r] = 0.0;
}

__global__ __launch_bounds__(THREADS) void pp_dist_kernel(const double *__restrict__ boxes, int n, const double *__restrict__ cent,
                                                          const int *__restrict__ nfound, double *__restrict__ part, int pitch) {
    __shared__ double s_c[2 * MAXK], s_tot[THREADS];
    const int chunk = blockIdx.x, r = blockIdx.y, m = nfound[r];
    if (threadIdx.x < 2 * MAXK) s_c[threadIdx.x] = cent[r * MAXK * 2 + threadIdx.x];
    __syncthreads();
    double l[PER_THREAD];
    pp_chunk(boxes, n, chunk, s_c, m, l, s_tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int t = 0; t < THREADS; ++t) S += s_tot[t];
        part[(size_t)r * NV * pitch + chunk] = S;
    }
}

__global__ __launch_bounds__(THREADS) void pp_select_kernel(const double *__restrict__ boxes, int n, int nchunks, int pick,
                                                            const double *__restrict__ u, double *cent, int *nfound,
                                                            const double *__restrict__ part, int pitch) {
    __shared__ double s_tile[PP_TILE], s_l[PER_THREAD][THREADS], s_tot[THREADS], s_c[2 * MAXK], s_P[2];
    __shared__ int s_found;
    const int r = blockIdx.x, tid = threadIdx.x, m = nfound[r];
    const double *tot = part + (size_t)r * NV * pitch;
    if (tid < 2 * MAXK) s_c[tid] = cent[r * MAXK * 2 + tid];
    double P = 0.0, thresh = 0.0, Pc = 0.0;
    int found = -1;
    for (int pass = 0; pass < 2; ++pass) {                        // 0: the total; 1: the first chunk whose prefix exceeds thresh
        P = 0.0;
        for (int base = 0; base < nchunks; base += PP_TILE) {
            const int cnt = nchunks - base < PP_TILE ? nchunks - base : PP_TILE;
            for (int i = tid; i < cnt; i += THREADS) s_tile[i] = tot[base + i];
            __syncthreads();
            if (tid == 0)
                for (int c = 0; c < cnt && found < 0; ++c) {
                    if (pass == 1 && P + s_tile[c] > thresh) {
                        found = base + c;
                        Pc = P;
                    } else {
                        P += s_tile[c];
                    }
                }
            __syncthreads();
        }
        if (pass == 0) thresh = P * u[r * (MAXK - 1) + pick];
    }
    if (tid == 0) {
        s_found = found;
        s_P[0] = Pc;
        s_P[1] = thresh;
    }
    __syncthreads();
    found = s_found;
    if (found < 0) return;                                        // no prefix exceeds thresh: nothing is appended
    double l[PER_THREAD];
    pp_chunk(boxes, n, found, s_c, m, l, s_tot);
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) s_l[j][tid] = l[j];
    __syncthreads();
    if (tid == 0 && m < MAXK) {
        Pc = s_P[0];
        thresh = s_P[1];
        double S = 0.0;
        long long at = -1;
        for (int t = 0; t < THREADS && at < 0; ++t) {
            if (Pc + (S + s_tot[t]) > thresh) {
                for (int j = 0; j < PER_THREAD && at < 0; ++j)
                    if (Pc + (S + s_l[j][t]) > thresh) at = (long long)found * CHUNK + PER_THREAD * t + j;
            } else {
                S += s_tot[t];
            }
        }
        if (at >= 0 && at < n) {
            cent[(r * MAXK + m) * 2] = boxes[2 * (size_t)at];
            cent[(r * MAXK + m) * 2 + 1] = boxes[2 * (size_t)at + 1];
            nfound[r] = m + 1;
        }
    }
}

// SCORE: one given anchor set (R = 1, never done), the value summed is the IoU with the chosen anchor instead of the distance
template <bool SCORE>
__global__ __launch_bounds__(THREADS) void assign_kernel(const double *__restrict__ boxes, int n, int k, int R, const int *__restrict__ done,
                                                         const double *__restrict__ cent, double *__restrict__ part, int pitch,
                                                         uint8_t *__restrict__ groups, size_t gpitch) {
    __shared__ double s_c[MAXR * MAXK * 2];
    __shared__ double s_red[WAVES][NV];
    __shared__ int s_done[MAXR];
    const int tid = threadIdx.x, chunk = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < R * MAXK * 2; i += THREADS) s_c[i] = cent[i];
    if (tid < R) s_done[tid] = SCORE ? 0 : done[tid];
    double w[PER_THREAD], h[PER_THREAD];
    bool valid[PER_THREAD];
#pragma unroll
    for (int j = 0; j < PER_THREAD; ++j) {
        const int i = chunk * CHUNK + j * THREADS + tid;
        valid[j] = i < n;
        w[j] = valid[j] ? boxes[2 * (size_t)i] : 1.0;
        h[j] = valid[j] ? boxes[2 * (size_t)i + 1] : 1.0;
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        if (s_done[r]) continue;                                  // the same for the whole workgroup
        const double *c = s_c + r * MAXK * 2;
        int g[PER_THREAD];
        double val = 0.0;                                         // do_kmeans :98-109
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) {
            double md = 1.0, bi = 0.0;
            int gi = 0;
            for (int q = 0; q < k; ++q) {
                const double iou = iou_(w[j], h[j], c[2 * q], c[2 * q + 1]);
                const double d = 1.0 - iou;
                if (d < md) {
                    md = d;
                    gi = q;
                    bi = iou;
                }
            }
            g[j] = valid[j] ? gi : -1;
            val += valid[j] ? (SCORE ? bi : md) : 0.0;
            if (valid[j]) groups[(size_t)r * gpitch + (size_t)chunk * CHUNK + j * THREADS + tid] = (uint8_t)gi;
        }
        val = wave_sum(val);
        if (lane == 0) s_red[wave][V_LOSS] = val;
        for (int q = 0; q < k; ++q) {
            double sw = 0.0, sh = 0.0;
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < PER_THREAD; ++j) {
                const bool in = g[j] == q;
                sw += in ? w[j] : 0.0;
                sh += in ? h[j] : 0.0;
                cnt += __popcll(__ballot(in));
            }
            sw = wave_sum(sw);
            sh = wave_sum(sh);
            if (lane == 0) {
                s_red[wave][3 * q] = sw;
                s_red[wave][3 * q + 1] = sh;
                s_red[wave][3 * q + 2] = (double)cnt;
            }
        }
        __syncthreads();
        if (tid < 3 * k || tid == V_LOSS) {
            double v = s_red[0][tid];
            for (int wv = 1; wv < WAVES; ++wv) v += s_red[wv][tid];
            part[((size_t)r * NV + tid) * pitch + chunk] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void update_kernel(const double *__restrict__ part, int pitch, int nchunks, int k, int max_iters,
                                                         double convergence, double *cent, int *counts, double *loss, double *old_loss,
                                                         int *iters, int *done) {
    __shared__ double s_tile[NV * TILE_LD], s_sum[NV];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (done[r]) return;
    sum_chunks(part + (size_t)r * NV * pitch, pitch, nchunks, k, s_tile, s_sum);
    if (tid < k) {                                                // do_kmeans :111-113
        const double cnt = s_sum[3 * tid + 2], div = cnt > 1.0 ? cnt : 1.0;
        cent[(r * MAXK + tid) * 2] = s_sum[3 * tid] / div;
        cent[(r * MAXK + tid) * 2 + 1] = s_sum[3 * tid + 1] / div;
        counts[r * MAXK + tid] = (int)cnt;
    }
    if (tid == 0) {                                               // anchor_box_kmeans :139-147
        const double l = s_sum[V_LOSS];
        const int s = iters[r] + 1;
        iters[r] = s;
        loss[r] = l;
        if (s == 1) old_loss[r] = l;
        else if (fabs(old_loss[r] - l) < convergence || s > max_iters) done[r] = 1;
        else old_loss[r] = l;
    }
}

__global__ __launch_bounds__(THREADS) void score_finish_kernel(const double *__restrict__ part, int pitch, int nchunks, int k, int n, double *out) {
    __shared__ double s_tile[NV * TILE_LD], s_sum[NV];
    sum_chunks(part, pitch, nchunks, k, s_tile, s_sum);
    if ((int)threadIdx.x < k) out[1 + threadIdx.x] = s_sum[3 * threadIdx.x + 2];
    if (threadIdx.x == 0) out[0] = s_sum[V_LOSS] / (double)n;
}

// ------------------------------------------------------------------------------------------------------ the handle
// y355_anchors_create in two parts, as host_state_check.cpp runs them on the CPU: the rules of the sizes and the host state (no
// device call; the handle gets its device memory from mem), ...
int anchors_open(int32_t device_id, int64_t max_boxes, int32_t max_restarts, int32_t max_k, const DevMem &mem, y355_anchors **out) {
    if (!out) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_create: null out");
    *out = nullptr;
    if (device_id < 0) return y355_fail(Y355_ANCHORS_EINVAL, "device_id < 0");
    if (max_boxes < 1 || max_boxes > Y355_ANCHORS_MAX_BOXES) return y355_fail(Y355_ANCHORS_EINVAL, "max_boxes must be 1..2^28");
    if (max_restarts < 1 || max_restarts > MAXR) return y355_fail(Y355_ANCHORS_EINVAL, "max_restarts must be 1..64");
    if (max_k < 1 || max_k > MAXK) return y355_fail(Y355_ANCHORS_EINVAL, "max_k must be 1..16");
    y355_anchors *h = new y355_anchors();
    h->device_id = device_id;
    h->max_boxes = max_boxes;
    h->max_restarts = max_restarts;
    h->max_k = max_k;
    h->chunks_cap = (int)((max_boxes + CHUNK - 1) / CHUNK);
    h->own.mem = mem;
    *out = h;
    return Y355_ANCHORS_OK;
}
// ... and all of its device memory (on the current device), or none of it
int anchors_buffers(y355_anchors *h) {
    const size_t R = (size_t)h->max_restarts, nb = (size_t)h->max_boxes;
    DevOwner &o = h->own;
    int rc = y355_dev_get(o, &h->boxes, nb * 2);
    rc = rc ? rc : y355_dev_get(o, &h->groups, R * nb);
    rc = rc ? rc : y355_dev_get(o, &h->score_idx, nb);
    rc = rc ? rc : y355_dev_get(o, &h->partial, R * NV * h->chunks_cap);
    rc = rc ? rc : y355_dev_get_all(o, MAXR * MAXK * 2, &h->cent, &h->init);
    rc = rc ? rc : y355_dev_get_all(o, MAXR, &h->loss, &h->old_loss, &h->iters, &h->done, &h->nfound, &h->first);
    rc = rc ? rc : y355_dev_get(o, &h->u, MAXR * (MAXK - 1));
    rc = rc ? rc : y355_dev_get(o, &h->score_anchors, MAXK * 2);
    rc = rc ? rc : y355_dev_get(o, &h->score_out, 1 + MAXK);
    rc = rc ? rc : y355_dev_get_all(o, MAXR * MAXK, &h->counts, &h->init_index);
    rc = rc ? rc : y355_dev_get(o, &h->flag, 1);
    if (rc) y355_dev_release_all(o);
    return rc;
}
DevOwner &anchors_owner(y355_anchors *h) { return h->own; }        // (host_state_check.cpp does not see the struct)
void anchors_free(y355_anchors *h) {
    y355_dev_release_all(h->own);
    delete h;
}

static bool bad_size(double v) { return !std::isfinite(v) || !(v > 0.0); }
#pragma GCC visibility pop

// ------------------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char *y355_anchors_last_error(void) { return g_err.c_str(); }

int y355_anchors_chunk(void) { return CHUNK; }

int y355_anchors_create(int32_t device_id, int64_t max_boxes, int32_t max_restarts, int32_t max_k, y355_anchors **out) {
    if (int rc = anchors_open(device_id, max_boxes, max_restarts, max_k, y355_hip_mem(), out)) return rc;
    DeviceGuard g;
    const hipError_t e = g.set(device_id);
    const int rc = e != hipSuccess ? y355_fail(Y355_ANCHORS_EHIP, std::string("y355_anchors_create: ") + hipGetErrorString(e)) : anchors_buffers(*out);
    if (rc) {
        anchors_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_anchors_destroy(y355_anchors *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->device_id);
    anchors_free(h);
}

int64_t y355_anchors_num_boxes(const y355_anchors *h) { return h ? h->n : y355_fail(Y355_ANCHORS_EINVAL, "null handle"); }

static int check_n(const y355_anchors *h, int64_t n) {
    if (n < 1 || n > h->max_boxes) return y355_fail(Y355_ANCHORS_EINVAL, "n must be 1..max_boxes (" + std::to_string(h->max_boxes) + ")");
    return Y355_ANCHORS_OK;
}

static void hold(y355_anchors *h, int64_t n) {
    h->n = (int)n;
    h->nchunks = (int)((n + CHUNK - 1) / CHUNK);
    h->fit_k = h->fit_r = 0;
}

int y355_anchors_set_boxes(y355_anchors *h, const double *wh, int64_t n) {
    if (!h || !wh) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_set_boxes: null argument");
    if (check_n(h, n)) return Y355_ANCHORS_EINVAL;
    for (int64_t i = 0; i < 2 * n; ++i)
        if (bad_size(wh[i]))
            return y355_fail(Y355_ANCHORS_EINVAL, "box " + std::to_string(i / 2) + ": " + (i & 1 ? "h" : "w") + " must be finite and > 0");
    hold(h, 0);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipMemcpy(h->boxes, wh, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice));
    hold(h, n);
    return Y355_ANCHORS_OK;
}

int y355_anchors_set_boxes_dev(y355_anchors *h, const void *wh_dev, int64_t n, void *stream) {
    if (!h || !wh_dev) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_set_boxes_dev: null argument");
    if (check_n(h, n)) return Y355_ANCHORS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hold(h, 0);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    int flag = 0;
    HIPCHK(hipMemsetAsync(h->flag, 0, sizeof(int), s));
    HIPCHK(hipMemcpyAsync(h->boxes, wh_dev, (size_t)n * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(check_boxes_kernel, dim3((unsigned)((2 * n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, h->boxes, (long long)(2 * n), h->flag);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&flag, h->flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flag) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_set_boxes_dev: every w and h must be finite and > 0");
    hold(h, n);
    return Y355_ANCHORS_OK;
}

int y355_anchors_fit(y355_anchors *h, int32_t k, int32_t restarts, int32_t max_iters, double convergence, const int32_t *first,
                     const double *u, const int32_t *init_index, void *stream) {
    if (!h) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_fit: null handle");
    if (k < 1 || k > h->max_k) return y355_fail(Y355_ANCHORS_EINVAL, "k must be 1..max_k (" + std::to_string(h->max_k) + ")");
    if (restarts < 1 || restarts > h->max_restarts)
        return y355_fail(Y355_ANCHORS_EINVAL, "restarts must be 1..max_restarts (" + std::to_string(h->max_restarts) + ")");
    if (max_iters < 1) return y355_fail(Y355_ANCHORS_EINVAL, "max_iters must be >= 1");
    if (!std::isfinite(convergence) || convergence < 0.0) return y355_fail(Y355_ANCHORS_EINVAL, "convergence must be finite and >= 0");
    if (init_index ? (first || u) : !first)
        return y355_fail(Y355_ANCHORS_EINVAL, "exactly one start: first (with u) or init_index");
    if (!init_index && k > 1 && !u) return y355_fail(Y355_ANCHORS_EINVAL, "u is null and k > 1");
    if (h->n < 1) return y355_fail(Y355_ANCHORS_ENOTREADY, "y355_anchors_fit: no boxes set");
    const int R = restarts, n = h->n;
    std::vector<int> h_first(MAXR, 0), h_index(MAXR * MAXK, 0);
    std::vector<double> h_u(MAXR * (MAXK - 1), 0.0);
    for (int r = 0; r < R; ++r) {
        if (init_index) {
            for (int c = 0; c < k; ++c) {
                const int v = init_index[r * k + c];
                if (v < 0 || v >= n) return y355_fail(Y355_ANCHORS_EINVAL, "init_index[" + std::to_string(r) + "][" + std::to_string(c) + "] outside 0..n-1");
                h_index[r * MAXK + c] = v;
            }
        } else {
            if (first[r] < 0 || first[r] >= n) return y355_fail(Y355_ANCHORS_EINVAL, "first[" + std::to_string(r) + "] outside 0..n-1");
            h_first[r] = first[r];
            for (int j = 0; j < k - 1; ++j) {
                const double v = u[r * (k - 1) + j];
                if (!(v >= 0.0) || !(v < 1.0)) return y355_fail(Y355_ANCHORS_EINVAL, "u[" + std::to_string(r) + "][" + std::to_string(j) + "] outside [0, 1)");
                h_u[r * (MAXK - 1) + j] = v;
            }
        }
    }
    hipStream_t s = (hipStream_t)stream;
    h->fit_k = h->fit_r = 0;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipMemcpyAsync(h->first, h_first.data(), MAXR * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->init_index, h_index.data(), MAXR * MAXK * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->u, h_u.data(), MAXR * (MAXK - 1) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                              // the vectors above are pageable: the copies have read them now
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, s, h->boxes, k, R, h->first, h->init_index, init_index ? 1 : 0, h->cent, h->nfound,
                       h->iters, h->done, h->counts, h->loss, h->old_loss);
    HIPCHK(hipGetLastError());
    if (!init_index)
        for (int pick = 0; pick < k - 1; ++pick) {               // init_centroids :61-83
            hipLaunchKernelGGL(pp_dist_kernel, dim3(h->nchunks, R), dim3(THREADS), 0, s, h->boxes, n, h->cent, h->nfound, h->partial, h->chunks_cap);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(pp_select_kernel, dim3(R), dim3(THREADS), 0, s, h->boxes, n, h->nchunks, pick, h->u, h->cent, h->nfound,
                               h->partial, h->chunks_cap);
            HIPCHK(hipGetLastError());
        }
    HIPCHK(hipMemcpyAsync(h->init, h->cent, MAXR * MAXK * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
    const long long steps_max = (long long)max_iters + 1 > 2 ? (long long)max_iters + 1 : 2;      // every restart is done by then
    int h_done[MAXR];
    for (long long queued = 0; queued < steps_max;) {
        const long long grp = steps_max - queued < QUEUE_GROUP ? steps_max - queued : QUEUE_GROUP;
        for (long long i = 0; i < grp; ++i) {
            hipLaunchKernelGGL(assign_kernel<false>, dim3(h->nchunks), dim3(THREADS), 0, s, h->boxes, n, k, R, h->done, h->cent, h->partial,
                               h->chunks_cap, h->groups, (size_t)h->max_boxes);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(update_kernel, dim3(R), dim3(THREADS), 0, s, h->partial, h->chunks_cap, h->nchunks, k, max_iters, convergence,
                               h->cent, h->counts, h->loss, h->old_loss, h->iters, h->done);
            HIPCHK(hipGetLastError());
        }
        queued += grp;
        HIPCHK(hipMemcpyAsync(h_done, h->done, R * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        bool all = true;
        for (int r = 0; r < R; ++r) all = all && h_done[r];
        if (all) break;
    }
    h->fit_k = k;
    h->fit_r = R;
    return Y355_ANCHORS_OK;
}

int y355_anchors_get_result(y355_anchors *h, double *centroids, double *loss, int32_t *iterations, int32_t *counts,
                            double *init_centroids, int32_t *best) {
    if (!h) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_get_result: null handle");
    if (!h->fit_r) return y355_fail(Y355_ANCHORS_ENOTREADY, "y355_anchors_get_result: no fit made");
    const int R = h->fit_r, k = h->fit_k;
    std::vector<double> c(MAXR * MAXK * 2), c0(MAXR * MAXK * 2), l(MAXR);
    std::vector<int> it(MAXR), cn(MAXR * MAXK);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipMemcpy(c.data(), h->cent, c.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(c0.data(), h->init, c0.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(l.data(), h->loss, l.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(it.data(), h->iters, it.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cn.data(), h->counts, cn.size() * sizeof(int), hipMemcpyDeviceToHost));
    int b = 0;
    for (int r = 0; r < R; ++r) {
        for (int q = 0; q < k; ++q) {
            for (int j = 0; j < 2; ++j) {
                if (centroids) centroids[(r * k + q) * 2 + j] = c[(r * MAXK + q) * 2 + j];
                if (init_centroids) init_centroids[(r * k + q) * 2 + j] = c0[(r * MAXK + q) * 2 + j];
            }
            if (counts) counts[r * k + q] = cn[r * MAXK + q];
        }
        if (loss) loss[r] = l[r];
        if (iterations) iterations[r] = it[r];
        if (l[r] < l[b]) b = r;
    }
    if (best) *best = b;
    return Y355_ANCHORS_OK;
}

static int widen(const uint8_t *src_dev, int n, int32_t *dst) {
    std::vector<uint8_t> tmp((size_t)n);
    HIPCHK(hipMemcpy(tmp.data(), src_dev, (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) dst[i] = tmp[i];
    return Y355_ANCHORS_OK;
}

int y355_anchors_assignments(y355_anchors *h, int32_t restart, int32_t *dst) {
    if (!h || !dst) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_assignments: null argument");
    if (!h->fit_r) return y355_fail(Y355_ANCHORS_ENOTREADY, "y355_anchors_assignments: no fit made");
    if (restart < 0 || restart >= h->fit_r) return y355_fail(Y355_ANCHORS_EINVAL, "restart must be 0..restarts-1 of the last fit");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    return widen(h->groups + (size_t)restart * h->max_boxes, h->n, dst);
}

int y355_anchors_score(y355_anchors *h, const double *anchors, int32_t k, double *mean_iou, int32_t *counts, int32_t *best_index) {
    if (!h || !anchors || !mean_iou || !counts) return y355_fail(Y355_ANCHORS_EINVAL, "y355_anchors_score: null argument");
    if (k < 1 || k > h->max_k) return y355_fail(Y355_ANCHORS_EINVAL, "k must be 1..max_k (" + std::to_string(h->max_k) + ")");
    double a[MAXK * 2] = {0.0};
    for (int i = 0; i < 2 * k; ++i) {
        if (!std::isfinite(anchors[i]) || anchors[i] < 0.0) return y355_fail(Y355_ANCHORS_EINVAL, "anchors must be finite and >= 0");
        a[i] = anchors[i];
    }
    if (h->n < 1) return y355_fail(Y355_ANCHORS_ENOTREADY, "y355_anchors_score: no boxes set");
    // slot 0 of `partial` is free between fits; the results of a fit (cent, loss, counts, groups) are not touched.  The anchor
    // set goes to the handle's score_anchors: the upload is synchronous, the two launches run on the null stream behind it,
    // and the synchronous read-back returns only after them -- so the next call's upload cannot overtake this call's kernels.
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipMemcpy(h->score_anchors, a, sizeof(a), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(assign_kernel<true>, dim3(h->nchunks), dim3(THREADS), 0, nullptr, h->boxes, h->n, k, 1, (const int *)nullptr,
                       h->score_anchors, h->partial, h->chunks_cap, h->score_idx, (size_t)0);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(THREADS), 0, nullptr, h->partial, h->chunks_cap, h->nchunks, k, h->n, h->score_out);
    HIPCHK(hipGetLastError());
    double out[1 + MAXK];
    HIPCHK(hipMemcpy(out, h->score_out, sizeof(out), hipMemcpyDeviceToHost));
    *mean_iou = out[0];
    for (int q = 0; q < k; ++q) counts[q] = (int32_t)out[1 + q];
    if (best_index) return widen(h->score_idx, h->n, best_index);
    return Y355_ANCHORS_OK;
}

}  // extern "C"
