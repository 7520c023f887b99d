// yolo355 -- COCO bbox AP on the GPU behind y355_apeval_set_gt_coco / compute_coco / coco_matches (include/yolo355.h): what
// COCOeval(cocoGt, cocoGt.loadRes(data_dict), 'bbox').evaluate() / accumulate() / summarize() compute after the loop of
// utils/cocoapi_evaluator.py:53-126, from the device store that y355_apeval_add fills.  DESIGN.md section 6c has the contract.
//
//   sort A   (class, image rank, score descending, position): the store's radix sort (apeval_shared.h) over the word
//            rank << 20 | position; every (image, category) group is then one run, in the order evaluateImg walks it
//   match    one workgroup per (image, category), one wave per (area range, threshold) pair at a time: the sequential chain over the
//            group's first maxDets[-1] detections, each link a wave-wide argmax over the group's boxes -- the best free kept box (of
//            equal IoUs the later one), else the best ignored one (crowd boxes are always free).  Lane l owns boxes l, l + 64, ...:
//            it alone reads and writes their marks, which live in global memory, so a group may hold any number of boxes; the IoU is
//            recomputed per link instead of being kept as a D x G matrix
//   sort B   (class, score descending, image rank, position): the score and class passes again, over sort A's order (stable)
//   accum    one workgroup per (category, area range, budget), thresholds in turn: the masked sums of TP / FP (the carry runs
//            backwards from the total), pr at every true positive, its running maximum from the right, and per recall threshold
//            the first true positive whose recall reaches it.  Detections past the budget or ignored add nothing to either
//            sum, so they stay in place as zeros instead of being compacted away: neither the envelope nor a lower bound sees them
#include "apeval_shared.h"

#include <cfloat>
#include <cmath>

namespace {
// gkey[r] = class << 24 | image rank of the r-th entry of sort A: ascending, one run per (image, category) group
__global__ void __launch_bounds__(256) coco_gkey_kernel(long long n, const unsigned int *permA, const uint8_t *scls, const unsigned long long *w0,
                                                        unsigned int *gkey) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const unsigned int e = permA[r];
    gkey[r] = ((unsigned int)scls[e] << 24) | (unsigned int)(w0[e] >> AP_POS_BITS);
}

__device__ __forceinline__ long long coco_lower_bound(const unsigned int *a, long long n, unsigned long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((unsigned long long)a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int coco_lower_bound_cls(const int *a, int lo, int hi, int key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// bbIou of maskApi.c for one pair of x y w h boxes
__device__ __forceinline__ double coco_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh, bool crowd) {
    const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
    if (w <= 0) return 0.0;
    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? dw * dh : dw * dh + gw * gh - i;
    return i / u;
}

// the better of two candidates of one link: the larger IoU, of equal ones the later box; idx < 0 = none
__device__ __forceinline__ void coco_pick(double &iou, int &idx, double iou2, int idx2) {
    if (idx2 >= 0 && (idx < 0 || iou2 > iou || (iou2 == iou && idx2 > idx))) iou = iou2, idx = idx2;
}

// One workgroup per (image, category) group.  tap != null: the group (tap_img, tap_cls) alone, area range tap_a alone, by one
// workgroup, which also writes the parity tap: tap[0] = D, tap[1] = G, then (when D <= cap_d and G <= cap_g) pos [cap_d],
// matched box [T][cap_d], ignore flag [T][cap_d], marks [T][cap_g]
__global__ void __launch_bounds__(256) coco_match_kernel(CocoParams P, long long n, long long n_gt, const unsigned int *permA, const unsigned int *gkey,
                                                         const unsigned long long *w0, const float *sbox, const int *img_rank, const int *gt_off,
                                                         const int *gt_cls, const double *gt_box, const double *gt_area, const uint8_t *gt_crowd,
                                                         uint8_t *marks, uint8_t *flags, unsigned int *gidx, int tap_img, int tap_cls, int tap_a,
                                                         int32_t *tap, int cap_d, int cap_g) {
    const int img = tap ? tap_img : (int)blockIdx.x, c = tap ? tap_cls : (int)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g0 = coco_lower_bound_cls(gt_cls, gt_off[img], gt_off[img + 1], c), g1 = coco_lower_bound_cls(gt_cls, g0, gt_off[img + 1], c + 1);
    const unsigned long long key = ((unsigned long long)c << 24) | (unsigned int)img_rank[img];
    const long long d0 = coco_lower_bound(gkey, n, key), d1 = coco_lower_bound(gkey, n, key + 1);
    const int G = g1 - g0;
    const long long Dall = d1 - d0;
    const int D = (int)(Dall < (long long)P.max_det[P.M - 1] ? Dall : (long long)P.max_det[P.M - 1]);
    const bool fits = tap && D <= cap_d && G <= cap_g;
    if (tap && threadIdx.x == 0) tap[0] = D, tap[1] = G;
    if (G == 0 && Dall == 0) return;
    for (long long j = threadIdx.x; j < Dall; j += 256) {
        const unsigned int e = permA[d0 + j];
        gidx[e] = (unsigned int)j;                        // the detection's place in its group: what a budget cuts by
        if (fits && j < D) tap[2 + j] = (int32_t)(w0[e] & ((1u << AP_POS_BITS) - 1));
    }
    int32_t *tap_m = fits ? tap + 2 + cap_d : nullptr, *tap_i = fits ? tap_m + (size_t)P.T * cap_d : nullptr,
            *tap_g = fits ? tap_i + (size_t)P.T * cap_d : nullptr;
    for (int combo = wave; combo < P.A * P.T; combo += 4) {
        const int a = combo / P.T, t = combo - a * P.T;
        if (tap && a != tap_a) continue;
        const double lo = P.alo[a], hi = P.ahi[a];
        const double start = fmin(P.thr[t], 1 - 1e-10);
        uint8_t *mk = marks + (size_t)combo * n_gt + g0;
        for (int g = lane; g < G; g += 64) mk[g] = 0;
        for (int d = 0; d < D; ++d) {
            const unsigned int e = permA[d0 + d];
            const float4 bf = ((const float4 *)sbox)[e];
            const double dx = (double)bf.x, dy = (double)bf.y, dw = (double)bf.z - (double)bf.x, dh = (double)bf.w - (double)bf.y;
            // this lane's boxes in order: a candidate among the free kept ones (1) and among the available ignored ones (2)
            double iou1 = start, iou2 = start;
            int idx1 = -1, idx2 = -1;
            for (int g = lane; g < G; g += 64) {
                const bool crowd = gt_crowd[g0 + g] != 0;
                if (mk[g] && !crowd) continue;
                const double ar = gt_area[g0 + g];
                const bool ig = crowd || ar < lo || ar > hi;
                const double *gb = gt_box + 4 * (size_t)(g0 + g);
                const double iou = coco_iou(dx, dy, dw, dh, gb[0], gb[1], gb[2], gb[3], crowd);
                if (ig) {
                    if (!(iou < iou2)) iou2 = iou, idx2 = g;
                } else {
                    if (!(iou < iou1)) iou1 = iou, idx1 = g;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                coco_pick(iou1, idx1, __shfl_xor(iou1, o, 64), __shfl_xor(idx1, o, 64));
                coco_pick(iou2, idx2, __shfl_xor(iou2, o, 64), __shfl_xor(idx2, o, 64));
            }
            const int m = idx1 >= 0 ? idx1 : idx2;
            bool ign;
            if (m >= 0) {
                ign = idx1 < 0;
                if ((m & 63) == lane) mk[m] = 1;          // by the lane that owns the box
            } else {
                const double area = dw * dh;
                ign = area < lo || area > hi;
            }
            if (lane == 0) {
                flags[(size_t)combo * n + e] = (uint8_t)((m >= 0 ? 1 : 0) | (ign ? 2 : 0));
                if (fits) tap_m[(size_t)t * cap_d + d] = m, tap_i[(size_t)t * cap_d + d] = ign ? 1 : 0;
            }
        }
        if (fits)
            for (int g = lane; g < G; g += 64) tap_g[(size_t)t * cap_g + g] = mk[g];
    }
}

// One workgroup per (category, area range, budget); the thresholds in turn.
__global__ void __launch_bounds__(AP_SCORE_THREADS) coco_accum_kernel(CocoParams P, long long n, int K, const long long *start, const unsigned int *permB,
                                                                      const uint8_t *flags, const unsigned int *gidx, const int *npig,
                                                                      const double *rec_thrs, double *precision, double *recall) {
    __shared__ unsigned long long sh_u[AP_SCORE_THREADS / 64];
    __shared__ double sh_d[AP_SCORE_THREADS / 64];
    __shared__ double envq[AP_SCORE_THREADS];
    const int k = blockIdx.x, a = blockIdx.y / P.M, m = blockIdx.y - a * P.M, r = threadIdx.x;
    const long long s0 = start[k], nd = start[k + 1] - s0;
    const int np = npig[k * P.A + a];
    const unsigned int md = (unsigned int)P.max_det[m];
    const double dnp = (double)np;
    const long long nch = (nd + AP_SCORE_THREADS - 1) / AP_SCORE_THREADS;
    for (int t = 0; t < P.T; ++t) {
        double *pout = precision + ((((size_t)t * P.R + r) * K + k) * P.A + a) * P.M + m;
        double *rout = recall + (((size_t)t * K + k) * P.A + a) * P.M + m;
        if (np == 0) {                                    // no kept box of the category in this range: the entries stay -1
            if (r < P.R) *pout = -1.0;
            if (r == 0) *rout = -1.0;
            continue;
        }
        const uint8_t *fl = flags + (size_t)(a * P.T + t) * n;
        // the totals: TP in the high word, FP in the low one
        unsigned long long tot = 0;
        for (long long ch = 0; ch < nch; ++ch) {
            const long long i = ch * AP_SCORE_THREADS + r;
            unsigned long long v = 0;
            if (i < nd) {
                const unsigned int e = permB[s0 + i];
                if (gidx[e] < md) {
                    const int f = fl[e];
                    v = (f & 2) ? 0ull : (f & 1) ? (1ull << 32) : 1ull;
                }
            }
            unsigned long long all;
            (void)block_scan_add(v, sh_u, &all);
            tot += all;
        }
        // searchsorted(rc, recThrs, 'left'): recall first reaches the threshold at the need-th true positive, need = the smallest
        // count q with double(q) / npig >= the threshold (0: the first entry, whose envelope is that of the first true positive)
        long long need = 0;
        if (r < P.R) {
            const double thr = rec_thrs[r];
            long long lo = 0, hi = (long long)np + 1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if ((double)mid / dnp >= thr) hi = mid;
                else lo = mid + 1;
            }
            need = lo < 1 ? 1 : lo;
        }
        double ans = 0.0, cmax = 0.0;
        unsigned long long after = tot;
        for (long long ch = nch - 1; ch >= 0; --ch) {
            const long long i = ch * AP_SCORE_THREADS + r;
            unsigned long long v = 0;
            if (i < nd) {
                const unsigned int e = permB[s0 + i];
                if (gidx[e] < md) {
                    const int f = fl[e];
                    v = (f & 2) ? 0ull : (f & 1) ? (1ull << 32) : 1ull;
                }
            }
            unsigned long long all;
            const unsigned long long incl = block_scan_add(v, sh_u, &all);
            const unsigned long long base = after - all, pre = base + incl;          // the carry, backwards from the total
            const long long q0 = (long long)(base >> 32), nq = (long long)(all >> 32);      // true positives q0 + 1 .. q0 + nq are here
            __syncthreads();                              // envq of the chunk before has been read
            if (v >> 32) {
                const double tp = (double)(pre >> 32), fp = (double)(pre & 0xffffffffull);
                envq[(long long)(pre >> 32) - q0 - 1] = tp / ((fp + tp) + DBL_EPSILON);
            }
            __syncthreads();
            const double p = r < nq ? envq[nq - 1 - r] : 0.0;                                 // from the right
            double top;
            const double env = fmax(cmax, block_scan_max(p, sh_d, &top));
            cmax = fmax(cmax, top);
            __syncthreads();
            if (r < nq) envq[nq - 1 - r] = env;
            __syncthreads();
            if (r < P.R && need > q0 && need <= q0 + nq) ans = envq[need - q0 - 1];
            after = base;
        }
        if (r < P.R) *pout = ans;
        if (r == 0) *rout = (double)(tot >> 32) / dnp;
        __syncthreads();
    }
}

void coco_launch_match(y355_apeval *e, y355_coco *c, dim3 grid, int tap_img, int tap_cls, int tap_a, int32_t *tap, int cap_d, int cap_g) {
    hipLaunchKernelGGL(coco_match_kernel, grid, dim3(256), 0, e->s, c->P, c->n, c->n_gt, c->permA, c->gkey, c->w0, e->d_box, c->img_rank, c->gt_off,
                       c->gt_cls, c->gt_box, c->gt_area, c->gt_crowd, c->marks, c->flags, c->gidx, tap_img, tap_cls, tap_a, tap, cap_d, cap_g);
}

// mean of the entries > -1 of one summarize() selection, summed in order; -1 without any
struct CocoMean {
    double sum = 0.0;
    long long cnt = 0;
    void add(double v) {
        if (v > -1) sum += v, ++cnt;
    }
    double get() const { return cnt ? sum / (double)cnt : -1.0; }
};
}  // namespace

// ---- e->coco's device memory (apeval_shared.h)
int coco_set_gt(y355_apeval *e, const int32_t *offsets, const int32_t *rank, const std::vector<double> &h_box, std::vector<int32_t> &h_cls,
                std::vector<double> &h_area, std::vector<uint8_t> &h_crowd) {
    const size_t n = h_cls.size(), N = (size_t)e->num_images;
    if (!e->coco) e->coco = new y355_coco;
    y355_coco *c = e->coco;
    DevOwner &o = e->own;
    c->have_gt = false, c->have_result = false, c->n_gt = 0;
    y355_dev_drop(o, &c->gt_off, &c->gt_cls, &c->img_rank, &c->gt_box, &c->gt_area, &c->gt_crowd);
    int rc = y355_dev_get(o, &c->gt_off, N + 1);
    rc = rc ? rc : y355_dev_get(o, &c->img_rank, N);
    rc = rc ? rc : y355_dev_get(o, &c->gt_box, 4 * n);
    rc = rc ? rc : y355_dev_get_all(o, n, &c->gt_cls, &c->gt_area, &c->gt_crowd);
    rc = rc ? rc : o.mem.upload(c->gt_off, offsets, (N + 1) * sizeof(int32_t), e->s);
    rc = rc ? rc : o.mem.upload(c->img_rank, rank, N * sizeof(int32_t), e->s);
    if (n > 0) {
        rc = rc ? rc : o.mem.upload(c->gt_cls, h_cls.data(), n * sizeof(int32_t), e->s);
        rc = rc ? rc : o.mem.upload(c->gt_box, h_box.data(), 4 * n * sizeof(double), e->s);
        rc = rc ? rc : o.mem.upload(c->gt_area, h_area.data(), n * sizeof(double), e->s);
        rc = rc ? rc : o.mem.upload(c->gt_crowd, h_crowd.data(), n, e->s);
    }
    if (rc) return rc;
    c->h_cls.swap(h_cls), c->h_area.swap(h_area), c->h_crowd.swap(h_crowd);
    c->n_gt = (long long)n, c->have_gt = true;
    return 0;
}

int coco_workspaces(y355_apeval *e, long long n, int T, int R, int A, int M) {
    y355_coco *c = e->coco;
    DevOwner &o = e->own;
    const size_t K = (size_t)e->C, n1 = (size_t)(n > 0 ? n : 1), g1 = (size_t)(c->n_gt > 0 ? c->n_gt : 1);
    int rc = c->npig ? 0 : y355_dev_get(o, &c->npig, K * COCO_MAX_A);
    rc = rc || c->rec_thrs ? rc : y355_dev_get(o, &c->rec_thrs, (size_t)COCO_MAX_R);
    rc = rc ? rc : y355_dev_grow(o, &c->prec_cap, (size_t)T * R * K * A * M, &c->prec_out);
    rc = rc ? rc : y355_dev_grow(o, &c->rec_cap, (size_t)T * K * A * M, &c->rec_out);
    rc = rc ? rc : y355_dev_grow(o, &c->n_cap, n1, &c->permA, &c->permB, &c->gkey, &c->gidx, &c->w0);
    rc = rc ? rc : y355_dev_grow(o, &c->flags_cap, (size_t)A * T * n1, &c->flags);
    rc = rc ? rc : y355_dev_grow(o, &c->marks_cap, (size_t)A * T * g1, &c->marks);
    return rc;
}

extern "C" {

int y355_apeval_set_gt_coco(y355_apeval *e, const int32_t *offsets, const double *boxes_xywh, const double *area, const int32_t *cls,
                            const uint8_t *iscrowd, const int32_t *image_rank) {
    long long n = 0;
    if (int rc = ap_check_gt(e, offsets, cls, boxes_xywh && area && cls && iscrowd, &n)) return rc;
    const int N = e->num_images;
    std::vector<int32_t> rank(N);
    if (image_rank) {
        std::vector<uint8_t> seen(N, 0);
        for (int i = 0; i < N; ++i) {
            if (image_rank[i] < 0 || image_rank[i] >= N) return y355_fail(Y355_EINVAL, "image_rank outside 0 .. num_images - 1");
            if (seen[image_rank[i]]) return y355_fail(Y355_EINVAL, "image_rank holds a rank twice (duplicate image ids)");
            seen[image_rank[i]] = 1;
            rank[i] = image_rank[i];
        }
    } else {
        for (int i = 0; i < N; ++i) rank[i] = i;
    }
    // inside an image: stable by class, so a group is one run in annotation order
    std::vector<int32_t> h_cls((size_t)n);
    std::vector<double> h_box(4 * (size_t)n), h_area((size_t)n);
    std::vector<uint8_t> h_crowd((size_t)n);
    {
        std::vector<int32_t> cnt(e->C + 1);
        for (int i = 0; i < N; ++i) {
            const int32_t a = offsets[i], b = offsets[i + 1];
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int32_t g = a; g < b; ++g) ++cnt[cls[g] + 1];
            for (int k = 0; k < e->C; ++k) cnt[k + 1] += cnt[k];
            for (int32_t g = a; g < b; ++g) {
                const size_t o = (size_t)a + cnt[cls[g]]++;
                h_cls[o] = cls[g], h_area[o] = area[g], h_crowd[o] = iscrowd[g] != 0;
                for (int j = 0; j < 4; ++j) h_box[4 * o + j] = boxes_xywh[4 * (size_t)g + j];
            }
        }
    }
    if (int rc = ap_enter(e)) return rc;
    HIPCHK(hipStreamSynchronize(e->s));                   // nothing in flight reads the arrays that go
    return coco_set_gt(e, offsets, rank.data(), h_box, h_cls, h_area, h_crowd);
}

int y355_apeval_compute_coco(y355_apeval *e, const double *iou_thrs, int T, const double *rec_thrs, int R, const double *area_rng, int A,
                             const int32_t *max_dets, int M, double *precision, double *recall, double *stats) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!iou_thrs || !rec_thrs || !area_rng || !max_dets) return y355_fail(Y355_EINVAL, "null parameter array");
    if (!precision || !recall) return y355_fail(Y355_EINVAL, "null output");
    if (T < 1 || T > COCO_MAX_T) return y355_fail(Y355_EINVAL, "T outside 1 .. 16");
    if (R < 1 || R > COCO_MAX_R) return y355_fail(Y355_EINVAL, "R outside 1 .. 1024");
    if (A < 1 || A > COCO_MAX_A) return y355_fail(Y355_EINVAL, "A outside 1 .. 8");
    if (M < 1 || M > COCO_MAX_M) return y355_fail(Y355_EINVAL, "M outside 1 .. 8");
    for (int m = 0; m < M; ++m) {
        if (max_dets[m] < 1 || max_dets[m] > (1 << AP_POS_BITS)) return y355_fail(Y355_EINVAL, "max_dets outside 1 .. 2^20");
        if (m && max_dets[m] < max_dets[m - 1]) return y355_fail(Y355_EINVAL, "max_dets must be ascending");
    }
    y355_coco *c = e->coco;
    if (!c || !c->have_gt) return y355_fail(Y355_ENOTREADY, "no COCO ground truth: call y355_apeval_set_gt_coco first");
    if (int rc = ap_enter(e)) return rc;
    c->have_result = false;
    hipStream_t s = e->s;
    long long n = 0;
    if (int rc = ap_store_count(e, &n)) return rc;
    const int K = e->C;
    CocoParams &P = c->P;
    P.T = T, P.A = A, P.M = M, P.R = R;
    for (int t = 0; t < T; ++t) P.thr[t] = iou_thrs[t];
    for (int a = 0; a < A; ++a) P.alo[a] = area_rng[2 * a], P.ahi[a] = area_rng[2 * a + 1];
    for (int m = 0; m < M; ++m) P.max_det[m] = max_dets[m];
    c->n = n;
    // kept boxes per (category, area range): every image with a box of the category is part of the category's list
    std::vector<int32_t> npig((size_t)K * A, 0);
    for (long long g = 0; g < c->n_gt; ++g)
        for (int a = 0; a < A; ++a)
            if (!(c->h_crowd[g] || c->h_area[g] < P.alo[a] || c->h_area[g] > P.ahi[a])) ++npig[(size_t)c->h_cls[g] * A + a];
    const size_t np = (size_t)T * R * K * A * M, nr = (size_t)T * K * A * M;
    if (int rc = coco_workspaces(e, n, T, R, A, M)) return rc;
    HIPCHK(hipMemcpyAsync(c->npig, npig.data(), npig.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->rec_thrs, rec_thrs, (size_t)R * sizeof(double), hipMemcpyHostToDevice, s));
    if (n > 0) {
        unsigned long long h[8];
        if (int rc = ap_keys(e, n, 0, c->img_rank, c->w0, h)) return rc;
        ApPass pa[15], pb[9];
        int na = 0, nb = 0;
        pa[na++] = ApPass{0, 0, 255u}, pa[na++] = ApPass{0, 8, 255u}, pa[na++] = ApPass{0, 16, 15u};                  // the position
        for (int j = 0; j < 8; ++j) pa[na++] = ApPass{1, 8 * j, 255u}, pb[nb++] = ApPass{1, 8 * j, 255u};            // the score
        for (int j = 0; j < 3; ++j) pa[na++] = ApPass{0, AP_POS_BITS + 8 * j, 255u};                                 // the image rank
        pa[na++] = ApPass{2, 0, 255u}, pb[nb++] = ApPass{2, 0, 255u};                                                // the class
        if (int rc = ap_sort(e, n, c->w0, h, pa, na)) return rc;
        HIPCHK(hipMemcpyAsync(c->permA, e->perm[e->cur], (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(coco_gkey_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, s, n, c->permA, e->d_cls, c->w0, c->gkey);
        // inside equal (class, score), sort A's order is already (image rank, position)
        if (int rc = ap_sort(e, n, c->w0, h, pb, nb)) return rc;
        HIPCHK(hipMemcpyAsync(c->permB, e->perm[e->cur], (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToDevice, s));
        ap_class_bounds(e, n);
    } else {
        HIPCHK(hipMemsetAsync(e->start, 0, ((size_t)K + 1) * sizeof(long long), s));
    }
    if (n > 0 || c->n_gt > 0) coco_launch_match(e, c, dim3(e->num_images, K), 0, 0, 0, nullptr, 0, 0);
    hipLaunchKernelGGL(coco_accum_kernel, dim3(K, A * M), dim3(AP_SCORE_THREADS), 0, s, P, n, K, e->start, c->permB, c->flags, c->gidx, c->npig,
                       c->rec_thrs, c->prec_out, c->rec_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(precision, c->prec_out, np * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(recall, c->rec_out, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c->have_result = true;
    if (stats && T == 10 && R == 101 && A == 4 && M == 3) {
        auto ap = [&](int t0, int t1, int a) {
            CocoMean mean;
            for (int t = t0; t < t1; ++t)
                for (int r = 0; r < R; ++r)
                    for (int k = 0; k < K; ++k) mean.add(precision[((((size_t)t * R + r) * K + k) * A + a) * M + (M - 1)]);
            return mean.get();
        };
        auto ar = [&](int a, int m) {
            CocoMean mean;
            for (int t = 0; t < T; ++t)
                for (int k = 0; k < K; ++k) mean.add(recall[(((size_t)t * K + k) * A + a) * M + m]);
            return mean.get();
        };
        stats[0] = ap(0, T, 0), stats[1] = ap(0, 1, 0), stats[2] = ap(5, 6, 0);
        stats[3] = ap(0, T, 1), stats[4] = ap(0, T, 2), stats[5] = ap(0, T, 3);
        stats[6] = ar(0, 0), stats[7] = ar(0, 1), stats[8] = ar(0, 2);
        stats[9] = ar(1, 2), stats[10] = ar(2, 2), stats[11] = ar(3, 2);
    }
    return 0;
}

int y355_apeval_coco_matches(y355_apeval *e, int image, int cls, int area_index, int64_t cap_d, int64_t cap_g, int64_t *num_d, int64_t *num_g,
                             int32_t *det_pos, int32_t *dt_match, uint8_t *dt_ignore, uint8_t *gt_marked) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!num_d || !num_g) return y355_fail(Y355_EINVAL, "null count");
    if (image < 0 || image >= e->num_images) return y355_fail(Y355_EINVAL, "image outside 0 .. num_images - 1");
    if (cls < 0 || cls >= e->C) return y355_fail(Y355_EINVAL, "class outside 0 .. num_classes - 1");
    if (cap_d < 0 || cap_g < 0 || cap_d > (1 << AP_POS_BITS) || cap_g > (1 << 24)) return y355_fail(Y355_EINVAL, "capacity outside 0 .. 2^20 / 2^24");
    y355_coco *c = e->coco;
    if (!c || !c->have_result)
        return y355_fail(Y355_ENOTREADY, "no matches: y355_apeval_compute_coco has not succeeded since the last add / reset");
    if (area_index < 0 || area_index >= c->P.A) return y355_fail(Y355_EINVAL, "area index outside 0 .. A - 1");
    if (int rc = ap_enter(e)) return rc;
    const int T = c->P.T;
    const size_t words = 2 + (size_t)cap_d * (1 + 2 * (size_t)T) + (size_t)cap_g * T;
    if (int rc = coco_tap(e, words)) return rc;
    coco_launch_match(e, c, dim3(1), image, cls, area_index, c->tap, (int)cap_d, (int)cap_g);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> h(words);
    HIPCHK(hipMemcpyAsync(h.data(), c->tap, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->s));
    HIPCHK(hipStreamSynchronize(e->s));
    const int64_t D = h[0], G = h[1];
    *num_d = D, *num_g = G;
    if (D > cap_d || G > cap_g) return 0;
    HIPCHK(hipMemcpy(h.data(), c->tap, words * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int32_t *pos = h.data() + 2, *tm = pos + cap_d, *ti = tm + (size_t)T * cap_d, *tg = ti + (size_t)T * cap_d;
    for (int64_t d = 0; d < D; ++d) {
        if (det_pos) det_pos[d] = pos[d];
        for (int t = 0; t < T; ++t) {
            if (dt_match) dt_match[(size_t)t * cap_d + d] = tm[(size_t)t * cap_d + d];
            if (dt_ignore) dt_ignore[(size_t)t * cap_d + d] = (uint8_t)ti[(size_t)t * cap_d + d];
        }
    }
    if (gt_marked)
        for (int t = 0; t < T; ++t)
            for (int64_t g = 0; g < G; ++g) gt_marked[(size_t)t * cap_g + g] = (uint8_t)tg[(size_t)t * cap_g + g];
    return 0;
}

}  // extern "C"
