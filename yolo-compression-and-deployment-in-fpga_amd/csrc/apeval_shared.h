// yolo355 -- what the two users of a y355_apeval handle share: the handle itself (device store of detection records, sort
// workspace), the entry points of the append store's radix sort (apeval.hip) and the workgroup scans.  apeval.hip scores a run the
// VOC way, cocoeval.hip the COCO way; DESIGN.md section 6c has both contracts.
#pragma once
#include "../../include/yolo355.h"
#include "y355_common.h"

#define AP_POS_BITS 20            // position of a detection in its image's list: max_det <= 2^20
#define AP_TILE 1024              // keys per workgroup of a sort pass: 4 waves x 4 rounds x 64
#define AP_SCORE_THREADS 1024

#define COCO_MAX_T 16
#define COCO_MAX_A 8
#define COCO_MAX_M 8
#define COCO_MAX_R 1024

struct CocoParams {
    int T, A, M, R;
    int max_det[COCO_MAX_M];
    double thr[COCO_MAX_T];
    double alo[COCO_MAX_A], ahi[COCO_MAX_A];
};

// the COCO ground truth, parameters and workspaces of a handle (cocoeval.hip); made by the first y355_apeval_set_gt_coco
struct y355_coco {
    // ground truth: CSR by image (the caller's image index), inside an image stable-sorted by class
    bool have_gt = false;
    long long n_gt = 0;
    int *gt_off = nullptr, *gt_cls = nullptr, *img_rank = nullptr;
    double *gt_box = nullptr, *gt_area = nullptr;
    uint8_t *gt_crowd = nullptr;
    std::vector<int32_t> h_cls;
    std::vector<double> h_area;
    std::vector<uint8_t> h_crowd;
    // workspaces, grown on demand
    unsigned long long *w0 = nullptr;     // [n] image rank << AP_POS_BITS | position
    unsigned int *permA = nullptr, *permB = nullptr, *gkey = nullptr, *gidx = nullptr;
    size_t n_cap = 0;                     // of w0, permA, permB, gkey and gidx
    uint8_t *flags = nullptr;             // [A T][n] by store entry: bit 0 matched, bit 1 ignored
    size_t flags_cap = 0;
    uint8_t *marks = nullptr;             // [A T][n_gt]
    size_t marks_cap = 0;
    int *npig = nullptr;                  // [K][A]
    double *rec_thrs = nullptr;           // [COCO_MAX_R]
    double *prec_out = nullptr, *rec_out = nullptr;
    size_t prec_cap = 0, rec_cap = 0;
    int32_t *tap = nullptr;
    size_t tap_cap = 0;
    // last compute
    bool have_result = false;
    long long n = 0;
    CocoParams P;
};

struct y355_apeval {
    int device = 0, C = 0, num_images = 0;
    long long cap = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    DevOwner own;                         // every device array of the handle, e->coco's included
    // ground truth, CSR by image
    bool have_gt = false;
    long long n_gt = 0;
    int *gt_off = nullptr;
    float *gt_box = nullptr;
    int *gt_cls = nullptr;
    uint8_t *gt_diff = nullptr;
    unsigned int *gt_first = nullptr;     // [n_gt] smallest rank that matched the box
    std::vector<int32_t> npos;
    // the store
    unsigned long long *ctr = nullptr;    // [0] detections offered, [1] of them with a class outside [0, C); [2..7] OR / AND of the keys
    unsigned long long *d_imgpos = nullptr;
    uint8_t *d_cls = nullptr;
    float *d_score = nullptr;
    float *d_box = nullptr;
    // compute workspace
    unsigned long long *khi = nullptr;
    unsigned int *perm[2] = {nullptr, nullptr};
    unsigned int *hist = nullptr;         // [256][tiles]
    unsigned int *dtot = nullptr;         // [256] keys per digit of the pass at hand
    int *jm = nullptr;
    uint8_t *flag = nullptr;
    double *rec = nullptr, *prec = nullptr;
    long long *start = nullptr;           // [C + 1]
    double *ap = nullptr;                 // [C]
    // staging of add_host
    char *stage = nullptr;
    size_t stage_bytes = 0;
    // last compute
    bool have_curve = false;
    int cur = 0;
    std::vector<long long> h_start;
    y355_coco *coco = nullptr;
};

inline int ap_check_handle(const y355_apeval *e) { return e ? 0 : y355_fail(Y355_EINVAL, "null apeval handle"); }
inline int ap_enter(y355_apeval *e) {
    HIPCHK(hipSetDevice(e->device));
    return 0;
}
// the top of add, add_host and reset: a mutation of the store forgets the last results, VOC and COCO
inline int ap_mutate(y355_apeval *e) {
    if (int rc = ap_enter(e)) return rc;
    e->have_curve = false;
    if (e->coco) e->coco->have_result = false;
    return 0;
}

// ---- the handle's device memory (apeval.hip, cocoeval.hip).  These reach the device through e->own alone, so
// host_state_check.cpp runs them on the CPU with an allocator that fails on demand.
// the store and the compute workspace for e->C classes and e->cap detections: all of them or, after a failure, none
int ap_buffers(y355_apeval *e);
// the five rules of a ground truth, VOC or COCO, behind the null-handle check; have_arrays: no per-box array is null; *n = its boxes
int ap_check_gt(const y355_apeval *e, const int32_t *offsets, const int32_t *cls, bool have_arrays, long long *n);
// replace the ground truth by a checked one (the stream is idle); a failure leaves the handle without one
int ap_set_gt(y355_apeval *e, const int32_t *offsets, const float *boxes, const int32_t *cls, const uint8_t *difficult);
// the same for the COCO one (the per-box arrays grouped by class inside an image); the host copies are swapped in on success only
int coco_set_gt(y355_apeval *e, const int32_t *offsets, const int32_t *rank, const std::vector<double> &h_box, std::vector<int32_t> &h_cls,
                std::vector<double> &h_area, std::vector<uint8_t> &h_crowd);
// e->coco's workspaces for n detections (and its n_gt boxes) under T thresholds, R recall points, A area ranges, M budgets
int coco_workspaces(y355_apeval *e, long long n, int T, int R, int A, int M);
inline int coco_tap(y355_apeval *e, size_t words) { return y355_dev_grow(e->own, &e->coco->tap_cap, words, &e->coco->tap); }
inline int ap_stage(y355_apeval *e, size_t bytes) { return y355_dev_grow(e->own, &e->stage_bytes, bytes, &e->stage); }
// returns every array and e->coco; the sizes, the stream and the event stay.  A second call does nothing
void ap_close(y355_apeval *e);

// ---- the store and its sort (apeval.hip)
// One digit of a sort key: (word[src][entry] >> shift) & mask, mask <= 255.  src 0: the 64-bit word w0 of ap_sort (image <<
// AP_POS_BITS | position of the store, or any other per-entry word); 1: the score key; 2: the class.
struct ApPass { int src, shift; unsigned int mask; };
// waits for every append; *n = the detections in the store; Y355_ERANGE as y355_apeval_compute documents it
int ap_store_count(y355_apeval *e, long long *n);
// e->khi = the score keys (ascending key = descending score, NaN last), e->perm[0] = identity, e->cur = 0; with rank:
// w0_out[i] = rank[image of entry i] << AP_POS_BITS | position; h[2..7] = OR / AND of w0 (the store's own word without rank), of the
// score keys and of the classes.  Synchronous.
int ap_keys(y355_apeval *e, long long n, int quantize, const int *rank, unsigned long long *w0_out, unsigned long long h[8]);
// stable LSD radix sort of e->perm[e->cur] by the digits passes[0 .. np) (least significant first); a digit every key shares
// moves nothing.  Asynchronous on e->s; the result is e->perm[e->cur].
int ap_sort(y355_apeval *e, long long n, const unsigned long long *w0, const unsigned long long h[8], const ApPass *passes, int np);
// e->start[c] = the first rank of class c in e->perm[e->cur] (start[C] = n), for an order whose most significant key is the class
void ap_class_bounds(y355_apeval *e, long long n);

#ifdef __HIPCC__
__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_and(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v &= (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}

// inclusive scan over a workgroup of AP_SCORE_THREADS; sh: one slot per wave
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long *sh, unsigned long long *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = (unsigned long long)__shfl_up((long long)v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();
    if (lane == 63) sh[w] = v;
    __syncthreads();
    unsigned long long off = 0, all = 0;
    for (int k = 0; k < AP_SCORE_THREADS / 64; ++k) {
        if (k < w) off += sh[k];
        all += sh[k];
    }
    *total = all;
    return v + off;
}
__device__ __forceinline__ double block_scan_max(double v, double *sh, double *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o, 64);
        if (lane >= o) v = fmax(v, u);
    }
    __syncthreads();
    if (lane == 63) sh[w] = v;
    __syncthreads();
    double off = 0.0, all = 0.0;          // precisions are >= 0
    for (int k = 0; k < AP_SCORE_THREADS / 64; ++k) {
        if (k < w) off = fmax(off, sh[k]);
        all = fmax(all, sh[k]);
    }
    *total = all;
    return fmax(v, off);
}
#endif
