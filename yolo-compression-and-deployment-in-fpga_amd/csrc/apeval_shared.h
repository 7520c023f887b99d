// yolo355 -- what the two users of a y355_apeval handle share: the handle itself (device store of detection records, sort
// workspace), the entry points of the append store's radix sort (apeval.hip) and the workgroup scans.  apeval.hip scores a run the
// VOC way, cocoeval.hip the COCO way; DESIGN.md section 6c has both contracts.
#pragma once
#include "../../include/yolo355.h"
#include "y355_common.h"

#include <string>
#include <vector>

#define AP_POS_BITS 20            // position of a detection in its image's list: max_det <= 2^20
#define AP_TILE 1024              // keys per workgroup of a sort pass: 4 waves x 4 rounds x 64
#define AP_SCORE_THREADS 1024

struct y355_coco;                 // cocoeval.hip: the COCO ground truth, parameters and workspaces of a handle

struct y355_apeval {
    int device = 0, C = 0, num_images = 0;
    long long cap = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
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
    void *stage = nullptr;
    size_t stage_bytes = 0;
    // last compute
    bool have_curve = false;
    int cur = 0;
    std::vector<long long> h_start;
    y355_coco *coco = nullptr;
};

template <typename T> int ap_alloc(T **p, size_t count) {
    HIPCHK(hipMalloc((void **)p, (count ? count : 1) * sizeof(T)));
    return 0;
}
inline int ap_enter(y355_apeval *e) {
    HIPCHK(hipSetDevice(e->device));
    return 0;
}

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
// cocoeval.hip: frees e->coco (y355_apeval_destroy), forgets its last result (add / reset)
void y355_coco_destroy(y355_apeval *e);
void y355_coco_invalidate(y355_apeval *e);

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
