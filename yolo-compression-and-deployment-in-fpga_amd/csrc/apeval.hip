// yolo355 -- VOC mAP on the GPU behind the y355_apeval_* C ABI (include/yolo355.h): the step that follows the evaluators' loops,
// write_voc_results_file + voc_eval + voc_ap of utils/vocapi_evaluator_mask.py:140-336 (utils/vocapi_evaluator.py alike), for
// detections that never leave the device.  DESIGN.md section 6c has the contract (quantisation, rank order, matching, curve, AP).
//
//   append   one batch of engine outputs -> records (image << 20 | position, class, raw score, raw box) in a device store; the slot
//            comes from one wave-aggregated atomic, so batches may arrive from several streams and in any order
//   rank     keys (class, score_q descending, image, position) and a stable LSD radix sort of a permutation, 8 bits per pass
//            (histogram per 1024-key tile, a scan per digit, stable scatter); passes whose digit is the same in every key are skipped
//   match    one thread per detection: float64 overlaps in the reference's operation order against the image's boxes of the class,
//            np.max / np.argmax semantics; the reference's sequential `det` marks are an atomicMin of the rank per ground-truth box
//            (the first detection in rank order that matches a box is its true positive, every later one a false positive)
//   score    one workgroup per class: inclusive scans of the flags, rec / prec, the reverse running maximum, the eleven thresholds
//            or the envelope sum
// The handle, the sort's entry points (ap_keys / ap_sort / ap_class_bounds) and the workgroup scans are in apeval_shared.h:
// cocoeval.hip scores the same store the COCO way.
#include "apeval_shared.h"
#include "handle_core.h"

#include <cfloat>
#include <cmath>

namespace {
// ---- append: one workgroup per image of the batch
__global__ void __launch_bounds__(256) ap_append_kernel(const float *boxes, const float *scores, const int *cls, const int *count, int first_image,
                                                        int max_det, int C, long long cap, unsigned long long *ctr, unsigned long long *imgpos,
                                                        uint8_t *scls, float *sscore, float *sbox) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int n = min(max(count[b], 0), max_det);
    const size_t row = (size_t)b * max_det;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        int c = 0;
        bool ok = false, bad = false;
        if (i < n) {
            c = cls[row + i];
            ok = c >= 0 && c < C;
            bad = !ok;
        }
        const unsigned long long m = __ballot(ok), mb = __ballot(bad);
        unsigned long long base = 0;
        if (lane == 0) {
            if (m) base = atomicAdd(&ctr[0], (unsigned long long)__popcll(m));
            if (mb) atomicAdd(&ctr[1], (unsigned long long)__popcll(mb));
        }
        base = (unsigned long long)__shfl((long long)base, 0, 64);
        if (ok) {
            const unsigned long long slot = base + __popcll(m & ((1ull << lane) - 1));
            if (slot < (unsigned long long)cap) {          // past the capacity: counted above, never stored
                imgpos[slot] = ((unsigned long long)(first_image + b) << AP_POS_BITS) | (unsigned int)i;
                scls[slot] = (uint8_t)c;
                sscore[slot] = scores[row + i];
                const float *bp = boxes + 4 * (row + i);      // the caller's buffer: no alignment assumed
                ((float4 *)sbox)[slot] = make_float4(bp[0], bp[1], bp[2], bp[3]);
            }
        }
    }
}

__device__ __forceinline__ double ap_score_q(float s, int quantize) {
    return quantize ? rint((double)s * 1000.0) / 1000.0 : (double)s;
}
__device__ __forceinline__ double ap_coord_q(float v, int quantize) {
    return quantize ? rint((double)(v + 1.0f) * 10.0) / 10.0 : (double)v;
}

// ---- keys: khi ascending = score_q descending (NaN last, as np.argsort(-confidence) places it); OR / AND of every key word
// with rank: the word that is sorted (and reduced) is w0[i] = rank[image] << AP_POS_BITS | position instead of the store's own
__global__ void __launch_bounds__(256) ap_keys_kernel(long long n, int quantize, const float *sscore, const unsigned long long *imgpos,
                                                      const uint8_t *scls, unsigned long long *khi, unsigned int *perm, unsigned long long *ctr,
                                                      const int *rank, unsigned long long *w0) {
    unsigned long long lo_or = 0, lo_and = ~0ull, hi_or = 0, hi_and = ~0ull, c_or = 0, c_and = ~0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double q = ap_score_q(sscore[i], quantize) + 0.0;           // -0.0 -> +0.0: equal scores, equal keys
        unsigned long long k;
        if (q != q) {
            k = ~0ull;
        } else {
            const unsigned long long u = (unsigned long long)__double_as_longlong(q);
            k = ~((u >> 63) ? ~u : (u | 0x8000000000000000ull));
        }
        khi[i] = k;
        perm[i] = (unsigned int)i;
        unsigned long long ip = imgpos[i];
        if (rank) {
            ip = ((unsigned long long)rank[ip >> AP_POS_BITS] << AP_POS_BITS) | (ip & ((1ull << AP_POS_BITS) - 1));
            w0[i] = ip;
        }
        const unsigned long long cc = scls[i];
        lo_or |= ip, lo_and &= ip, hi_or |= k, hi_and &= k, c_or |= cc, c_and &= cc;
    }
    lo_or = wave_or(lo_or), hi_or = wave_or(hi_or), c_or = wave_or(c_or);
    lo_and = wave_and(lo_and), hi_and = wave_and(hi_and), c_and = wave_and(c_and);
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&ctr[2], lo_or), atomicAnd(&ctr[3], lo_and);
        atomicOr(&ctr[4], hi_or), atomicAnd(&ctr[5], hi_and);
        atomicOr(&ctr[6], c_or), atomicAnd(&ctr[7], c_and);
    }
}

// the digit `pass` (ApPass) of the key of store entry e
__device__ __forceinline__ unsigned int ap_digit(ApPass pass, unsigned int e, const unsigned long long *imgpos, const unsigned long long *khi,
                                                 const uint8_t *scls) {
    if (pass.src == 0) return (unsigned int)(imgpos[e] >> pass.shift) & pass.mask;
    if (pass.src == 1) return (unsigned int)(khi[e] >> pass.shift) & pass.mask;
    return scls[e];
}

__global__ void __launch_bounds__(256) ap_hist_kernel(long long n, ApPass pass, int tiles, const unsigned int *perm, const unsigned long long *imgpos,
                                                      const unsigned long long *khi, const uint8_t *scls, unsigned int *hist) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * AP_TILE;
#pragma unroll
    for (int r = 0; r < AP_TILE / 256; ++r) {
        const long long i = t0 + r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&h[ap_digit(pass, perm[i], imgpos, khi, scls)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of every digit's row hist[d][0 .. tiles) in place, one workgroup per digit; tot[d] = the row's sum.  The scatter
// adds the sum of the smaller digits' totals itself, so no workgroup ever walks all 256 * tiles counters
__global__ void __launch_bounds__(256) ap_scan_kernel(unsigned int *hist, int tiles, unsigned int *tot) {
    __shared__ unsigned int wsum[4];
    unsigned int *row = hist + (size_t)blockIdx.x * tiles;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int carry = 0;
    for (int i0 = 0; i0 < tiles; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const unsigned int v = i < tiles ? row[i] : 0u;
        unsigned int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned int u = (unsigned int)__shfl_up((int)incl, o, 64);
            if (lane >= o) incl += u;
        }
        __syncthreads();
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        unsigned int off = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < w) off += wsum[k];
            all += wsum[k];
        }
        if (i < tiles) row[i] = carry + off + incl - v;
        carry += all;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// stable scatter of one tile: wave w owns keys [256 w, 256 w + 256) of the tile and walks them 64 at a time in order
__global__ void __launch_bounds__(256) ap_scatter_kernel(long long n, ApPass pass, int tiles, const unsigned int *perm_in, unsigned int *perm_out,
                                                         const unsigned long long *imgpos, const unsigned long long *khi, const uint8_t *scls,
                                                         const unsigned int *hist, const unsigned int *tot) {
    __shared__ unsigned int wcnt[4][256];
    __shared__ unsigned int dbase[256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long t0 = (long long)blockIdx.x * AP_TILE + w * 256;
#pragma unroll
    for (int k = 0; k < 4; ++k) wcnt[k][threadIdx.x] = 0;
    __syncthreads();
    dbase[threadIdx.x] = tot[threadIdx.x];
    unsigned int e[4], d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = t0 + r * 64 + lane;
        e[r] = 0, d[r] = 0;
        if (i < n) {
            e[r] = perm_in[i];
            d[r] = ap_digit(pass, e[r], imgpos, khi, scls);
            atomicAdd(&wcnt[w][d[r]], 1u);
        }
    }
    __syncthreads();
    {   // thread = digit: the first output slot of every wave's keys of that digit = the keys of smaller digits (all tiles) + the
        // keys of this digit in earlier tiles + those of this tile's earlier waves
        unsigned int base = hist[(size_t)threadIdx.x * tiles + blockIdx.x];
        for (int k = 0; k < (int)threadIdx.x; ++k) base += dbase[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned int c = wcnt[k][threadIdx.x];
            wcnt[k][threadIdx.x] = base;
            base += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long i = t0 + r * 64 + lane;
        const bool valid = i < n;
        unsigned long long m = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d[r] >> bit) & 1u;
            const unsigned long long bb = __ballot(valid && one);
            m &= one ? bb : ~bb;
        }
        unsigned int base = 0;
        const int leader = valid ? __ffsll((long long)m) - 1 : 0;
        if (valid && lane == leader) {
            base = wcnt[w][d[r]];
            wcnt[w][d[r]] = base + (unsigned int)__popcll(m);
        }
        base = (unsigned int)__shfl((int)base, leader, 64);
        if (valid) perm_out[base + (unsigned int)__popcll(m & ((1ull << lane) - 1))] = e[r];
        __syncthreads();      // the next round reads the counters this one advanced
    }
}

// start[c] = first rank of class c (start[C] = n) from the sorted order
__global__ void __launch_bounds__(256) ap_bounds_kernel(long long n, int C, const unsigned int *perm, const uint8_t *scls, long long *start) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    const int a = r == 0 ? -1 : (int)scls[perm[r - 1]], b = r == n ? C : (int)scls[perm[r]];
    for (int c = a + 1; c <= b; ++c) start[c] = r;
}

// np.maximum / np.minimum (a NaN operand gives NaN)
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : b != b ? b : a > b ? a : b; }
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : b != b ? b : a < b ? a : b; }

// jm[r] = the ground-truth box detection r (rank order) claims, -1 = false positive, -2 = matched a difficult box
__global__ void __launch_bounds__(256) ap_match_kernel(long long n, double ovthresh, int quantize, const unsigned int *perm,
                                                       const unsigned long long *imgpos, const uint8_t *scls, const float *sbox, const int *gt_off,
                                                       const float *gt_box, const int *gt_cls, const uint8_t *gt_diff, unsigned int *gt_first,
                                                       int *jm) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const unsigned int e = perm[r];
    const int img = (int)(imgpos[e] >> AP_POS_BITS), c = scls[e];
    const float4 bf = ((const float4 *)sbox)[e];
    const double bx1 = ap_coord_q(bf.x, quantize), by1 = ap_coord_q(bf.y, quantize), bx2 = ap_coord_q(bf.z, quantize),
                 by2 = ap_coord_q(bf.w, quantize);
    const double barea = (bx2 - bx1) * (by2 - by1);
    double ovmax = -INFINITY;
    int jmax = -1;
    bool nan = false;
    for (int g = gt_off[img], g1 = gt_off[img + 1]; g < g1; ++g) {
        if (gt_cls[g] != c) continue;
        const float4 gf = ((const float4 *)gt_box)[g];
        const double gx1 = gf.x, gy1 = gf.y, gx2 = gf.z, gy2 = gf.w;
        const double iw = np_max(np_min(gx2, bx2) - np_max(gx1, bx1), 0.0), ih = np_max(np_min(gy2, by2) - np_max(gy1, by1), 0.0);
        const double inters = iw * ih;
        const double uni = barea + (gx2 - gx1) * (gy2 - gy1) - inters;
        const double ov = inters / uni;
        if (ov != ov) nan = true;
        if (ov > ovmax) ovmax = ov, jmax = g;
    }
    int res = -1;
    if (!nan && jmax >= 0 && ovmax > ovthresh) {
        if (gt_diff[jmax]) {
            res = -2;
        } else {
            res = jmax;
            atomicMin(&gt_first[jmax], (unsigned int)r);
        }
    }
    jm[r] = res;
}

__global__ void __launch_bounds__(256) ap_flag_kernel(long long n, const int *jm, const unsigned int *gt_first, uint8_t *flag) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int j = jm[r];
    flag[r] = j == -2 ? 0 : j == -1 ? 2 : gt_first[j] == (unsigned int)r ? 1 : 2;
}

// one workgroup per class: curve (rec, prec in rank order) and AP
__global__ void __launch_bounds__(AP_SCORE_THREADS) ap_score_kernel(int metric, const long long *start, const int *npos, const uint8_t *flag,
                                                                    double *rec, double *prec, double *ap) {
    __shared__ unsigned long long sh_u[AP_SCORE_THREADS / 64];
    __shared__ double sh_d[AP_SCORE_THREADS / 64];
    __shared__ double red[12][AP_SCORE_THREADS / 64];
    const int c = blockIdx.x;
    const long long s0 = start[c], nd = start[c + 1] - s0;
    if (nd == 0) {
        if (threadIdx.x == 0) ap[c] = -1.0;                 // no detection of the class: voc_eval's else branch
        return;
    }
    const double dnpos = (double)npos[c];
    // forward: inclusive sums of TP (high word) and FP (low word), rec = tp / npos, prec = tp / max(tp + fp, eps)
    unsigned long long carry = 0;
    for (long long i0 = 0; i0 < nd; i0 += AP_SCORE_THREADS) {
        const long long i = i0 + threadIdx.x;
        const int f = i < nd ? flag[s0 + i] : 0;
        unsigned long long tot;
        const unsigned long long v = carry + block_scan_add(f == 1 ? (1ull << 32) : f == 2 ? 1ull : 0ull, sh_u, &tot);
        carry += tot;
        if (i < nd) {
            const double tp = (double)(v >> 32), fp = (double)(v & 0xffffffffull);
            rec[s0 + i] = tp / dnpos;
            prec[s0 + i] = tp / fmax(tp + fp, DBL_EPSILON);
        }
    }
    __syncthreads();
    // backward: reverse running maximum of prec; the eleven thresholds, or the terms of the envelope sum
    double pm[11], acc = 0.0, cmax = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) pm[k] = 0.0;
    for (long long i0 = 0; i0 < nd; i0 += AP_SCORE_THREADS) {
        const long long i = nd - 1 - (i0 + threadIdx.x);
        const bool in = i >= 0;
        const double p = in ? prec[s0 + i] : 0.0, rc = in ? rec[s0 + i] : 0.0;
        if (metric == Y355_AP_VOC07) {
            if (in) {
#pragma unroll
                for (int k = 0; k < 11; ++k)
                    if (rc >= (double)k * 0.1) pm[k] = fmax(pm[k], p);
            }
        } else {
            double tot;
            const double env = fmax(cmax, block_scan_max(p, sh_d, &tot));
            cmax = fmax(cmax, tot);
            if (in) {
                const double prev = i == 0 ? 0.0 : rec[s0 + i - 1];
                if (rc != prev) acc += (rc - prev) * env;
            }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (metric == Y355_AP_VOC07) {
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            double v = pm[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
            if (lane == 0) red[k][w] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0;
            for (int k = 0; k < 11; ++k) {
                double v = 0.0;
                for (int j = 0; j < AP_SCORE_THREADS / 64; ++j) v = fmax(v, red[k][j]);
                a = a + v / 11.0;
            }
            ap[c] = a;
        }
    } else {
        double v = acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[0][w] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double a = 0.0;
            for (int j = 0; j < AP_SCORE_THREADS / 64; ++j) a += red[0][j];
            const double last = rec[s0 + nd - 1];          // the sentinel pair (mrec 1, mpre 0)
            if (1.0 != last) a += (1.0 - last) * 0.0;
            ap[c] = a;
        }
    }
}

int ap_check_add(y355_apeval *e, int first_image, int batch, int max_det, const void *a, const void *b, const void *c, const void *d) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!a || !b || !c || !d) return y355_fail(Y355_EINVAL, "null detection buffer");
    if (batch < 1 || first_image < 0 || (long long)first_image + batch > e->num_images)
        return y355_fail(Y355_EINVAL, "images first_image .. first_image + batch - 1 are not inside 0 .. num_images - 1");
    if (max_det < 1 || max_det > (1 << AP_POS_BITS)) return y355_fail(Y355_EINVAL, "max_det outside 1 .. 2^20");
    return 0;
}
void ap_launch_append(y355_apeval *e, int first_image, int batch, int max_det, const float *boxes, const float *scores, const int32_t *cls,
                      const int32_t *count, hipStream_t s) {
    hipLaunchKernelGGL(ap_append_kernel, dim3(batch), dim3(256), 0, s, boxes, scores, cls, count, first_image, max_det, e->C, e->cap, e->ctr,
                       e->d_imgpos, e->d_cls, e->d_score, e->d_box);
}
}  // namespace

int ap_store_count(y355_apeval *e, long long *n) {
    unsigned long long h[2];
    HIPCHK(hipStreamSynchronize(e->s));
    HIPCHK(hipMemcpy(h, e->ctr, sizeof h, hipMemcpyDeviceToHost));
    if (h[1]) return y355_fail(Y355_ERANGE, std::to_string(h[1]) + " detections carry a class index outside 0 .. " + std::to_string(e->C - 1));
    if (h[0] > (unsigned long long)e->cap)
        return y355_fail(Y355_ERANGE, std::to_string(h[0]) + " detections were added, the store holds max_dets = " + std::to_string(e->cap));
    *n = (long long)h[0];
    return 0;
}

int ap_keys(y355_apeval *e, long long n, int quantize, const int *rank, unsigned long long *w0_out, unsigned long long h[8]) {
    hipStream_t s = e->s;
    const unsigned long long init[6] = {0, ~0ull, 0, ~0ull, 0, ~0ull};
    HIPCHK(hipMemcpyAsync(e->ctr + 2, init, sizeof init, hipMemcpyHostToDevice, s));
    const int nb = (int)((n + 255) / 256);
    hipLaunchKernelGGL(ap_keys_kernel, dim3(nb < 256 ? nb : 256), dim3(256), 0, s, n, quantize, e->d_score, e->d_imgpos, e->d_cls, e->khi, e->perm[0],
                       e->ctr, rank, w0_out);
    HIPCHK(hipMemcpyAsync(h, e->ctr, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    e->cur = 0;
    return 0;
}

int ap_sort(y355_apeval *e, long long n, const unsigned long long *w0, const unsigned long long h[8], const ApPass *passes, int np) {
    hipStream_t s = e->s;
    const int tiles = (int)((n + AP_TILE - 1) / AP_TILE);
    int cur = e->cur;
    for (int p = 0; p < np; ++p) {                        // a digit every key shares moves nothing
        const ApPass pass = passes[p];
        const unsigned long long diff = (h[2 + 2 * pass.src] ^ h[3 + 2 * pass.src]) >> pass.shift;
        if (!(diff & pass.mask)) continue;
        hipLaunchKernelGGL(ap_hist_kernel, dim3(tiles), dim3(256), 0, s, n, pass, tiles, e->perm[cur], w0, e->khi, e->d_cls, e->hist);
        hipLaunchKernelGGL(ap_scan_kernel, dim3(256), dim3(256), 0, s, e->hist, tiles, e->dtot);
        hipLaunchKernelGGL(ap_scatter_kernel, dim3(tiles), dim3(256), 0, s, n, pass, tiles, e->perm[cur], e->perm[cur ^ 1], w0, e->khi, e->d_cls,
                           e->hist, e->dtot);
        cur ^= 1;
    }
    e->cur = cur;
    HIPCHK(hipGetLastError());
    return 0;
}

void ap_class_bounds(y355_apeval *e, long long n) {
    hipLaunchKernelGGL(ap_bounds_kernel, dim3((int)((n + 256) / 256)), dim3(256), 0, e->s, n, e->C, e->perm[e->cur], e->d_cls, e->start);
}

// ---- the handle's device memory (apeval_shared.h)
int ap_buffers(y355_apeval *e) {
    const size_t n = (size_t)e->cap, tiles = (n + AP_TILE - 1) / AP_TILE, C = (size_t)e->C;
    DevOwner &o = e->own;
    int rc = y355_dev_get(o, &e->ctr, 8);
    rc = rc ? rc : y355_dev_get_all(o, n, &e->d_imgpos, &e->d_cls, &e->d_score, &e->khi, &e->perm[0], &e->perm[1], &e->jm, &e->flag, &e->rec, &e->prec);
    rc = rc ? rc : y355_dev_get(o, &e->d_box, 4 * n);
    rc = rc ? rc : y355_dev_get(o, &e->hist, 256 * tiles);
    rc = rc ? rc : y355_dev_get(o, &e->dtot, 256);
    rc = rc ? rc : y355_dev_get(o, &e->start, C + 1);
    rc = rc ? rc : y355_dev_get(o, &e->ap, C);
    if (rc) ap_close(e);
    return rc;
}

int ap_check_gt(const y355_apeval *e, const int32_t *offsets, const int32_t *cls, bool have_arrays, long long *n) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!offsets) return y355_fail(Y355_EINVAL, "null offsets");
    if (offsets[0] != 0) return y355_fail(Y355_EINVAL, "offsets[0] must be 0");
    for (int i = 0; i < e->num_images; ++i)
        if (offsets[i + 1] < offsets[i]) return y355_fail(Y355_EINVAL, "offsets must not decrease");
    *n = offsets[e->num_images];
    if (*n > 0 && !have_arrays) return y355_fail(Y355_EINVAL, "null ground-truth array");
    for (long long g = 0; g < *n; ++g)
        if (cls[g] < 0 || cls[g] >= e->C) return y355_fail(Y355_EINVAL, "ground-truth class outside 0 .. num_classes - 1");
    return 0;
}

int ap_set_gt(y355_apeval *e, const int32_t *offsets, const float *boxes, const int32_t *cls, const uint8_t *difficult) {
    const size_t n = (size_t)offsets[e->num_images], ni = (size_t)e->num_images + 1;
    DevOwner &o = e->own;
    e->have_gt = false, e->have_curve = false, e->n_gt = 0;
    y355_dev_drop(o, &e->gt_off, &e->gt_box, &e->gt_cls, &e->gt_diff, &e->gt_first);
    int rc = y355_dev_get(o, &e->gt_off, ni);
    rc = rc ? rc : y355_dev_get(o, &e->gt_box, 4 * n);
    rc = rc ? rc : y355_dev_get_all(o, n, &e->gt_cls, &e->gt_diff, &e->gt_first);
    rc = rc ? rc : o.mem.upload(e->gt_off, offsets, ni * sizeof(int32_t), e->s);
    if (n > 0) {
        rc = rc ? rc : o.mem.upload(e->gt_box, boxes, 4 * n * sizeof(float), e->s);
        rc = rc ? rc : o.mem.upload(e->gt_cls, cls, n * sizeof(int32_t), e->s);
        rc = rc ? rc : o.mem.upload(e->gt_diff, difficult, n, e->s);
    }
    if (rc) return rc;                                    // (what it took stays the handle's: the next set_gt or the close returns it)
    e->npos.assign(e->C, 0);
    for (size_t g = 0; g < n; ++g)
        if (!difficult[g]) ++e->npos[cls[g]];
    e->n_gt = (long long)n, e->have_gt = true;
    return 0;
}

void ap_close(y355_apeval *e) {
    y355_dev_release_all(e->own);
    delete e->coco;
    y355_apeval z;                                        // every pointer null, nothing ready
    z.device = e->device, z.C = e->C, z.num_images = e->num_images, z.cap = e->cap, z.s = e->s, z.ev = e->ev, z.own.mem = e->own.mem;
    *e = std::move(z);
}

extern "C" {

int y355_apeval_create(int device_id, int num_classes, int num_images, int64_t max_dets, y355_apeval **out) {
    if (!out) return y355_fail(Y355_EINVAL, "null argument");
    *out = nullptr;
    if (device_id < 0) return y355_fail(Y355_EINVAL, "device_id < 0");
    if (num_classes < 1 || num_classes > 256) return y355_fail(Y355_EINVAL, "num_classes outside 1 .. 256");
    if (num_images < 1 || num_images > (1 << 24)) return y355_fail(Y355_EINVAL, "num_images outside 1 .. 2^24");
    if (max_dets < 1 || max_dets > ((int64_t)1 << 27)) return y355_fail(Y355_EINVAL, "max_dets outside 1 .. 2^27");
    HIPCHK(hipSetDevice(device_id));
    y355_apeval *e = new y355_apeval;
    e->device = device_id, e->C = num_classes, e->num_images = num_images, e->cap = max_dets, e->own.mem = y355_hip_mem();
    int rc = 0;
    if (hipStreamCreateWithFlags(&e->s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess)
        rc = y355_fail(Y355_EHIP, "hipStreamCreate / hipEventCreate failed");
    rc = rc ? rc : ap_buffers(e);
    if (!rc && (hipMemsetAsync(e->ctr, 0, 8 * sizeof(unsigned long long), e->s) != hipSuccess || hipStreamSynchronize(e->s) != hipSuccess))
        rc = y355_fail(Y355_EHIP, "hipMemset failed");
    if (rc) return y355_core_unwind(rc, [e] { y355_apeval_destroy(e); });
    *out = e;
    return 0;
}

void y355_apeval_destroy(y355_apeval *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->s) (void)hipStreamSynchronize(e->s);
    ap_close(e);
    if (e->ev) (void)hipEventDestroy(e->ev);
    if (e->s) (void)hipStreamDestroy(e->s);
    delete e;
}

int y355_apeval_set_gt(y355_apeval *e, const int32_t *offsets, const float *boxes, const int32_t *cls, const uint8_t *difficult) {
    long long n = 0;
    if (int rc = ap_check_gt(e, offsets, cls, boxes && cls && difficult, &n)) return rc;
    if (int rc = ap_enter(e)) return rc;
    HIPCHK(hipStreamSynchronize(e->s));                   // nothing in flight reads the arrays that go
    return ap_set_gt(e, offsets, boxes, cls, difficult);
}

int y355_apeval_add(y355_apeval *e, int first_image, int batch, int max_det, const float *boxes_dev, const float *scores_dev,
                    const int32_t *cls_dev, const int32_t *count_dev, void *after_stream) {
    if (int rc = ap_check_add(e, first_image, batch, max_det, boxes_dev, scores_dev, cls_dev, count_dev)) return rc;
    if (int rc = ap_mutate(e)) return rc;
    if (!after_stream) {
        ap_launch_append(e, first_image, batch, max_det, boxes_dev, scores_dev, cls_dev, count_dev, e->s);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // on the caller's stream, behind the producer of the buffers; the handle's stream then waits for it (reset and compute
    // leave nothing of their own running on the handle's stream, so the append needs no wait the other way)
    hipStream_t cs = after_stream == Y355_AP_NULL_STREAM ? (hipStream_t) nullptr : (hipStream_t)after_stream;
    ap_launch_append(e, first_image, batch, max_det, boxes_dev, scores_dev, cls_dev, count_dev, cs);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev, cs));
    HIPCHK(hipStreamWaitEvent(e->s, e->ev, 0));
    return 0;
}

int y355_apeval_add_host(y355_apeval *e, int first_image, int batch, int max_det, const float *boxes, const float *scores, const int32_t *cls,
                         const int32_t *count) {
    if (int rc = ap_check_add(e, first_image, batch, max_det, boxes, scores, cls, count)) return rc;
    if (int rc = ap_mutate(e)) return rc;
    const size_t m = (size_t)batch * max_det, need = m * 24 + (size_t)batch * 4;
    if (need > e->stage_bytes) HIPCHK(hipStreamSynchronize(e->s));       // (the buffer that goes is idle)
    if (int rc = ap_stage(e, need)) return rc;
    char *p = e->stage;
    float *db = (float *)p, *ds = (float *)(p + m * 16);
    int32_t *dc = (int32_t *)(p + m * 20), *dn = (int32_t *)(p + m * 24);
    HIPCHK(hipMemcpyAsync(db, boxes, m * 16, hipMemcpyHostToDevice, e->s));
    HIPCHK(hipMemcpyAsync(ds, scores, m * 4, hipMemcpyHostToDevice, e->s));
    HIPCHK(hipMemcpyAsync(dc, cls, m * 4, hipMemcpyHostToDevice, e->s));
    HIPCHK(hipMemcpyAsync(dn, count, (size_t)batch * 4, hipMemcpyHostToDevice, e->s));
    ap_launch_append(e, first_image, batch, max_det, db, ds, dc, dn, e->s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->s));
    return 0;
}

int y355_apeval_reset(y355_apeval *e) {
    if (int rc = ap_check_handle(e)) return rc;
    if (int rc = ap_mutate(e)) return rc;
    HIPCHK(hipMemsetAsync(e->ctr, 0, 8 * sizeof(unsigned long long), e->s));      // behind every append so far
    HIPCHK(hipStreamSynchronize(e->s));
    return 0;
}

int y355_apeval_compute(y355_apeval *e, double ovthresh, int metric, int quantize, double *ap, int32_t *npos, int64_t *ndet, double *mean_ap) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!ap || !npos || !ndet || !mean_ap) return y355_fail(Y355_EINVAL, "null output");
    if (metric != Y355_AP_VOC07 && metric != Y355_AP_AREA) return y355_fail(Y355_EINVAL, "metric: Y355_AP_VOC07 or Y355_AP_AREA");
    if (quantize != Y355_AP_Q_VOCFILE && quantize != Y355_AP_Q_NONE) return y355_fail(Y355_EINVAL, "quantize: Y355_AP_Q_VOCFILE or Y355_AP_Q_NONE");
    if (ovthresh != ovthresh) return y355_fail(Y355_EINVAL, "ovthresh is NaN");
    if (!e->have_gt) return y355_fail(Y355_ENOTREADY, "no ground truth: call y355_apeval_set_gt first");
    if (int rc = ap_enter(e)) return rc;
    e->have_curve = false;
    hipStream_t s = e->s;
    long long n = 0;
    if (int rc = ap_store_count(e, &n)) return rc;
    const int C = e->C;
    const int q = quantize == Y355_AP_Q_VOCFILE;          // the kernels' flag: 1 = round as the results file does
    e->h_start.assign(C + 1, 0);
    if (n > 0) {
        unsigned long long h[8];
        if (int rc = ap_keys(e, n, q, nullptr, nullptr, h)) return rc;
        ApPass passes[17];                                // image / position bytes, score-key bytes, the class
        for (int p = 0; p < 17; ++p) passes[p] = ApPass{p < 8 ? 0 : p < 16 ? 1 : 2, p < 16 ? 8 * (p & 7) : 0, 255u};
        if (int rc = ap_sort(e, n, e->d_imgpos, h, passes, 17)) return rc;
        const int nb = (int)((n + 255) / 256), cur = e->cur;
        ap_class_bounds(e, n);
        if (e->n_gt > 0) HIPCHK(hipMemsetAsync(e->gt_first, 0xff, (size_t)e->n_gt * sizeof(unsigned int), s));
        hipLaunchKernelGGL(ap_match_kernel, dim3(nb), dim3(256), 0, s, n, ovthresh, q, e->perm[cur], e->d_imgpos, e->d_cls, e->d_box, e->gt_off,
                           e->gt_box, e->gt_cls, e->gt_diff, e->gt_first, e->jm);
        hipLaunchKernelGGL(ap_flag_kernel, dim3(nb), dim3(256), 0, s, n, e->jm, e->gt_first, e->flag);
        // npos travels through the (idle) histogram buffer's first C words
        HIPCHK(hipMemcpyAsync(e->hist, e->npos.data(), (size_t)C * sizeof(int32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ap_score_kernel, dim3(C), dim3(AP_SCORE_THREADS), 0, s, metric, e->start, (const int *)e->hist, e->flag, e->rec, e->prec,
                           e->ap);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ap, e->ap, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(e->h_start.data(), e->start, ((size_t)C + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        for (int c = 0; c < C; ++c) ap[c] = -1.0;
    }
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
        npos[c] = e->npos[c];
        ndet[c] = e->h_start[c + 1] - e->h_start[c];
        sum += ap[c];
    }
    *mean_ap = sum / (double)C;
    e->have_curve = true;
    return 0;
}

int y355_apeval_curve(y355_apeval *e, int cls, int64_t capacity, double *rec, double *prec, uint8_t *flag, int64_t *n) {
    if (int rc = ap_check_handle(e)) return rc;
    if (!n) return y355_fail(Y355_EINVAL, "null n");
    if (cls < 0 || cls >= e->C) return y355_fail(Y355_EINVAL, "class outside 0 .. num_classes - 1");
    if (capacity < 0) return y355_fail(Y355_EINVAL, "capacity < 0");
    if (!e->have_curve) return y355_fail(Y355_ENOTREADY, "no curve: y355_apeval_compute has not succeeded since the last add / reset");
    const long long s0 = e->h_start[cls], nd = e->h_start[cls + 1] - s0;
    *n = nd;
    const size_t m = (size_t)(nd < capacity ? nd : capacity);
    if (!m) return 0;
    if (int rc = ap_enter(e)) return rc;
    if (rec) HIPCHK(hipMemcpy(rec, e->rec + s0, m * sizeof(double), hipMemcpyDeviceToHost));
    if (prec) HIPCHK(hipMemcpy(prec, e->prec + s0, m * sizeof(double), hipMemcpyDeviceToHost));
    if (flag) HIPCHK(hipMemcpy(flag, e->flag + s0, m, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
