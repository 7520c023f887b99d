// yolo355 -- greedy per-class NMS for images with more than Y355_NMS_CAP (4096) candidates, up to 65 536: the route beside
// head_nms.hip's bin sort / pair walk / rounds, whose 12-bit edge endpoints and LDS tables end at 4096.  Same result by
// definition: for every candidate, "kept unless an EARLIER (score desc, anchor index asc) kept candidate of its class
// suppresses it", with the reference's predicate (suppresses_exact of head_nms.h) on every pair that is looked at; no pruning.
//
//   compact_large_kernel  one workgroup per image: the anchors at or above conf_thresh, in the reference's anchor-index
//                 order, into [B][lcap] arrays (position = rank); decides the image's route on the count: at most 4096 (and the
//                 route not forced) -> the same dbox / dscore / dcls / rcount compact_kernel writes, lcount = 0; more ->
//                 rcount = 0 (head_nms.hip's kernels see an image without candidates), lcount = the count;
//   sort_large_kernel     one workgroup per image: stable LSD radix sort, five 8-bit passes through global memory, of
//                 (~score bits, class << 16 | rank) by score digit 0..3, then by class: the list ends up class-major, inside a
//                 class by (score desc, rank asc) -- equal scores keep their rank order because every pass is stable, and the
//                 position of an element is computed from counts alone (no atomic decides an order);
//   resolve_large_kernel  NMS_LG workgroups per image, the classes dealt round-robin (per-class NMS never pairs two classes, so
//                 the classes are independent): a class's segment of the sorted list is walked in tiles of NMS_LT candidates,
//                 phase A  every candidate of the tile against the boxes kept from the segment's earlier tiles,
//                 phase B  the NMS_LT x NMS_LT "i suppresses j" bit matrix of the tile in LDS, then one wave scans the rows in
//                          order: a row whose candidate is still alive is kept and ORs its row into the removed set;
//                 the kept boxes are appended to the segment's kept list (global memory, read back by phase A);
//   emit_large_kernel     one workgroup per image: survivors by rank (= anchor-index order) into the padded outputs, the first
//                 max_det of them, like resolve_emit_kernel.
// Every kernel returns at once for an image with lcount = 0.  LDS: the bit matrix is 8 x 513 x 8 = 32.8 KB, the tile's boxes
// 8 KB: 41 KB of the CU's 160.  (A 1024-candidate tile would need 128 KB for the matrix alone.)
#include "head_nms.h"
#include <vector>

#define NMS_CAP Y355_NMS_CAP
#define NMS_LT 512               // candidates per tile
#define NMS_LW (NMS_LT / 64)      // 64-bit words per row of the tile's matrix
#define NMS_LG 8                  // resolve workgroups per image

__global__ __launch_bounds__(1024) void compact_large_kernel(const HeadParams p, const HeadWork wk) {
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = p.A;
    const int HW0 = p.lev[0].Hs * p.lev[0].Ws, N0 = HW0 * A;
    const int HW1 = p.nlev > 1 ? p.lev[1].Hs * p.lev[1].Ws : 0, N1 = N0 + HW1 * A;
    const int HW2 = p.nlev > 2 ? p.lev[2].Hs * p.lev[2].Ws : 0;
    const int N = N1 + HW2 * A;
    if (tid == 0) base_s = 0;
    __syncthreads();
    const float4 *rb = (const float4 *)wk.rbox + (size_t)b * wk.rstride;
    const float *rs = wk.rscore + (size_t)b * wk.rstride;
    const int *rc = wk.rcls + (size_t)b * wk.rstride;
    float4 *db = (float4 *)wk.dbox + (size_t)b * NMS_CAP;
    float *ds = wk.dscore + (size_t)b * NMS_CAP;
    int *dc = wk.dcls + (size_t)b * NMS_CAP;
    float4 *lb = (float4 *)wk.lbox + (size_t)b * wk.lcap;
    float *ls = wk.lscore + (size_t)b * wk.lcap;
    int *lc = wk.lcls + (size_t)b * wk.lcap;
    const bool small_too = !wk.lforce;               // the first CAP candidates also go where the small route reads them
    for (int n0 = 0; n0 < N; n0 += 1024) {
        const int n = n0 + tid;
        bool keep = false;
        int np = 0;
        if (n < N) {
            const int lv = (n >= N0 ? 1 : 0) + (n >= N1 ? 1 : 0);
            const int lbase = lv == 0 ? 0 : (lv == 1 ? N0 : N1), HWl = lv == 0 ? HW0 : (lv == 1 ? HW1 : HW2);
            const int cell = (n - lbase) / A, a = (n - lbase) % A;
            np = lbase + a * HWl + cell;                     // where decode_kernel put anchor n
            keep = rs[np] >= p.conf_thresh;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + before;
        if (keep && pos < wk.lcap) {
            const float4 bx = rb[np];
            const float sc = rs[np];
            const int cl = rc[np];
            lb[pos] = bx; ls[pos] = sc; lc[pos] = cl;
            if (small_too && pos < NMS_CAP) { db[pos] = bx; ds[pos] = sc; dc[pos] = cl; }
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; base_s += t; }
        __syncthreads();
    }
    if (tid == 0) {
        const int total = base_s;
        const bool big = wk.lforce || total > NMS_CAP;
        if (total > wk.lcap) wk.ovf[b] = 1;
        wk.rcount[b] = big ? 0 : total;
        wk.lcount[b] = big ? min(total, wk.lcap) : 0;
    }
}

// ---- sort_large_kernel.  A pass: digit histogram of the whole list, exclusive scan, then the list in tiles of 1024 in order:
// inside a wave an element's rank among the lanes with its digit comes from eight ballots, the waves' counts of a digit are
// laid one after the other behind the digit's running base.
__global__ __launch_bounds__(1024) void sort_large_kernel(const HeadWork wk) {
    __shared__ int hist[256];               // digit counts, then the running base of every digit
    __shared__ int wcnt[16][256];           // elements of the tile with digit d in wave w
    __shared__ int woff[16][256];           // where wave w's elements with digit d go
    __shared__ int wtot[4];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = wk.lcount[b];
    if (M == 0) return;
    const float *ls = wk.lscore + (size_t)b * wk.lcap;
    const int *lc = wk.lcls + (size_t)b * wk.lcap;
    uint2 *buf[2] = {wk.lsort + (size_t)b * wk.lcap, wk.lsort + ((size_t)B + b) * wk.lcap};
    for (int k = tid; k < 16 * 256; k += 1024) (&wcnt[0][0])[k] = 0;
    for (int pass = 0; pass < 5; ++pass) {
        const uint2 *src = buf[(pass & 1) ^ 1];          // pass 0 reads the candidates themselves
        uint2 *dst = buf[pass & 1];                      // 0 -> buf 0, 1 -> buf 1, ..., 4 -> buf 0
        auto load = [&](int i) -> uint2 {
            if (pass == 0) return make_uint2(~__float_as_uint(ls[i]), ((unsigned int)lc[i] << 16) | (unsigned int)i);
            return src[i];
        };
        // (8 bits of the class: Y355_NMS_MAX_CLASSES; 16 of the rank: Y355_NMS_MAX_CAP)
        auto digit = [&](uint2 kv) -> int { return pass < 4 ? (int)((kv.x >> (8 * pass)) & 0xffu) : (int)((kv.y >> 16) & 0xffu); };
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < M; i += 1024) atomicAdd(&hist[digit(load(i))], 1);      // counts: the same in any order
        __syncthreads();
        const int v = tid < 256 ? hist[tid] : 0;         // exclusive scan of the counts: waves 0 .. 3
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (tid < 256 && lane == 63) wtot[wave] = incl;
        __syncthreads();
        if (tid < 256) {
            int base = 0;
            for (int w = 0; w < wave; ++w) base += wtot[w];
            hist[tid] = base + incl - v;
        }
        __syncthreads();
        for (int t0 = 0; t0 < M; t0 += 1024) {
            const int i = t0 + tid;
            const bool valid = i < M;
            const uint2 kv = valid ? load(i) : make_uint2(0u, 0u);
            const int d = digit(kv);
            unsigned long long peers = __ballot(valid);
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool one = (d >> bit) & 1;
                const unsigned long long bm = __ballot(one);
                peers &= one ? bm : ~bm;
            }
            const int rank = __popcll(peers & ((1ull << lane) - 1ull));
            if (valid && rank == 0) wcnt[wave][d] = __popcll(peers);
            __syncthreads();
            if (tid < 256) {
                int run = hist[tid];
#pragma unroll
                for (int w = 0; w < 16; ++w) {
                    const int c = wcnt[w][tid];
                    woff[w][tid] = run;
                    wcnt[w][tid] = 0;
                    run += c;
                }
                hist[tid] = run;
            }
            __syncthreads();
            if (valid) dst[woff[wave][d] + rank] = kv;
        }
        __syncthreads();                                 // the next pass reads what this one wrote (one workgroup, one CU's L1)
    }
}

// ---- resolve_large_kernel: grid (NMS_LG, B)
__global__ __launch_bounds__(1024) void resolve_large_kernel(const HeadWork wk, const int C, const float thr) {
    __shared__ unsigned long long mask[NMS_LW][NMS_LT + 1];       // mask[w][i]: bit j - 64 w set: i suppresses j (j > i); + 1: the scan's eight lanes hit eight banks
    __shared__ float4 tbox[NMS_LT];
    __shared__ int trank[NMS_LT];
    __shared__ unsigned char dead[NMS_LT];
    __shared__ unsigned long long keptw[NMS_LW];
    __shared__ int seg[2];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int M = wk.lcount[b];
    if (M == 0) return;
    const uint2 *sorted = wk.lsort + (size_t)b * wk.lcap;
    const float4 *lb = (const float4 *)wk.lbox + (size_t)b * wk.lcap;
    float4 *kb = (float4 *)wk.lkbox + (size_t)b * wk.lcap;
    unsigned char *keep = wk.lkeep + (size_t)b * wk.lcap;
    for (int c = blockIdx.x; c < C; c += NMS_LG) {
        if (tid == 0 || tid == 64) {                     // the class's segment [first position with class >= c, with class >= c + 1)
            const unsigned int want = (unsigned int)(c + (tid ? 1 : 0));
            int lo = 0, hi = M;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((sorted[mid].y >> 16) < want) lo = mid + 1; else hi = mid;
            }
            seg[tid ? 1 : 0] = lo;
        }
        __syncthreads();
        const int s0 = seg[0], s1 = seg[1];
        float4 *kseg = kb + s0;                          // kept boxes of this class: at most as many as the segment holds
        int nk = 0;
        for (int t0 = s0; t0 < s1; t0 += NMS_LT) {
            const int nt = min(NMS_LT, s1 - t0);
            if (tid < NMS_LT) {
                dead[tid] = 0;
                if (tid < nt) {
                    const int r = (int)(sorted[t0 + tid].y & 0xffffu);
                    trank[tid] = r;
                    tbox[tid] = lb[r];
                }
            }
            __syncthreads();
            {   // phase A: two threads per candidate, each every other kept box of the earlier tiles
                const int j = tid & (NMS_LT - 1), half = tid >> 9;
                if (j < nt) {
                    const float4 bj = tbox[j];
                    const float aj = (bj.z - bj.x) * (bj.w - bj.y);
                    for (int k = half; k < nk; k += 2) {
                        const float4 bk = kseg[k];
                        if (suppresses_exact(bk, (bk.z - bk.x) * (bk.w - bk.y), bj, aj, thr)) { dead[j] = 1; break; }
                    }
                }
            }
            // phase B, the matrix: word (w, i) = 64 candidates j = 64 w .. 64 w + 63 against row i; a wave holds 64 rows of one w
            for (int wi = tid; wi < NMS_LW * NMS_LT; wi += 1024) {
                const int i = wi & (NMS_LT - 1), w = wi >> 9;
                unsigned long long bits = 0ull;
                if (i < nt && 64 * w + 63 > i) {
                    const float4 bi = tbox[i];
                    const float ai = (bi.z - bi.x) * (bi.w - bi.y);
                    const int j1 = min(64 * w + 64, nt);
                    for (int j = max(64 * w, i + 1); j < j1; ++j) {
                        const float4 bj = tbox[j];
                        if (suppresses_exact(bi, ai, bj, (bj.z - bj.x) * (bj.w - bj.y), thr)) bits |= 1ull << (j & 63);
                    }
                }
                mask[w][i] = bits;
            }
            __syncthreads();
            if (tid < 64) {                                // the scan: lane w < NMS_LW holds word w of the removed set
                unsigned long long removed = 0ull;
#pragma unroll
                for (int w = 0; w < NMS_LW; ++w) {
                    const int j = 64 * w + lane;
                    const unsigned long long m = __ballot(j >= nt || dead[j] != 0);
                    if (lane == w) removed = m;
                }
                const int wl = lane < NMS_LW ? lane : 0;
                for (int i0 = 0; i0 < nt; i0 += 8) {
                    unsigned long long rows[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) rows[u] = lane < NMS_LW ? mask[wl][i0 + u] : 0ull;
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int i = i0 + u;
                        const unsigned long long word = __shfl(removed, i >> 6, 64);
                        if (!((word >> (i & 63)) & 1ull)) removed |= rows[u];      // uniform: every lane reads the same word
                    }
                }
                if (lane < NMS_LW) keptw[lane] = ~removed;
            }
            __syncthreads();
            int total = 0;
            {
                const int j = tid < NMS_LT ? tid : 0;
                int before = 0;
#pragma unroll
                for (int w = 0; w < NMS_LW; ++w) {
                    const int pc = __popcll(keptw[w]);
                    if (w < (j >> 6)) before += pc;
                    total += pc;
                }
                if (tid < nt) {
                    const unsigned long long kw = keptw[j >> 6];
                    const bool kept = (kw >> (j & 63)) & 1ull;
                    keep[trank[j]] = kept ? 1 : 0;
                    if (kept) kseg[nk + before + __popcll(kw & ((1ull << (j & 63)) - 1ull))] = tbox[j];
                }
            }
            nk += total;
            __syncthreads();                             // tbox / dead are rewritten, the kept list is read by the next tile
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void emit_large_kernel(const HeadParams p, const HeadWork wk) {
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = wk.lcount[b];
    if (M == 0) return;
    if (tid == 0) base_s = 0;
    __syncthreads();
    const float4 *lb = (const float4 *)wk.lbox + (size_t)b * wk.lcap;
    const float *ls = wk.lscore + (size_t)b * wk.lcap;
    const int *lc = wk.lcls + (size_t)b * wk.lcap;
    const unsigned char *keep = wk.lkeep + (size_t)b * wk.lcap;
    float4 *ob = (float4 *)p.out_box + (size_t)b * p.max_det;
    float *os = p.out_score + (size_t)b * p.max_det;
    int *oc = p.out_cls + (size_t)b * p.max_det;
    for (int r0 = 0; r0 < M; r0 += 1024) {
        const int r = r0 + tid;
        const bool k = r < M && keep[r] != 0;
        const unsigned long long m = __ballot(k);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base_s;
        for (int w = 0; w < wave; ++w) off += wsum[w];
        const int pos = off + before;
        if (k && pos < p.max_det) { ob[pos] = lb[r]; os[pos] = ls[r]; oc[pos] = lc[r]; }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; base_s += t; }
        __syncthreads();
    }
    if (tid == 0) {
        p.out_count[b] = min(base_s, p.max_det);
        wk.count[b] = M;                                  // diagnostics: the image's candidates (its edge count stays 0)
    }
}

void y355_launch_compact_large(const HeadParams &p, const HeadWork &wk, int batch, hipStream_t s) {
    hipLaunchKernelGGL(compact_large_kernel, dim3(batch), dim3(1024), 0, s, p, wk);
}

void y355_launch_nms_large(const HeadParams &p, const HeadWork &wk, int batch, hipStream_t s) {
    // (p.C <= Y355_NMS_MAX_CLASSES: y355_create, y355_net_create and y355_head_f32_ex refuse A * (5 + C) > 256 with Y355_EINVAL)
    hipLaunchKernelGGL(sort_large_kernel, dim3(batch), dim3(1024), 0, s, wk);
    hipLaunchKernelGGL(resolve_large_kernel, dim3(NMS_LG, batch), dim3(1024), 0, s, wk, p.C, p.nms_thresh);
    hipLaunchKernelGGL(emit_large_kernel, dim3(batch), dim3(1024), 0, s, p, wk);
}
