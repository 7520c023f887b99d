// yolo355 -- general-geometry implicit-GEMM convolution for gfx950 (utils/modules.py Conv2d / Conv2d_fuse*,
// backbone/darknet.py Conv_BN_LeakyReLU with any ksize / padding / stride / dilation), in the two arithmetic types of convg.hip:
//   bf16 : bf16 x bf16 -> fp32 on v_mfma_f32_16x16x32_bf16; bias + LeakyReLU(slope) [+ residual], bf16 or fp32 result
//   int8 : int8 x int8 -> int32 on v_mfma_i32_16x16x64_i8; t = acc * 2^shl + bias, t' = LeakyReLU / ReLU of t, written as int64
//          (no requantisation: the caller scales by 2^-F', exact)
//
// Mapping: GEMM rows = output pixels of the whole batch (BM per workgroup), columns = output channels (BN per workgroup),
// K = taps x 64-byte chunks of one input pixel -- a k-step is 32 bf16 or 64 int8 channels of one pixel at one tap, the byte
// layout of convg.hip, so the A/B fragments of both MFMA shapes are the same bytes (lane (g, j) holds 16 bytes of row/column j
// at k-offset 16 g).  K runs tap-major: ks = tap * nchunk + chunk.
//
// A stage is one tap and up to GK chunks.  Each staging thread owns one GEMM row for the whole tile: its output pixel's
// (iy0, ix0) = (oy * stride_h - pad_top, ox * stride_w - pad_left) is computed once; a stage adds the tap's (ky * dil_h,
// kx * dil_w).  A tap outside the input map is a PREDICATE: the load goes to an in-bounds address (the batch item's first
// chunk) and its value is replaced by zero -- no read ever leaves the tensor, whatever the pads.  The A rows of stage s + 1 are
// loaded into registers before the MFMAs of stage s and written to the other of two LDS slabs after them: one barrier per
// stage.  B fragments come from global memory (L2-resident, packed by y355_convgeom_pack), one k-step ahead.  Waits are the
// compiler's.
#include "y355_common.h"
#include "convg_shared.h"
#include <type_traits>

namespace {
constexpr int GK = 4;                     // 64-byte k-steps per stage (one tap) at most
constexpr int GROW = GK * 64 + 16;        // LDS bytes per A row: 16-byte pad, conflict-free ds_read_b128 across rows

template <bool BF, int WM, int WN, int MT, int NT>
__global__ __launch_bounds__(256) void convgeom_kernel(const ConvGeomParams p) {
    constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
    constexpr int TPR = 256 / BM;                 // staging threads per A row
    constexpr int SEGS = GK * 4 / TPR;            // 16-byte segments per staging thread and stage
    constexpr int SLAB = BM * GROW;
    static_assert(WM * WN == 4, "4 waves");
    static_assert(256 % BM == 0 && (GK * 4) % TPR == 0, "staging split");
    (void)BN;
    using ACC = MmaAcc<BF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int bid = y355_xcd_remap(blockIdx.x, gridDim.x);
    const int nb = bid % p.nblk;
    const int m0 = (bid / p.nblk) * BM;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 15, g = lane >> 4;
    const int nch = p.nchunk, ncg = (nch + GK - 1) / GK;
    const int taps = p.kh * p.kw;
    const int NS = taps * ncg, KS = taps * nch;

    // ---- staging role, fixed for the tile: row sr, segments [sq * SEGS, + SEGS)
    const int sr = tid % BM, sq = tid / BM;
    const bool srow = m0 + sr < p.M;
    int iy0, ix0;
    size_t pix0;                                  // pixel index of the batch item's halo origin
    {
        const int mm = srow ? m0 + sr : 0;
        const int ox = mm % p.Wo, t = mm / p.Wo;
        const int oy = t % p.Ho, b = t / p.Ho;
        iy0 = oy * p.sh - p.pt;
        ix0 = ox * p.sw - p.pl;
        pix0 = (size_t)b * (p.H + 2) * (p.W + 2);
    }
    v4i stg[SEGS];
    auto stage_load = [&](int s) {
        const int tap = s / ncg, cg = s - tap * ncg;
        const int ky = tap / p.kw, kx = tap - ky * p.kw;
        const int iy = iy0 + ky * p.dh, ix = ix0 + kx * p.dw;
        const bool ok = srow && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const size_t pix = ok ? pix0 + (size_t)(iy + 1) * (p.W + 2) + (ix + 1) : pix0;
        const char *src = p.in + pix * p.in_pb + cg * (GK * 64);
        const int kg = min(GK, nch - cg * GK);
#pragma unroll
        for (int u = 0; u < SEGS; ++u) {
            const int seg = sq * SEGS + u;
            const bool v = ok && (seg >> 2) < kg;
            const v4i x = *(const v4i *)(src + (v ? seg * 16 : 0));
            stg[u] = v ? x : (v4i){0, 0, 0, 0};
        }
    };
    auto stage_store = [&](char *slab) {
#pragma unroll
        for (int u = 0; u < SEGS; ++u) *(v4i *)(slab + sr * GROW + (sq * SEGS + u) * 16) = stg[u];
    };

    int abase[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) abase[m] = ((wm * MT + m) * 16 + li) * GROW + g * 16;

    ACC acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[m][t] = ACC{};

    const char *wp = p.w + ((size_t)nb * KS * WN + wn) * NT * 1024 + lane * 16;
    constexpr size_t WSTEP = (size_t)WN * NT * 1024;
    v4i bcur[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bcur[t] = *(const v4i *)(wp + t * 1024);
    int ksg = 0;
    auto kstep = [&](const char *slab, int ko) {
        const int nx = min(ksg + 1, KS - 1);
        v4i bnext[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bnext[t] = *(const v4i *)(wp + (size_t)nx * WSTEP + t * 1024);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const v4i a = *(const v4i *)(slab + abase[m] + ko);
#pragma unroll
            for (int t = 0; t < NT; ++t) mma_step<BF>(acc[m][t], a, bcur[t]);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) bcur[t] = bnext[t];
        ++ksg;
    };

    stage_load(0);
    stage_store(smem);
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < NS; ++s) {
        const bool more = s + 1 < NS;
        if (more) stage_load(s + 1);              // in flight under this stage's MFMAs
        const char *slab = smem + cur * SLAB;
        const int cg = s % ncg;
        const int kg = min(GK, nch - cg * GK);
#pragma unroll
        for (int k = 0; k < GK; ++k)
            if (k < kg) kstep(slab, k * 64);
        if (more) {
            stage_store(smem + (cur ^ 1) * SLAB);
            __syncthreads();
            cur ^= 1;
        }
    }

    // ---- epilogue: lane (g, li) holds rows 4 g + r of each 16-row block, channels nlane .. nlane + NT - 1
    const int nlane = nb * BN + wn * (NT * 16) + li * NT;
    float biasf[NT];
    long long biasw[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if constexpr (BF) { biasf[t] = p.bias_f[nlane + t]; biasw[t] = 0; }
        else { biasw[t] = p.bias_w[nlane + t]; biasf[t] = 0.f; }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int mm = m0 + (wm * MT + m) * 16 + 4 * g + r;
            if (mm < p.M) {
                if constexpr (BF) {
                    const int ox = mm % p.Wo, t0 = mm / p.Wo;
                    const int oy = t0 % p.Ho, b = t0 / p.Ho;
                    const size_t opix = ((size_t)b * (p.Ho + 2) + oy + 1) * (p.Wo + 2) + ox + 1;
                    float y[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const float x = acc[m][t][r] + biasf[t];
                        y[t] = x >= 0.f ? x : x * p.slope;
                    }
                    if (p.res) {                  // the residual is a bf16 activation: exact in fp32
                        const unsigned short *rr = (const unsigned short *)(p.res + opix * p.out_pb) + nlane;
#pragma unroll
                        for (int t = 0; t < NT; ++t) y[t] += __uint_as_float((unsigned int)rr[t] << 16);
                    }
                    char *dst = p.out + opix * p.out_pb;
                    if (p.out_f32) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) ((float *)dst)[nlane + t] = y[t];
                    } else {
                        store_bf16<NT>(dst + (size_t)nlane * 2, y);
                    }
                } else {
                    long long *dst = p.raw + (size_t)mm * p.cout_pad + nlane;
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const long long tt = (long long)acc[m][t][r] * (1ll << p.shl) + biasw[t];
                        dst[t] = tt >= 0 ? tt * (1ll << p.lk) : tt * (long long)p.neg_mul;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int WM, int WN, int MT, int NT>
struct GeomInst {
    static constexpr size_t LDS = 2 * (size_t)(WM * MT * 16) * GROW;
    static void launch(int bf, const ConvGeomParams &p, int nblocks, hipStream_t s) {
        if (bf) hipLaunchKernelGGL((convgeom_kernel<true, WM, WN, MT, NT>), dim3(nblocks), dim3(256), LDS, s, p);
        else hipLaunchKernelGGL((convgeom_kernel<false, WM, WN, MT, NT>), dim3(nblocks), dim3(256), LDS, s, p);
    }
    static int prepare() {
        if (int e = (int)hipFuncSetAttribute((const void *)convgeom_kernel<true, WM, WN, MT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)LDS)) return e;
        return (int)hipFuncSetAttribute((const void *)convgeom_kernel<false, WM, WN, MT, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)LDS);
    }
    static constexpr ConvGeomInfo info() { return ConvGeomInfo{WM * MT * 16, WN * NT * 16, WM, WN, MT, NT, LDS}; }
};

struct GeomEntry {
    ConvGeomInfo info;
    void (*launch)(int bf, const ConvGeomParams &p, int nblocks, hipStream_t s);
    int (*prepare)(void);
};
#define GEOM_ENTRY(WM, WN, MT, NT) GeomEntry{GeomInst<WM, WN, MT, NT>::info(), &GeomInst<WM, WN, MT, NT>::launch, &GeomInst<WM, WN, MT, NT>::prepare}
const GeomEntry g_geom[Y355_GEOM_COUNT] = {
    GEOM_ENTRY(2, 2, 4, 4),    // 0: 128 pixels x 128 channels (wide layers that fill the chip)
    GEOM_ENTRY(4, 1, 2, 2),    // 1: 128 pixels x 32 channels (few output channels)
    GEOM_ENTRY(2, 2, 2, 2),    // 2: 64 pixels x 64 channels (everything else: more workgroups per layer)
};
}  // namespace

const ConvGeomInfo *y355_convgeom_info(int id) { return (id >= 0 && id < Y355_GEOM_COUNT) ? &g_geom[id].info : nullptr; }

int y355_prepare_convgeom(void) {
    for (const GeomEntry &e : g_geom)
        if (int rc = e.prepare()) return rc;
    return 0;
}

// tile shape for M output pixels x cout channels on `cu` compute units: the 128 x 128 tile when it alone gives every CU a
// workgroup, 32-channel columns when that is all there is, 64 x 64 otherwise
int y355_convgeom_select(int M, int cout, int cu) {
    const int c16 = (cout + 15) / 16 * 16;
    if (c16 <= 32) return 1;
    const long tiles = (long)((M + 127) / 128) * ((cout + 127) / 128);
    if (c16 > 64 && tiles >= cu) return 0;
    return 2;
}

size_t y355_convgeom_packed_bytes(int id, int in_pb, int taps, int cout_pad) {
    const ConvGeomInfo &ki = g_geom[id].info;
    return (size_t)(cout_pad / ki.bn) * taps * (in_pb / 64) * ki.wn * ki.nt * 1024;
}

// B fragments (y355_pack_bfrags) with the k-steps tap-major: ks = tap * nchunk + chunk covers input bytes [64 chunk, + 64) at
// tap = ky * kw + kx.  w is [cout][cin][kh][kw], fp32 or int8.
void y355_convgeom_pack(int id, int bf, const float *w_f, const int8_t *w_q, int cout, int cin, int taps, int in_pb, int cout_pad,
                        char *dst) {
    const ConvGeomInfo &ki = g_geom[id].info;
    const int nch = in_pb / 64, kel = bf ? 32 : 64;
    y355_pack_bfrags(bf != 0, taps * nch, ki.bn, ki.wn, ki.nt, w_f, w_q, cout, cin, taps, cout_pad, dst, [=](int ks, int k, int &tap, int &ci) {
        tap = ks / nch;
        ci = (ks % nch) * kel + k;
    });
}

void y355_launch_convgeom(int id, int bf, const ConvGeomParams &p, hipStream_t s) {
    const int nblocks = (p.M + g_geom[id].info.bm - 1) / g_geom[id].info.bm * p.nblk;
    g_geom[id].launch(bf, p, nblocks, s);
}
