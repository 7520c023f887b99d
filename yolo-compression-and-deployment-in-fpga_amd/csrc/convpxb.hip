// yolo355 -- the thin 3x3 layers of the bf16 nets with the WEIGHTS IN REGISTERS (round 6): the bf16
// form of convpx.hip for SlimYOLOv2's conv3_1 (32 -> 64), conv3_2 + pool3 (64 -> 64) and conv4_1 (64 -> 128)
// (models/slim_yolo_v2.py:403-412, forward :561-575, BatchNorm folded on the host).
//
// convr.hip runs these layers on the deep layers' ring discipline (weights streamed through an LDS ring, a barrier per k-step):
// 52 / 55 / 39 us at B = 64 for 10 / 20 / 10 us of MFMA work -- their K is 9 x 32 .. 9 x 64 channels, too shallow for a k-loop to
// amortise a tile's start-up.  convpx.hip's construction carries over unchanged because v_mfma_f32_16x16x32_bf16 takes the same 16
// operand bytes per lane as the int8 MFMA: a bf16 pixel of C channels is an "int8 pixel" of 2 C bytes for the LDS-DMA row ring, the
// swizzles and every address; only the k-step holds 32 channels instead of 64.  So, as there:
//   * the weights are the MFMA's A operand (rows = output channels); a wave keeps ALL fragments of its block of 16 NTN output
//     channels in registers for the whole launch (36 fragments = 144 VGPRs in all three instantiations);
//   * the pixels are the B operand (16 consecutive pixels, or 16 consecutive 2x2 pooling windows whose 4x4 neighbourhood is read
//     once and fed to the window's four conv outputs), read from a rolling ring of whole padded input rows in LDS that LDS-DMA fills
//     one chunk ahead, behind a counted vmcnt;
//   * a lane ends up with 4 NTN consecutive channels of ONE pixel: 16- or 32-byte stores straight from the registers.
// What differs is the epilogue, which is the bf16 nets' (convg.hip / convr.hip): fp32 accumulator (the bias rides in as the MFMAs' C
// operand) -> [2x2 max] -> LeakyReLU(slope) -> bf16 (RNE) -- no saturation, no cold pass, no counters.
// Parity: tolerance against the fp32 oracle (tests/test_fp32_models.py); the accumulation order differs from convr's in where the bias
// enters, so the two routes are not bit-identical and are compared within 2 bf16 ulps (tests/test_fp32_models.py::test_convpxb_...).
#include "y355_rowring.h"
#include <cstring>
#include <type_traits>
#ifndef PXB_R31
#define PXB_R31 11               // groups per wave and chunk of the unpooled layers
#define PXB_R41 6
#endif

namespace {
using namespace y355dev;
// PXB = bytes per input pixel (2 x channels): 64 or 128
template <int PXB, int NTN, int NCB, bool POOL>
struct PbGeom {
    static constexpr int KPP = PXB / 64;                         // k-steps (32 channels) per tap
    static constexpr int KS = 9 * KPP;
    static constexpr int CPB = 16 * NTN;                         // output channels per block (per wave)
    static constexpr int COUT = CPB * NCB;
    static constexpr int NFRAG = NCB * KS * NTN;
    static_assert(PXB == 64 || PXB == 128, "input channels 32 or 64");
};
}  // namespace

template <int PXB, int NTN, int NCB, bool POOL, int NW>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void convpxb_kernel(const ConvGParams p, const RowRingArgs a) {
    using G = PbGeom<PXB, NTN, NCB, POOL>;
    constexpr int KPP = G::KPP, KS = G::KS, CPB = G::CPB;
    constexpr int NPS = NW / NCB;                        // pixel streams: waves that share a channel block
    constexpr int NV = POOL ? 4 : 1;                     // conv outputs per column (pooling window)
    constexpr int SPG = NTN / 2;                         // 16-byte stores per lane and group
    static_assert(NW % NCB == 0 && (NTN == 4 || NTN == 2), "geometry");
    extern __shared__ __attribute__((aligned(16))) char smem[];       // ring of 2^logr rows of PWL * PXB bytes
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = wave % NCB, ps = wave / NCB;
    const int g = lane >> 4;

    // ---- weights of this wave's channel block: A fragments [k-step][n-tile], registers for the whole launch
    v4i wf[KS][NTN];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int n = 0; n < NTN; ++n) wf[ks][n] = *(const v4i *)(p.w + ((size_t)(cb * KS + ks) * NTN + n) * 1024 + lane * 16);
    // accumulator register r of n-tile n of lane group g = channel cb * CPB + 4 NTN g + 4 n + r; the bias is the MFMAs' C operand
    v4f cin[NTN];
#pragma unroll
    for (int n = 0; n < NTN; ++n) cin[n] = *(const v4f *)(p.bias_f + cb * CPB + 4 * NTN * g + 4 * n);
    float slope = p.slope;
    asm volatile("" : "+v"(slope));                      // a VGPR operand for the epilogue's multiply (y355_fp32epi.h has the measurement)

    // ---- this workgroup's share of the batch's groups, walked in chunks of <= cg groups on the ring of padded input rows
    // (y355_rowring.h, shared with convpx.hip: the ring's invariants, the counted wait and the swizzles)
    using Ring = RowRing<PXB, NW, POOL>;
    int gbeg, gend;
    if (!Ring::share(a, gbeg, gend)) return;
    const Ring ring(a, p.in, smem, p.H, p.W, lane, wave, gend);
    constexpr int MUL = Ring::MUL;
    const int H = ring.H, Ho = ring.Ho, Wo = ring.Wo, rowb = ring.rowb, RM = ring.RM;

    RowChunk ch = ring.chunk_at(gbeg);
    ring.issue_rows(ch.lo, ch.hi);
    int loaded = ch.hi;
    int gg = gbeg, nstores = -1;                         // stores this wave issued behind its last DMA piece (-1: wait for everything)
    for (;;) {
        wait_vmcnt_upto<24>(nstores);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        ring.late_rows(ch, loaded);
        const int gnext = gg + (ch.g1 - ch.g0);
        const bool more = gnext < gend;
        RowChunk nx = ch;
        if (more) nx = ring.chunk_at(gnext);
        int pf_r0, pf_nr;
        ring.next_window(ch, nx, more, loaded, pf_r0, pf_nr);
        int pfc = ring.rr0;
        auto prefetch = [&](int count) {
            if (ring.issue_pieces(pf_r0, pf_nr, pfc, count) > 0) nstores = 0;
        };
        char *outb = p.out + (((size_t)ch.b * (Ho + 2) + 1) * (Wo + 2) + 1) * (size_t)p.out_pb + p.out_off + cb * CPB * 2;    // wave-uniform
        const int rbase = ch.b * (H + 2);

        auto mfma = [&](const v4i &wa, const v4i &b, const v4f &c) {
            return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8bf, wa), __builtin_bit_cast(v8bf, b), c, 0, 0, 0);
        };
        auto issue = [&](int grp, v4f (&acc)[NV][NTN]) {
            int oy, ox;
            ring.locate(grp, oy, ox);
            const int ar = rbase + MUL * oy, x0 = MUL * ox;
            constexpr int NC = POOL ? 4 : 3;
            int xoff[NC], roff[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                xoff[c] = Ring::read_off(x0 + c, g);
                roff[c] = ((ar + c) & RM) * rowb;
            }
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int n = 0; n < NTN; ++n) acc[v][n] = cin[n];
            if constexpr (!POOL) {
                if constexpr (KPP == 1) {                          // every read of the group, then its MFMAs (one exposed LDS wait per group)
                    v4i bq[9];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) bq[tap] = *(const v4i *)(smem + roff[tap / 3] + xoff[tap % 3]);
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                        for (int n = 0; n < NTN; ++n) acc[0][n] = mfma(wf[tap][n], bq[tap], acc[0][n]);
                    __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 9 * NTN, 0);
                } else {                                           // a filter row's reads, then its MFMAs (18 operands do not fit beside 144 VGPRs of weights)
#pragma unroll
                    for (int ty = 0; ty < 3; ++ty) {
                        v4i bq[3][KPP];
#pragma unroll
                        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                            for (int h = 0; h < KPP; ++h) bq[tx][h] = *(const v4i *)(smem + roff[ty] + (xoff[tx] ^ (h << 6)));
#pragma unroll
                        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                            for (int h = 0; h < KPP; ++h)
#pragma unroll
                                for (int n = 0; n < NTN; ++n) acc[0][n] = mfma(wf[(ty * 3 + tx) * KPP + h][n], bq[tx][h], acc[0][n]);
                    }
                }
            } else {
                // neighbourhood row r feeds conv output (dy, dx) with filter tap (r - dy, c - dx)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v4i bq[4][KPP];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int h = 0; h < KPP; ++h) bq[c][h] = *(const v4i *)(smem + roff[r] + (xoff[c] ^ (h << 6)));
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
                        const int ty = r - dy;
                        if (ty < 0 || ty > 2) continue;
#pragma unroll
                        for (int c = 0; c < 4; ++c)
#pragma unroll
                            for (int dx = 0; dx < 2; ++dx) {
                                const int tx = c - dx;
                                if (tx < 0 || tx > 2) continue;
#pragma unroll
                                for (int h = 0; h < KPP; ++h)
#pragma unroll
                                    for (int n = 0; n < NTN; ++n)
                                        acc[2 * dy + dx][n] = mfma(wf[(ty * 3 + tx) * KPP + h][n], bq[c][h], acc[2 * dy + dx][n]);
                            }
                    }
                }
            }
        };
        auto finish = [&](int grp, const v4f (&acc)[NV][NTN]) {
            int oy, ox;
            ring.locate(grp, oy, ox);
            unsigned int word[NTN][2];
#pragma unroll
            for (int n = 0; n < NTN; ++n) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = acc[0][n][r];
                    if constexpr (POOL) t = fmaxf(fmaxf(t, acc[1][n][r]), fmaxf(acc[2][n][r], acc[3][n][r]));   // the max commutes with the monotone LeakyReLU
                    y[r] = fmaxf(t, t * slope);                    // LeakyReLU for 0 <= slope <= 1 (launcher); slope 1: identity
                }
                word[n][0] = pk_bf16(y[0], y[1]);
                word[n][1] = pk_bf16(y[2], y[3]);
            }
            // unconditional: the padding lanes rewrite the image's last pixel with the same bytes, and the number of stores a
            // wave has in flight stays a function of its group count (the counted wait above)
            char *dst = outb + (size_t)(oy * (Wo + 2) + ox) * (size_t)p.out_pb + 8 * NTN * g;
            *(v4i *)dst = (v4i){(int)word[0][0], (int)word[0][1], (int)word[1][0], (int)word[1][1]};
            if constexpr (NTN == 4) *(v4i *)(dst + 16) = (v4i){(int)word[2][0], (int)word[2][1], (int)word[3][0], (int)word[3][1]};
        };
        nstores = 0;
        {
            v4f acc[NV][NTN];
#pragma unroll 1
            for (int grp = ch.g0 + ps; grp < ch.g1; grp += NPS) {
                issue(grp, acc);
                prefetch(a.ppg);
                finish(grp, acc);
                nstores += SPG;
            }
            prefetch(1 << 30);
        }
        if (!more) break;
        gg = gnext;
        ch = nx;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------
namespace {
// A fragments: fragment ((cb * KS + ks) * NTN + n), lane (i = l & 15, g = l >> 4), 8 bf16:
//   row i = output channel cb * CPB + 4 NTN (i >> 2) + 4 n + (i & 3);  k = tap ks / KPP, input channels 32 (ks % KPP) + 8 g .. + 7
template <int PXB, int NTN, int NCB, bool POOL>
void pb_pack(const float *w, int cout, int cin, char *dst) {
    using G = PbGeom<PXB, NTN, NCB, POOL>;
    memset(dst, 0, (size_t)G::NFRAG * 1024);
    unsigned short *d = (unsigned short *)dst;
    for (int cb = 0; cb < NCB; ++cb)
        for (int ks = 0; ks < G::KS; ++ks)
            for (int n = 0; n < NTN; ++n)
                for (int l = 0; l < 64; ++l) {
                    const int i = l & 15, g = l >> 4;
                    const int ch = cb * G::CPB + 4 * NTN * (i >> 2) + 4 * n + (i & 3);
                    const int tap = ks / G::KPP, c0 = 32 * (ks % G::KPP) + 8 * g;
                    if (ch >= cout) continue;
                    for (int kk = 0; kk < 8; ++kk)
                        if (c0 + kk < cin)
                            d[((((size_t)cb * G::KS + ks) * NTN + n) * 1024 + l * 16) / 2 + kk] = y355_bf16_rne(w[((size_t)ch * cin + c0 + kk) * 9 + tap]);
                }
}

template <int PXB, int NTN, int NCB, bool POOL, int NW>
struct PbInst {
    using G = PbGeom<PXB, NTN, NCB, POOL>;
    static constexpr int NPS = NW / NCB;
    static RowRingArgs args(const ConvGParams &p, int rounds) { return rowring_args<PXB, NW, NPS, POOL>(p.B, p.H, p.W, rounds); }
    static size_t lds_bytes(const RowRingArgs &a) { return rowring_lds_bytes<PXB>(a); }
    static bool launch(const ConvGParams &p, int rounds, hipStream_t s) {
        const int Wo = POOL ? p.W / 2 : p.W;
        if (p.in_pb != PXB || !p.out_halo || p.out_f32 || p.res || p.taps != 9 || !p.bias_f || p.W < 16 || Wo < 1) return false;
        if (POOL && ((p.H | p.W) & 1)) return false;
        if (!(p.slope >= 0.f && p.slope <= 1.f)) return false;                 // the epilogue takes max(t, slope * t)
        if (((p.out_pb | p.out_off) & 15) || p.out_pb < p.out_off + G::COUT * 2) return false;
        if ((long long)p.B * (p.H + 2) * (p.W + 2) * PXB >= (1ll << 31)) return false;      // 32-bit row arithmetic
        // the largest chunk (groups per pixel stream: `rounds` at most) whose ring of whole padded rows fits LDS -- a bf16 row is twice
        // an int8 row, so the shapes of this network take about half of convpx.hip's chunk; a map too wide for any chunk is declined
        RowRingArgs a = args(p, rounds);
        while (lds_bytes(a) > 160 * 1024 && rounds > 1) a = args(p, --rounds);
        if (lds_bytes(a) > 160 * 1024) return false;
        int grid = y355_cu_count();                                // one NW-wave workgroup per CU
        if (p.grid_limit > 0 && p.grid_limit < grid) grid = p.grid_limit;
        if (grid > a.total_groups) grid = a.total_groups;
        hipLaunchKernelGGL((convpxb_kernel<PXB, NTN, NCB, POOL, NW>), dim3(grid), dim3(NW * 64), lds_bytes(a), s, p, a);
        return true;
    }
    static int prepare() {
        return (int)hipFuncSetAttribute((const void *)convpxb_kernel<PXB, NTN, NCB, POOL, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
};
//                    PXB NTN NCB POOL  NW        SlimYOLOv2 on bf16
using PB_C3_1 = PbInst<64, 4, 1, false, 8>;       // 32 -> 64:           eight pixel streams
using PB_C3_2 = PbInst<128, 2, 2, true, 8>;       // 64 -> 64, pooled:   two 32-channel blocks x four window streams
using PB_C4_1 = PbInst<128, 2, 4, false, 8>;      // 64 -> 128:          four 32-channel blocks x two pixel streams
}  // namespace

int y355_prepare_convpxb(void) {
    int e = PB_C3_1::prepare();
    if (!e) e = PB_C3_2::prepare();
    if (!e) e = PB_C4_1::prepare();
    return e;
}

// id of the instantiation for a 3x3 / stride 1 layer with in_pb bytes per input pixel, cout output channels and a fused 2x2 pool
// (or none): -1 = none.  Packed weights: y355_convpxb_packed_bytes / y355_convpxb_pack (w fp32 [cout][cin][3][3]).
int y355_convpxb_select(int in_pb, int cout, int pool) {
    if (in_pb == 64 && cout == 64 && !pool) return 0;
    if (in_pb == 128 && cout == 64 && pool) return 1;
    if (in_pb == 128 && cout == 128 && !pool) return 2;
    return -1;
}
size_t y355_convpxb_packed_bytes(int id) {
    switch (id) {
    case 0: return (size_t)PB_C3_1::G::NFRAG * 1024;
    case 1: return (size_t)PB_C3_2::G::NFRAG * 1024;
    case 2: return (size_t)PB_C4_1::G::NFRAG * 1024;
    default: return 0;
    }
}
bool y355_convpxb_pack(int id, const float *w, int cout, int cin, char *dst) {
    switch (id) {
    case 0: if (cin > 32 || cout != 64) return false; pb_pack<64, 4, 1, false>(w, cout, cin, dst); return true;
    case 1: if (cin > 64 || cout != 64) return false; pb_pack<128, 2, 2, true>(w, cout, cin, dst); return true;
    case 2: if (cin > 64 || cout != 128) return false; pb_pack<128, 2, 4, false>(w, cout, cin, dst); return true;
    default: return false;
    }
}
// false = not available for this launch: the caller runs convr.hip / convg.hip.  p.w = y355_convpxb_pack layout.
bool y355_launch_convpxb(int id, const ConvGParams &p, hipStream_t s) {
    switch (id) {
    case 0: return PB_C3_1::launch(p, PXB_R31, s);
    case 1: return PB_C3_2::launch(p, 2, s);
    case 2: return PB_C4_1::launch(p, PXB_R41, s);
    default: return false;
    }
}
