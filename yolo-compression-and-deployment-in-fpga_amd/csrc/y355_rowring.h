// yolo355 -- the rolling ring of whole padded input rows in LDS that the weights-in-registers kernels walk: convpx.hip (int8)
// and convpxb.hip (bf16, whose pixel of C channels is an "int8 pixel" of 2 C bytes for everything here).  The host geometry
// (rowring_args) and the device side (RowRing) in one place; the kernels keep their MFMA bodies, epilogues and chunk loops.
//
// Work: groups of 16 pixels (or 16 2x2 pooling windows) in row-major order over the batch.  Workgroup i owns the contiguous
// share [gbeg, gend) and walks it in CHUNKS of at most cg groups that stay inside one image; pixel stream ps of NPS takes the
// groups g0 + ps, g0 + ps + NPS, ... of a chunk.  A chunk reads the absolute padded input rows [lo, hi) (row = b * (H + 2) +
// padded row of image b).
//
// The ring.  Row r lives in slot r & (R - 1), R = 2^logr rows of pwl * PXB bytes; every row is copied once per workgroup by
// LDS-DMA in 1 KiB pieces of PPP pixels that each stay inside one row (the pitch pwl is a multiple of PPP).
//   * Live rows: those of the chunk being computed, [ch.lo, ch.hi), and, in flight or landed, the next chunk's rows below
//     ch.lo + R (next_window).  Rows below ch.lo are dead: every wave passed the barrier at the head of the chunk only when it
//     was done with the previous one.  A new row r < ch.lo + R takes the slot of row r - R < ch.lo, a dead one, and it is issued
//     behind that barrier: the write-after-read rule of LDS-DMA holds without a second barrier.
//   * R >= MUL * rows2 + 2, where rows2 bounds the output rows two consecutive chunks of an image touch (MUL = 2 when pooled;
//     + 2: the 3x3 halo): inside an image the whole next chunk fits beside the current one.  Across an image boundary the row
//     numbers jump and the tail may not fit: late_rows issues it behind the chunk's barrier and pays a full wait and a second
//     barrier.
//   * The counted wait.  vmcnt retires in order.  A wave issues the next chunk's pieces a few at a time behind its groups,
//     between its output stores; `nstores` counts the stores it issued after its LAST piece (any piece resets it to 0), so
//     s_waitcnt vmcnt(nstores) at the head of the next chunk covers every piece of the wave and leaves exactly those stores in
//     flight.  The stores are unconditional (padding lanes rewrite the image's last pixel) so that the count is a function
//     of the group count; -1 (the first chunk, or after a cold pass) waits for everything.  A wave waits for its own pieces
//     only; the barrier behind the wait publishes everybody's.  nstores <= rounds * (stores per group): the kernels' tables
//     (wait_vmcnt_upto<16> / <24>) cover it, and a count beyond them only waits longer.
//   * Source-side swizzle.  LDS-DMA writes lane l's 16 bytes at piece + 16 l: chunk l % CPX of pixel l / CPX (CPX = PXB / 16
//     chunks per pixel).  The lane READS source chunk (l % CPX) ^ f(x) of pixel x instead, f(x) = 2 ((x >> 2) & 1) for 64-byte
//     and 2 ((x >> 1) & 3) for 128-byte pixels: LDS chunk c of pixel x holds source chunk c ^ f(x), and a reader that applies
//     the same f to its chunk index gets every ds_read_b128 conflict-free under gfx950's 4 x 16 lane grouping.  32-byte pixels
//     are not swizzled.  Columns past the padded row's end (the pitch's slack) re-read its last pixel.
//   * Who sends what: a wave owns ONE piece column pc0 (its lanes' pixel, swizzled chunk and byte offset inside a row are
//     launch constants) and every RS-th row of it -- ppr <= NW: NW / ppr rows per round of the waves (the waves beyond RS * ppr
//     send nothing); wider rows: every row, the columns pc0, pc0 + NW, ...  A piece then costs one scalar multiply-add for the
//     row's offsets and the DMA (before: a (row, column) cursor with a wrap loop, ~17 scalar and 6 vector instructions per
//     piece, 900 - 1 600 scalar instructions per wave and launch: profiles/r04_notes.md 13).
#pragma once
#include "y355_dev.h"

namespace y355dev {
struct RowRingArgs {
    int total_groups;     // groups of 16 pixels / windows in the batch (ngi per image)
    int ngi;              // groups per image
    int cg;               // groups per chunk (a multiple of the pixel streams of a workgroup)
    int pwl;              // LDS row pitch in pixels (a multiple of PPP, >= W + 2)
    int logr;             // ring of 2^logr rows
    int ppg;              // DMA pieces a wave issues behind each of its groups
};
// image, groups [g0, g1) of it, absolute padded input rows [lo, hi) it reads
struct RowChunk { int b, g0, g1, lo, hi; };

// PXB bytes per input pixel, NW waves, NPS pixel streams; rounds: groups per pixel stream per chunk
template <int PXB, int NW, int NPS, bool POOL>
inline RowRingArgs rowring_args(int B, int H, int W, int rounds) {
    constexpr int PPP = 1024 / PXB;
    RowRingArgs a;
    const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
    a.ngi = (Ho * Wo + 15) / 16;
    a.total_groups = a.ngi * B;
    a.cg = rounds * NPS;
    a.pwl = (W + 2 + PPP - 1) / PPP * PPP;
    // two consecutive chunks of an image are in the ring together: MUL * (output rows they touch) + 2 rows
    const int rows2 = (2 * 16 * a.cg + Wo - 1) / Wo + 1;
    const int need = (POOL ? 2 : 1) * rows2 + 2;
    a.logr = 2;
    while ((1 << a.logr) < need) ++a.logr;
    // a chunk adds about MUL * 16 cg / Wo rows = that many * pwl / PPP pieces, dealt over NW waves and `rounds` groups each
    const int newrows = (POOL ? 2 : 1) * ((16 * a.cg + Wo - 1) / Wo + 1);
    const int ppr = a.pwl / PPP, rs = ppr < NW ? NW / ppr : 1, cpw = ppr < NW ? 1 : (ppr + NW - 1) / NW;
    const int per_wave = (newrows + rs - 1) / rs * cpw;         // a wave sends one piece column of every rs-th row
    a.ppg = (per_wave + rounds - 1) / rounds;
    return a;
}
template <int PXB>
inline size_t rowring_lds_bytes(const RowRingArgs &a) { return ((size_t)a.pwl * PXB) << a.logr; }

template <int PXB, int NW, bool POOL>
struct RowRing {
    static constexpr int PPP = 1024 / PXB;               // pixels per 1 KiB DMA piece (= LDS pitch granule)
    static constexpr int CPX = PXB / 16;                 // 16-byte chunks per pixel
    static constexpr int MUL = POOL ? 2 : 1;
    const RowRingArgs a;
    const char *const in;                                // padded input map
    char *const smem;                                    // the ring: 2^logr rows of rowb bytes
    int H, PW, Ho, Wo, npw, rowb;                        // map geometry; npw pixels / windows per image; bytes per ring row
    float invWo;
    int gend;                                            // end of this workgroup's share of the batch's groups
    int R, RM;
    int li, dpx, dch, ppr, RS, CPW, pc0, rr0, goff0;     // piece dealing: see the header

    // this workgroup's contiguous, equal share [gbeg, gend) of the batch's groups; false: it has none
    __device__ __forceinline__ static bool share(const RowRingArgs &a, int &gbeg, int &gend) {
        const int G_ = gridDim.x;
        gbeg = (int)((long long)a.total_groups * blockIdx.x / G_), gend = (int)((long long)a.total_groups * (blockIdx.x + 1) / G_);
        return gbeg < gend;
    }
    __device__ __forceinline__ RowRing(const RowRingArgs &a_, const void *in_, char *smem_, int H_, int W, int lane, int wave, int gend_)
        : a(a_), in((const char *)in_), smem(smem_), gend(gend_) {
        H = H_;
        PW = W + 2;
        const int PWL = a.pwl;
        Ho = POOL ? H >> 1 : H, Wo = POOL ? W >> 1 : W;
        npw = Ho * Wo;
        rowb = PWL * PXB;
        invWo = 1.0f / (float)Wo;
        R = 1 << a.logr, RM = R - 1;
        li = lane & 15;
        dpx = lane / CPX, dch = lane % CPX;
        ppr = PWL / PPP;                                 // pieces per row
        RS = ppr < NW ? NW / ppr : 1;
        CPW = ppr < NW ? 1 : (ppr + NW - 1) / NW;
        pc0 = ppr < NW ? wave % ppr : wave;
        rr0 = ppr < NW ? (wave / ppr < RS ? wave / ppr : (1 << 28)) : 0;
        goff0 = lane_off(pc0);
    }
    // the chunk that starts at group gg of the batch: <= cg groups inside one image and inside the share
    __device__ __forceinline__ RowChunk chunk_at(int gg) const {
        RowChunk c;
        c.b = gg / a.ngi;
        c.g0 = gg - c.b * a.ngi;
        c.g1 = min(min(c.g0 + a.cg, a.ngi), c.g0 + (gend - gg));
        const int ya = (16 * c.g0) / Wo, yb = (min(16 * c.g1, npw) - 1) / Wo;
        c.lo = c.b * (H + 2) + MUL * ya;
        c.hi = c.b * (H + 2) + MUL * yb + (POOL ? 4 : 3);
        return c;
    }
    // byte offset of this lane's 16 bytes inside a padded input row, piece column pc
    __device__ __forceinline__ int lane_off(int pc) const {
        const int col = pc * PPP + dpx;
        int sch = dch;
        if constexpr (CPX == 4) sch ^= ((col >> 2) & 1) << 1;
        if constexpr (CPX == 8) sch ^= ((col >> 1) & 3) << 1;
        return min(col, PW - 1) * PXB + 16 * sch;
    }
    // the reader's side of the swizzle: byte offset of chunk `sch` of padded column x inside a ring row
    __device__ __forceinline__ static int read_off(int x, int sch) {
        if constexpr (CPX == 4) sch ^= ((x >> 2) & 1) << 1;
        if constexpr (CPX == 8) sch ^= ((x >> 1) & 3) << 1;
        return x * PXB + 16 * sch;
    }
    // this wave's pieces of rows r0 + rr, rr = cursor, cursor + RS, ... < nrows: at most about `count` pieces; the cursor
    // travels with the caller
    __device__ __forceinline__ int issue_pieces(int r0, int nrows, int &rr, int count) const {
        int done = 0;
        for (; rr < nrows && done < count; rr += RS) {
            const int row = r0 + rr;
            const char *src = in + (size_t)row * (size_t)(PW * PXB);
            char *dst = smem + (row & RM) * rowb;
            glds16(src + goff0, dst + pc0 * 1024);
            ++done;
            for (int j = 1; j < CPW; ++j) {              // rows wider than NW pieces (not the shapes of this network)
                const int pc = pc0 + j * NW;
                if (pc < ppr) {
                    glds16(src + lane_off(pc), dst + pc * 1024);
                    ++done;
                }
            }
        }
        return done;
    }
    __device__ __forceinline__ void issue_rows(int r0, int r1) const {
        int rr = rr0;
        issue_pieces(r0, r1 - r0, rr, 1 << 30);
    }
    // rows of `ch` that could not be issued ahead (the ring was full: image boundaries); call behind the chunk's barrier
    __device__ __forceinline__ void late_rows(const RowChunk &ch, int &loaded) const {
        if (loaded < ch.hi) {
            issue_rows(max(loaded, ch.lo), ch.hi);
            loaded = ch.hi;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
    // the next chunk's new rows, as far as they fit beside the rows `ch` still reads: [r0, r0 + nr), from now on `loaded`
    __device__ __forceinline__ void next_window(const RowChunk &ch, const RowChunk &nx, bool more, int &loaded, int &r0, int &nr) const {
        r0 = 0, nr = 0;
        if (more) {
            const int top = min(nx.hi, ch.lo + R);
            r0 = max(loaded, nx.lo);
            if (top > r0) {
                nr = top - r0;
                loaded = top;
            }
        }
    }
    // group grp of an image -> this lane's pixel / window (oy, ox); padding lanes of an image's last group repeat its last one
    __device__ __forceinline__ void locate(int grp, int &oy, int &ox) const {
        const int pc = min(grp * 16 + li, npw - 1);
        oy = (int)(((float)pc + 0.5f) * invWo);          // pc / Wo (exact: pc < 2^16)
        ox = pc - oy * Wo;
    }
};
}  // namespace y355dev
