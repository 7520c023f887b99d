// yolo355_bntrain -- one training step of the BatchNorm SlimYOLOv2 on the GPU (gfx950): the convolutions of train_core.h (the
// kernels libyolo355_train.so compiles too) around BatchNorm2d in training mode; C ABI in include/yolo355_bntrain.h, linked
// into libyolo355_bntrain.so on its own.  The arithmetic contract is DESIGN.md section 6n.
//
// Per layer k = 1..9 the forward runs train_conv_kernel<M_Z> (Z_k = rb(conv + b), bf16 NHWC on the pre-pool grid), then
//   bn_stats_kernel<false>     per channel sum Z and sum Z^2 in float64 over a run of pixels: one workgroup a run, a lane owns
//                              eight channels (one 16-byte load a pixel), the workgroup's pixel rows are added through LDS in
//                              their order; one partial per run and channel to a workspace
//   bn_finalise_kernel<false>  adds the runs in their order; mean, var, invstd; moves running_mean and running_var
//   bn_norm_kernel             xhat, gamma, beta, LeakyReLU, the 2x2 pool with I_k (a lane holds the four window positions of
//                              its eight channels), rb -> A_k
// and the backward, after section 6m's data gradient has left dY_k,
//   bn_stats_kernel<true>      sum dY and sum dY xhat, the same runs
//   bn_finalise_kernel<true>   dbeta, dgamma and the per-channel factors m1, m2, gamma * invstd of the apply
//   bn_apply_kernel            G_k = rb((dY - m1 - xhat m2) (gamma invstd))
// before the unchanged weight-gradient and reduce kernels.  bn_sgd_kernel is train_sgd_kernel's update on gamma and beta.
// No atomics anywhere: the same bits from run to run.
#include "../../include/yolo355_bntrain.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_BNTRAIN_OK == Y355_OK && Y355_BNTRAIN_EINVAL == Y355_EINVAL && Y355_BNTRAIN_EHIP == Y355_EHIP &&
                  Y355_BNTRAIN_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_bntrain_last_error's text
#ifndef Y355_HOSTCHECK                                   // (bntrain_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

#include "train_core.h"
static_assert(NL == Y355_BNTRAIN_LAYERS, "train_core.h's layer table");
constexpr int NBN = Y355_BNTRAIN_BN_LAYERS;
constexpr int STAT_MAX_RUNS = 1024, STAT_ALIGN = 128;    // a workgroup of 256 lanes takes 8 (256 channels) to 128 (16) pixels a step

// ---------------------------------------------------------------------------------------------------------- kernels
__device__ __forceinline__ void unpack8_(const uint4 u, float (&v)[8]) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = __builtin_bit_cast(float, w[e] << 16);
        v[2 * e + 1] = __builtin_bit_cast(float, w[e] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 rb8_(const float (&v)[8]) {
    uint4 u;
    u.x = (unsigned)rb_(v[0]) | ((unsigned)rb_(v[1]) << 16);
    u.y = (unsigned)rb_(v[2]) | ((unsigned)rb_(v[3]) << 16);
    u.z = (unsigned)rb_(v[4]) | ((unsigned)rb_(v[5]) << 16);
    u.w = (unsigned)rb_(v[6]) | ((unsigned)rb_(v[7]) << 16);
    return u;
}

struct StatArgs {
    const bf16_t *z;                 // Z_k, NHWC, C channels
    const bf16_t *dy;                // BWD: dY_k
    const float *mean, *invstd;      // BWD: of the layer
    double *ws;                      // [run][2][C]
    size_t N, chunk;                 // chunk: pixels of a run, a multiple of STAT_ALIGN
    int C, cg_log2;                  // C / 8 lanes across the channels
};

// FWD: s = sum Z, q = sum Z^2.  BWD: s = sum dY, q = sum dY xhat, xhat = (Z - mean) * invstd in fp32.  Terms and products are
// exact in float64; a lane adds its pixels in their order, then the workgroup's rows in theirs.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_stats_kernel(const StatArgs a) {
    __shared__ double sh[2][256][8];
    const int t = threadIdx.x, ng = 1 << a.cg_log2, cg = t & (ng - 1), row = t >> a.cg_log2, rows = 256 >> a.cg_log2;
    const size_t start = (size_t)blockIdx.x * a.chunk, end = start + a.chunk < a.N ? start + a.chunk : a.N;
    double s[8], q[8];
    float mu[8], is[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s[e] = 0.0;
        q[e] = 0.0;
        mu[e] = BWD ? a.mean[cg * 8 + e] : 0.f;
        is[e] = BWD ? a.invstd[cg * 8 + e] : 0.f;
    }
    for (size_t p = start + row; p < end; p += rows) {
        float z[8];
        unpack8_(*(const uint4 *)(a.z + p * a.C + cg * 8), z);
        if constexpr (BWD) {
            float d[8];
            unpack8_(*(const uint4 *)(a.dy + p * a.C + cg * 8), d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xhat = (z[e] - mu[e]) * is[e];
                s[e] += (double)d[e];
                q[e] += (double)d[e] * (double)xhat;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                s[e] += (double)z[e];
                q[e] += (double)z[e] * (double)z[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sh[0][t][e] = s[e];
        sh[1][t][e] = q[e];
    }
    __syncthreads();
    if (t < a.C) {
        const int g = t >> 3, e = t & 7;
        double ss = 0.0, qq = 0.0;
        for (int r = 0; r < rows; ++r) {
            ss += sh[0][r * ng + g][e];
            qq += sh[1][r * ng + g][e];
        }
        double *ws = a.ws + (size_t)blockIdx.x * 2 * a.C;
        ws[t] = ss;
        ws[a.C + t] = qq;
    }
}

struct FinArgs {
    const double *ws;
    int runs, C;
    double N;
    float Nf;
    float *mean, *var, *invstd, *rmean, *rvar;       // FWD: written (rmean, rvar: moved)
    const float *gamma;                              // BWD
    float *dgamma, *dbeta, *m1, *m2, *gs;            // BWD: written
};

template <bool BWD>
__global__ __launch_bounds__(256) void bn_finalise_kernel(const FinArgs a) {
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double s = 0.0, q = 0.0;
    const size_t stride = 2 * (size_t)a.C;
    int r = 0;
    for (; r + 8 <= a.runs; r += 8) {                        // eight runs' loads in flight, added in the order of the runs all the same
        double vs[8], vq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            vs[u] = a.ws[(size_t)(r + u) * stride + c];
            vq[u] = a.ws[(size_t)(r + u) * stride + a.C + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s += vs[u];
            q += vq[u];
        }
    }
    for (; r < a.runs; ++r) {
        s += a.ws[r * stride + c];
        q += a.ws[r * stride + a.C + c];
    }
    if constexpr (BWD) {
        const float dbeta = (float)s, dgamma = (float)q;
        a.dbeta[c] = dbeta;
        a.dgamma[c] = dgamma;
        a.m1[c] = dbeta / a.Nf;
        a.m2[c] = dgamma / a.Nf;
        a.gs[c] = a.gamma[c] * a.invstd[c];
    } else {
        const double mean = s / a.N;
        double var = q / a.N - mean * mean;
        var = var > 0.0 ? var : 0.0;
        a.mean[c] = (float)mean;
        a.var[c] = (float)var;
        a.invstd[c] = (float)(1.0 / sqrt(var + Y355_BNTRAIN_EPS));
        a.rmean[c] = (float)((1.0 - Y355_BNTRAIN_MOMENTUM) * (double)a.rmean[c] + Y355_BNTRAIN_MOMENTUM * mean);
        a.rvar[c] = (float)((1.0 - Y355_BNTRAIN_MOMENTUM) * (double)a.rvar[c] + Y355_BNTRAIN_MOMENTUM * var * a.N / (a.N - 1.0));
    }
}

struct NormArgs {
    const bf16_t *z;
    const float *mean, *invstd, *gamma, *beta;
    bf16_t *out;                     // A_k
    unsigned char *idx;              // POOL: I_k
    size_t nout;                     // pixels of the output grid
    int H, W, C, cg_log2;            // H, W: of Z's grid
};

template <bool POOL>
__global__ __launch_bounds__(256) void bn_norm_kernel(const NormArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t o = i >> a.cg_log2;
    if (o >= a.nout) return;
    const int c0 = (int)(i & (((size_t)1 << a.cg_log2) - 1)) * 8;
    float mu[8], is[8], ga[8], be[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        mu[e] = a.mean[c0 + e];
        is[e] = a.invstd[c0 + e];
        ga[e] = a.gamma[c0 + e];
        be[e] = a.beta[c0 + e];
    }
    constexpr int NP = POOL ? 4 : 1;
    size_t src[NP];
    if constexpr (POOL) {
        const size_t Ho = a.H >> 1, Wo = a.W >> 1;
        const size_t b = o / (Ho * Wo), r = o - b * Ho * Wo, yo = r / Wo, xo = r - yo * Wo;
        const size_t base = (b * a.H + 2 * yo) * a.W + 2 * xo;
#pragma unroll
        for (int s = 0; s < 4; ++s) src[s] = base + (size_t)(s >> 1) * a.W + (s & 1);
    } else {
        src[0] = o;
    }
    float v[NP][8];
#pragma unroll
    for (int s = 0; s < NP; ++s) {
        float z[8];
        unpack8_(*(const uint4 *)(a.z + src[s] * a.C + c0), z);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xhat = (z[e] - mu[e]) * is[e];
            const float y = xhat * ga[e] + be[e];
            v[s][e] = y > 0.f ? y : y * SLOPE;
        }
    }
    if constexpr (POOL) {
        float best[8];
        unsigned int pos[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            best[e] = v[0][e];
            unsigned int w = 0;
#pragma unroll
            for (int s = 1; s < 4; ++s)
                if (v[s][e] > best[e]) {
                    best[e] = v[s][e];
                    w = s;
                }
            pos[e >> 2] |= w << (8 * (e & 3));
        }
        *(uint4 *)(a.out + o * a.C + c0) = rb8_(best);
        *(uint2 *)(a.idx + o * a.C + c0) = uint2{pos[0], pos[1]};
    } else {
        *(uint4 *)(a.out + o * a.C + c0) = rb8_(v[0]);
    }
}

struct ApplyArgs {
    const bf16_t *dy, *z;
    const float *mean, *invstd, *m1, *m2, *gs;
    bf16_t *out;                     // G_k
    size_t N;
    int C, cg_log2;
};

__global__ __launch_bounds__(256) void bn_apply_kernel(const ApplyArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t p = i >> a.cg_log2;
    if (p >= a.N) return;
    const int c0 = (int)(i & (((size_t)1 << a.cg_log2) - 1)) * 8;
    float z[8], d[8], g[8];
    unpack8_(*(const uint4 *)(a.z + p * a.C + c0), z);
    unpack8_(*(const uint4 *)(a.dy + p * a.C + c0), d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float xhat = (z[e] - a.mean[c0 + e]) * a.invstd[c0 + e];
        float t = d[e] - a.m1[c0 + e];
        t = t - xhat * a.m2[c0 + e];
        g[e] = t * a.gs[c0 + e];
    }
    *(uint4 *)(a.out + p * a.C + c0) = rb8_(g);
}

// train_sgd_kernel's update on gamma and beta of every layer (n elements, no packs)
__global__ __launch_bounds__(256) void bn_sgd_kernel(size_t n, float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ buf, float lr,
                                                     float momentum, float weight_decay, int first) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float w = p[i];
    float gr = grad[i];
    gr = gr + weight_decay * w;
    const float b = first ? gr : momentum * buf[i] + gr;
    buf[i] = b;
    p[i] = w - lr * b;
}

// ---------------------------------------------------------------------------------------------------------- the handle
struct y355_bntrain {
    DevOwner own;
    int device_id = 0;
    int max_h = 0, max_w = 0, max_batch = 0, num_classes = 0, num_anchors = 0;
    int H = 0, W = 0;
    int batch = 0;                   // of the last forward at this size (0: none)
    bool have_stats = false;         // a forward since create (batch statistics exist, whatever the size)
    bool have_grad = false;          // a backward since the last forward
    long long steps = 0;
    long long nbt[NBN] = {};         // num_batches_tracked
    NetDesc d;
    size_t coff[NBN] = {}, cs = 0;   // of a layer's channels in the per-channel arrays; their sum
    size_t pack_total = 0, ws_total = 0;
    float *p = nullptr, *g = nullptr, *m = nullptr;
    float *bnp = nullptr, *bng = nullptr, *bnm = nullptr;      // [gamma | beta], each cs
    float *rstat = nullptr;          // [running_mean | running_var]
    float *bstat = nullptr;          // [mean | var | invstd] of the last forward
    float *coef = nullptr;           // [m1 | m2 | gamma invstd] of the last backward
    double *sws = nullptr;           // the reductions' partials
    bf16_t *packs = nullptr;
    bf16_t *act[NL] = {};            // A_0 .. A_9
    unsigned char *idx[NL] = {};     // I_t, t = 1, 2, 4, 6 (index t)
    bf16_t *z[NL] = {};              // Z_1 .. Z_9 (index k)
    bf16_t *dy[NL] = {};             // dY_1 .. dY_9 (index k)
    bf16_t *grad[NL + 1] = {};       // G_1 .. G_10 (index k)
    float *pred = nullptr, *ws = nullptr;
};

// channels and grid divisor of A_t
static int act_c(const y355_bntrain *h, int t) { return t == 0 ? 8 : h->d.L[t - 1].cout; }
static int act_div(int t) { return t == 0 ? 1 : kDiv[t - 1] * (kPool[t - 1] ? 2 : 1); }

// The split of a BatchNorm layer's N = B h w pixels into runs of chunk pixels (a multiple of STAT_ALIGN; the last run may be
// shorter), at most STAT_MAX_RUNS of them: of the batch and the layer's grid alone.  Forward and backward launch from it and
// y355_bntrain_stats_plan reports it.
struct StatsPlan {
    size_t N, chunk;
    int runs;
};
static StatsPlan stats_plan(int B, int H, int W) {
    StatsPlan p;
    p.N = (size_t)B * H * W;
    const size_t want = std::min<size_t>((size_t)STAT_MAX_RUNS, (p.N + STAT_ALIGN - 1) / STAT_ALIGN);
    p.chunk = ((p.N + want - 1) / want + STAT_ALIGN - 1) / STAT_ALIGN * STAT_ALIGN;
    p.runs = (int)((p.N + p.chunk - 1) / p.chunk);
    return p;
}

// y355_bntrain_create in two parts, as bntrain_host_check.cpp runs them on the CPU: the rules and the host state (no device
// call), ...
int bntrain_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_bntrain **out) {
    if (!out) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_create: null argument");
    *out = nullptr;
    if (max_h < 16 || max_w < 16 || max_h % 16 || max_w % 16 || max_h > 4096 || max_w > 4096)
        return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_create: max_h and max_w must be multiples of 16 in 16..4096");
    if (num_classes < 1 || num_classes > 200) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_create: num_classes must be 1..200");
    if (num_anchors < 1 || num_anchors > 16) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_create: num_anchors must be 1..16");
    if (max_batch < 1 || max_batch > 1024) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_create: max_batch must be 1..1024");
    y355_bntrain *h = new y355_bntrain;
    h->own = DevOwner{mem, {}};
    h->max_h = h->H = max_h;
    h->max_w = h->W = max_w;
    h->max_batch = max_batch;
    h->num_classes = num_classes;
    h->num_anchors = num_anchors;
    size_t off = 0, poff = 0;
    for (int k = 0; k < NL; ++k) {
        LayerDesc &L = h->d.L[k];
        L.cin = kCin[k];
        L.cinp = k == 0 ? 8 : kCin[k];
        L.cout = k == NL - 1 ? num_anchors * (5 + num_classes) : kCout[k];
        L.coutp = k == NL - 1 ? pow2_at_least(L.cout, 32) : L.cout;
        L.ct = tiles_per_wave(L.cout);
        L.ksf = (9 * L.cinp + 31) / 32;
        L.ksd = 9 * L.coutp / 32;
        L.dct = tiles_per_wave(L.cin);
        L.woff = off;
        off += (size_t)L.cout * L.cin * 9;
        L.boff = off;
        off += L.cout;
        const int tf = ((L.cout + 15) / 16 + L.ct - 1) / L.ct * L.ct;
        L.wf_off = poff;
        poff += (size_t)tf * L.ksf * 512;
        L.wd_off = poff;
        if (k > 0) poff += (size_t)(L.cin / 16) * L.ksd * 512;
        h->ws_total = std::max(h->ws_total, (size_t)wgrad_max_runs(L) * wgrad_stride(L));
        if (k < NBN) {
            h->coff[k] = h->cs;
            h->cs += L.cout;
        }
    }
    h->d.total = off;
    h->pack_total = poff;
    *out = h;
    return Y355_BNTRAIN_OK;
}
// ... and all of its device memory (on the current device) with BatchNorm2d's initial values, or none of it
int bntrain_buffers(y355_bntrain *h) {
    DevOwner &o = h->own;
    const size_t mark = y355_dev_mark(o);
    const size_t B = h->max_batch;
    int rc = y355_dev_get_all<true>(o, h->d.total, &h->p, &h->g, &h->m);
    rc = rc ? rc : y355_dev_get_all<true>(o, 2 * h->cs, &h->bnp, &h->bng, &h->bnm);
    rc = rc ? rc : y355_dev_get_all<true>(o, 2 * h->cs, &h->rstat);
    rc = rc ? rc : y355_dev_get_all<true>(o, 3 * h->cs, &h->bstat, &h->coef);
    rc = rc ? rc : y355_dev_get(o, &h->sws, (size_t)STAT_MAX_RUNS * 2 * 256, true);
    rc = rc ? rc : y355_dev_get(o, &h->packs, h->pack_total, true);
    rc = rc ? rc : y355_dev_get(o, &h->ws, h->ws_total, true);
    for (int t = 0; t < NL && !rc; ++t) {
        const size_t n = B * (h->max_h / act_div(t)) * (h->max_w / act_div(t)) * act_c(h, t);
        rc = y355_dev_get(o, &h->act[t], n, true);
        if (!rc && t >= 1 && kPool[t - 1]) rc = y355_dev_get(o, &h->idx[t], n, true);
    }
    for (int k = 1; k <= NL && !rc; ++k) {
        const size_t n = B * (h->max_h / kDiv[k - 1]) * (h->max_w / kDiv[k - 1]) * h->d.L[k - 1].coutp;
        rc = y355_dev_get(o, &h->grad[k], n, true);
        if (k <= NBN) {
            rc = rc ? rc : y355_dev_get(o, &h->z[k], n, true);
            rc = rc ? rc : y355_dev_get(o, &h->dy[k], n, true);
        }
    }
    rc = rc ? rc : y355_dev_get(o, &h->pred, B * h->d.L[NL - 1].cout * (h->max_h / 16) * (h->max_w / 16), true);
    if (!rc) {                                                // gamma = 1, running_var = 1
        const std::vector<float> ones(h->cs, 1.0f);
        rc = o.mem.upload(h->bnp, ones.data(), h->cs * sizeof(float), nullptr);
        rc = rc ? rc : o.mem.upload(h->rstat + h->cs, ones.data(), h->cs * sizeof(float), nullptr);
    }
    if (rc) {
        y355_dev_rollback(o, mark);
        h->p = h->g = h->m = h->bnp = h->bng = h->bnm = h->rstat = h->bstat = h->coef = h->ws = h->pred = nullptr;
        h->sws = nullptr;
        h->packs = nullptr;
        for (int t = 0; t < NL; ++t) {
            h->act[t] = nullptr;
            h->idx[t] = nullptr;
            h->z[t] = nullptr;
            h->dy[t] = nullptr;
            h->grad[t + 1] = nullptr;
        }
    }
    return rc;
}
DevOwner &bntrain_owner(y355_bntrain *h) { return h->own; }  // (bntrain_host_check.cpp does not see the struct)
void bntrain_free(y355_bntrain *h) {
    y355_dev_release_all(h->own);
    delete h;
}
void bntrain_state(const y355_bntrain *h, int *hw_batch) {   // H, W, batch of the last forward, have_grad: for the host check
    hw_batch[0] = h->H;
    hw_batch[1] = h->W;
    hw_batch[2] = h->batch;
    hw_batch[3] = h->have_grad ? 1 : 0;
}

static int layer_arg(const char *who, const y355_bntrain *h, int k, int last = NL) {
    if (!h) return y355_fail(Y355_BNTRAIN_EINVAL, std::string(who) + ": null handle");
    if (k < 1 || k > last) return y355_fail(Y355_BNTRAIN_EINVAL, std::string(who) + (last == NL ? ": layer index must be 1..10" : ": layer index must be 1..9"));
    return 0;
}

static hipError_t launch_pack(y355_bntrain *h, float lr, float momentum, float wd, int first, int update, hipStream_t s) {
    hipLaunchKernelGGL(train_sgd_kernel, dim3((unsigned)((h->d.total + 255) / 256)), dim3(256), 0, s, h->d, h->p, h->g, h->m, h->packs, lr, momentum,
                       wd, first, update);
    return hipGetLastError();
}

// [B, h, w, c] of a tensor at the current size; false on a kind / index that does not exist
static bool tensor_dims(const y355_bntrain *h, int kind, int t, int *shape) {
    int div, c;
    if (kind == Y355_BNTRAIN_ACT && t >= 0 && t <= 9) {
        div = act_div(t);
        c = act_c(h, t);
    } else if (kind == Y355_BNTRAIN_IDX && t >= 1 && t <= 9 && kPool[t - 1]) {
        div = act_div(t);
        c = act_c(h, t);
    } else if (kind == Y355_BNTRAIN_GRAD && t >= 1 && t <= NL) {
        div = kDiv[t - 1];
        c = h->d.L[t - 1].coutp;
    } else if ((kind == Y355_BNTRAIN_Z || kind == Y355_BNTRAIN_DY) && t >= 1 && t <= NBN) {
        div = kDiv[t - 1];
        c = h->d.L[t - 1].cout;
    } else {
        return false;
    }
    shape[0] = h->batch;
    shape[1] = h->H / div;
    shape[2] = h->W / div;
    shape[3] = c;
    return true;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_bntrain_last_error(void) { return g_err.c_str(); }

int y355_bntrain_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_bntrain **out) {
    if (int rc = bntrain_open(max_h, max_w, num_classes, num_anchors, max_batch, y355_hip_mem(), out)) return rc;
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    (*out)->device_id = dev;
    const int rc = e != hipSuccess ? y355_fail(Y355_BNTRAIN_EHIP, std::string("y355_bntrain_create: ") + hipGetErrorString(e)) : bntrain_buffers(*out);
    if (rc) {
        bntrain_free(*out);
        *out = nullptr;
    }
    return rc;
}

void y355_bntrain_destroy(y355_bntrain *h) {
    if (!h) return;
    DeviceGuard g;
    (void)g.set(h->device_id);
    bntrain_free(h);
}

int y355_bntrain_set_size(y355_bntrain *h, int32_t height, int32_t width) {
    if (!h) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_set_size: null handle");
    if (height < 16 || width < 16 || height % 16 || width % 16)
        return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_set_size: height and width must be multiples of 16");
    if (height > h->max_h || width > h->max_w) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_set_size: size beyond the handle's maximum");
    if (height != h->H || width != h->W) {
        h->H = height;
        h->W = width;
        h->batch = 0;                                         // the stored tensors are of another size
        h->have_grad = false;
    }
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_layer_shape(const y355_bntrain *h, int32_t k, int32_t *shape) {
    if (int rc = layer_arg("y355_bntrain_layer_shape", h, k)) return rc;
    if (!shape) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_layer_shape: null argument");
    shape[0] = h->d.L[k - 1].cout;
    shape[1] = h->d.L[k - 1].cin;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_load_layer(y355_bntrain *h, int32_t k, const float *w, const float *b) {
    if (int rc = layer_arg("y355_bntrain_load_layer", h, k)) return rc;
    if (!w || !b) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_load_layer: null argument");
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->p + L.woff, w, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->p + L.boff, b, (size_t)L.cout * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(launch_pack(h, 0.f, 0.f, 0.f, 0, 0, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return Y355_BNTRAIN_OK;
}

static int get_pair(const char *who, y355_bntrain *h, int k, const float *src, float *w, float *b) {
    if (int rc = layer_arg(who, h, k)) return rc;
    const LayerDesc &L = h->d.L[k - 1];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    if (w) HIPCHK(hipMemcpy(w, src + L.woff, (size_t)L.cout * L.cin * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (b) HIPCHK(hipMemcpy(b, src + L.boff, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_BNTRAIN_OK;
}

// n per-channel arrays of layer k, the i-th at src + i * stride + coff, to the host pointers that are not null
static int get_channels(y355_bntrain *h, int k, const float *src, size_t stride, int n, float *const *dst) {
    const size_t c = h->d.L[k - 1].cout;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < n; ++i)
        if (dst[i]) HIPCHK(hipMemcpy(dst[i], src + i * stride + h->coff[k - 1], c * sizeof(float), hipMemcpyDeviceToHost));
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_get_layer(y355_bntrain *h, int32_t k, float *w, float *b) { return get_pair("y355_bntrain_get_layer", h, k, h ? h->p : nullptr, w, b); }

int y355_bntrain_get_grad(y355_bntrain *h, int32_t k, float *dw, float *db) {
    if (int rc = layer_arg("y355_bntrain_get_grad", h, k)) return rc;
    if (!h->have_grad) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_get_grad: no backward pass has run");
    return get_pair("y355_bntrain_get_grad", h, k, h->g, dw, db);
}

int y355_bntrain_get_momentum(y355_bntrain *h, int32_t k, float *mw, float *mb) {
    return get_pair("y355_bntrain_get_momentum", h, k, h ? h->m : nullptr, mw, mb);
}

int y355_bntrain_load_bn(y355_bntrain *h, int32_t k, const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                         int64_t num_batches_tracked) {
    if (int rc = layer_arg("y355_bntrain_load_bn", h, k, NBN)) return rc;
    if (!gamma || !beta || !running_mean || !running_var) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_load_bn: null argument");
    if (num_batches_tracked < 0) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_load_bn: num_batches_tracked must not be negative");
    const size_t c = h->d.L[k - 1].cout, off = h->coff[k - 1], bytes = c * sizeof(float);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->bnp + off, gamma, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->bnp + h->cs + off, beta, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->rstat + off, running_mean, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->rstat + h->cs + off, running_var, bytes, hipMemcpyHostToDevice));
    h->nbt[k - 1] = num_batches_tracked;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_get_bn(y355_bntrain *h, int32_t k, float *gamma, float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked) {
    if (int rc = layer_arg("y355_bntrain_get_bn", h, k, NBN)) return rc;
    float *const pb[2] = {gamma, beta}, *const rs[2] = {running_mean, running_var};
    if (int rc = get_channels(h, k, h->bnp, h->cs, 2, pb)) return rc;
    if (int rc = get_channels(h, k, h->rstat, h->cs, 2, rs)) return rc;
    if (num_batches_tracked) *num_batches_tracked = h->nbt[k - 1];
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_get_bn_grad(y355_bntrain *h, int32_t k, float *dgamma, float *dbeta) {
    if (int rc = layer_arg("y355_bntrain_get_bn_grad", h, k, NBN)) return rc;
    if (!h->have_grad) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_get_bn_grad: no backward pass has run");
    float *const d[2] = {dgamma, dbeta};
    return get_channels(h, k, h->bng, h->cs, 2, d);
}

int y355_bntrain_get_bn_momentum(y355_bntrain *h, int32_t k, float *mgamma, float *mbeta) {
    if (int rc = layer_arg("y355_bntrain_get_bn_momentum", h, k, NBN)) return rc;
    float *const d[2] = {mgamma, mbeta};
    return get_channels(h, k, h->bnm, h->cs, 2, d);
}

int y355_bntrain_get_batch_stats(y355_bntrain *h, int32_t k, float *mean, float *var, float *invstd) {
    if (int rc = layer_arg("y355_bntrain_get_batch_stats", h, k, NBN)) return rc;
    if (!h->have_stats) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_get_batch_stats: no forward pass has run");
    float *const d[3] = {mean, var, invstd};
    return get_channels(h, k, h->bstat, h->cs, 3, d);
}

int y355_bntrain_get_packed(y355_bntrain *h, int32_t k, uint16_t *w_bf16) {
    if (int rc = layer_arg("y355_bntrain_get_packed", h, k)) return rc;
    if (!w_bf16) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_get_packed: null argument");
    const LayerDesc &L = h->d.L[k - 1];
    const int tf = ((L.cout + 15) / 16 + L.ct - 1) / L.ct * L.ct;
    std::vector<bf16_t> pk((size_t)tf * L.ksf * 512);
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pk.data(), h->packs + L.wf_off, pk.size() * sizeof(bf16_t), hipMemcpyDeviceToHost));
    for (int co = 0; co < L.cout; ++co)
        for (int ci = 0; ci < L.cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                const int kidx = tap * L.cinp + ci;
                w_bf16[((size_t)co * L.cin + ci) * 9 + tap] =
                    pk[((((size_t)(co >> 4) * L.ksf + (kidx >> 5)) * 64 + ((kidx >> 3) & 3) * 16 + (co & 15)) << 3) + (kidx & 7)];
            }
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_forward(y355_bntrain *h, const void *x_dev, int32_t batch, void *stream) {
    if (!h || !x_dev) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_forward: null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_forward: batch must be 1..max_batch");
    if ((long long)batch * (h->H / 16) * (h->W / 16) < 2)
        return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_forward: BatchNorm in training mode needs more than one value per channel: batch * H/16 * W/16 >= 2");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->batch = 0;
    h->have_grad = false;
    const size_t npix = (size_t)batch * h->H * h->W;
    hipLaunchKernelGGL(train_input_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const float *)x_dev, h->act[0], npix,
                       (size_t)h->H * h->W);
    HIPCHK(hipGetLastError());
    for (int k = 1; k <= NL; ++k) {
        const LayerDesc &L = h->d.L[k - 1];
        ConvArgs a{};
        a.in = h->act[k - 1];
        a.w = h->packs + L.wf_off;
        a.bias = h->p + L.boff;
        a.cinp_log2 = ilog2_(L.cinp);
        a.ks = L.ksf;
        a.B = batch;
        a.H = h->H / kDiv[k - 1];
        a.W = h->W / kDiv[k - 1];
        a.cout = L.cout;
        a.outc = L.cout;
        const int tiles = (L.cout + 15) / 16;
        if (k == NL) {
            a.out = h->pred;
            HIPCHK(launch_conv<M_PRED>(a, L.ct, tiles, s));
            break;
        }
        a.out = h->z[k];
        HIPCHK(launch_conv<M_Z>(a, L.ct, tiles, s));
        const size_t off = h->coff[k - 1], cs = h->cs;
        const int cgl = ilog2_(L.cout / 8);
        const StatsPlan plan = stats_plan(batch, a.H, a.W);
        StatArgs sa{};
        sa.z = h->z[k];
        sa.ws = h->sws;
        sa.N = plan.N;
        sa.chunk = plan.chunk;
        sa.C = L.cout;
        sa.cg_log2 = cgl;
        hipLaunchKernelGGL((bn_stats_kernel<false>), dim3((unsigned)plan.runs), dim3(256), 0, s, sa);
        HIPCHK(hipGetLastError());
        FinArgs fa{};
        fa.ws = h->sws;
        fa.runs = plan.runs;
        fa.C = L.cout;
        fa.N = (double)plan.N;
        fa.mean = h->bstat + off;
        fa.var = h->bstat + cs + off;
        fa.invstd = h->bstat + 2 * cs + off;
        fa.rmean = h->rstat + off;
        fa.rvar = h->rstat + cs + off;
        hipLaunchKernelGGL((bn_finalise_kernel<false>), dim3((unsigned)((L.cout + 255) / 256)), dim3(256), 0, s, fa);
        HIPCHK(hipGetLastError());
        ++h->nbt[k - 1];
        NormArgs na{};
        na.z = h->z[k];
        na.mean = fa.mean;
        na.invstd = fa.invstd;
        na.gamma = h->bnp + off;
        na.beta = h->bnp + cs + off;
        na.out = h->act[k];
        na.H = a.H;
        na.W = a.W;
        na.C = L.cout;
        na.cg_log2 = cgl;
        if (kPool[k - 1]) {
            na.idx = h->idx[k];
            na.nout = plan.N / 4;
            hipLaunchKernelGGL((bn_norm_kernel<true>), dim3((unsigned)(((na.nout << cgl) + 255) / 256)), dim3(256), 0, s, na);
        } else {
            na.nout = plan.N;
            hipLaunchKernelGGL((bn_norm_kernel<false>), dim3((unsigned)(((na.nout << cgl) + 255) / 256)), dim3(256), 0, s, na);
        }
        HIPCHK(hipGetLastError());
        h->have_stats = true;
    }
    h->batch = batch;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_pred(y355_bntrain *h, void **out) {
    if (!h || !out) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_pred: null argument");
    *out = h->pred;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_backward(y355_bntrain *h, const void *dpred_dev, void *stream) {
    if (!h || !dpred_dev) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_backward: null argument");
    if (h->batch == 0) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_backward: no forward pass has run at this size");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    h->have_grad = false;
    const int B = h->batch;
    {
        const LayerDesc &L = h->d.L[NL - 1];
        const size_t hw = (size_t)(h->H / 16) * (h->W / 16), n = (size_t)B * hw * L.coutp;
        hipLaunchKernelGGL(train_dpred_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)dpred_dev, h->grad[NL], n, L.cout,
                           ilog2_(L.coutp), hw);
        HIPCHK(hipGetLastError());
    }
    for (int k = NL; k >= 1; --k) {
        const LayerDesc &L = h->d.L[k - 1];
        const int H = h->H / kDiv[k - 1], W = h->W / kDiv[k - 1];
        if (k <= NBN) {                                       // dY_k -> dgamma_k, dbeta_k, G_k
            const size_t off = h->coff[k - 1], cs = h->cs;
            const int cgl = ilog2_(L.cout / 8);
            const StatsPlan plan = stats_plan(B, H, W);
            StatArgs sa{};
            sa.z = h->z[k];
            sa.dy = h->dy[k];
            sa.mean = h->bstat + off;
            sa.invstd = h->bstat + 2 * cs + off;
            sa.ws = h->sws;
            sa.N = plan.N;
            sa.chunk = plan.chunk;
            sa.C = L.cout;
            sa.cg_log2 = cgl;
            hipLaunchKernelGGL((bn_stats_kernel<true>), dim3((unsigned)plan.runs), dim3(256), 0, s, sa);
            HIPCHK(hipGetLastError());
            FinArgs fa{};
            fa.ws = h->sws;
            fa.runs = plan.runs;
            fa.C = L.cout;
            fa.N = (double)plan.N;
            fa.Nf = (float)plan.N;
            fa.invstd = h->bstat + 2 * cs + off;
            fa.gamma = h->bnp + off;
            fa.dgamma = h->bng + off;
            fa.dbeta = h->bng + cs + off;
            fa.m1 = h->coef + off;
            fa.m2 = h->coef + cs + off;
            fa.gs = h->coef + 2 * cs + off;
            hipLaunchKernelGGL((bn_finalise_kernel<true>), dim3((unsigned)((L.cout + 255) / 256)), dim3(256), 0, s, fa);
            HIPCHK(hipGetLastError());
            ApplyArgs aa{};
            aa.dy = h->dy[k];
            aa.z = h->z[k];
            aa.mean = sa.mean;
            aa.invstd = sa.invstd;
            aa.m1 = fa.m1;
            aa.m2 = fa.m2;
            aa.gs = fa.gs;
            aa.out = h->grad[k];
            aa.N = plan.N;
            aa.C = L.cout;
            aa.cg_log2 = cgl;
            hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)(((plan.N << cgl) + 255) / 256)), dim3(256), 0, s, aa);
            HIPCHK(hipGetLastError());
        }
        WgradArgs wa{};
        wa.g = h->grad[k];
        wa.act = h->act[k - 1];
        wa.ws = h->ws;
        wa.ws_stride = wgrad_stride(L);
        const WgradPlan plan = wgrad_plan(L, B, H, W);
        const int runs = plan.runs;
        wa.npix = plan.npix;
        wa.chunk = plan.chunk;
        wa.H = H;
        wa.W = W;
        wa.cinp = L.cinp;
        wa.coutp = L.coutp;
        wa.cout = L.cout;
        const int mt = wgrad_mt(L);
        const dim3 grid((unsigned)((L.cinp + 15) / 16), (unsigned)((L.cout + 16 * mt - 1) / (16 * mt)), (unsigned)runs), block(64);
        if (mt == 1) hipLaunchKernelGGL((train_wgrad_kernel<1>), grid, block, 0, s, wa);
        else if (mt == 2) hipLaunchKernelGGL((train_wgrad_kernel<2>), grid, block, 0, s, wa);
        else hipLaunchKernelGGL((train_wgrad_kernel<4>), grid, block, 0, s, wa);
        HIPCHK(hipGetLastError());
        const size_t n = (size_t)L.cout * L.cin * 9 + L.cout;
        hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->ws, wa.ws_stride, runs, L.cin, L.cinp, L.cout,
                           h->g + L.woff, h->g + L.boff);
        HIPCHK(hipGetLastError());
        if (k == 1) break;                                    // the gradient with respect to the image is not computed
        ConvArgs a{};
        a.in = h->grad[k];
        a.w = h->packs + L.wd_off;
        a.cinp_log2 = ilog2_(L.coutp);
        a.ks = L.ksd;
        a.B = B;
        a.H = H;
        a.W = W;
        a.cout = L.cin;
        a.outc = L.cin;
        a.out = h->dy[k - 1];
        a.act_prev = h->act[k - 1];
        if (kPool[k - 2]) {
            a.idx_prev = h->idx[k - 1];
            HIPCHK(launch_conv<M_DGRAD_UNPOOL>(a, L.dct, L.cin / 16, s));
        } else {
            HIPCHK(launch_conv<M_DGRAD>(a, L.dct, L.cin / 16, s));
        }
    }
    h->have_grad = true;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_wgrad_plan(const y355_bntrain *h, int32_t k, int32_t batch, int32_t *out) {
    if (int rc = layer_arg("y355_bntrain_wgrad_plan", h, k)) return rc;
    if (!out) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_wgrad_plan: null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_wgrad_plan: batch must be 1..max_batch");
    const WgradPlan p = wgrad_plan(h->d.L[k - 1], batch, h->H / kDiv[k - 1], h->W / kDiv[k - 1]);
    if (p.npix > (size_t)INT32_MAX) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_wgrad_plan: more than 2^31 - 1 pixels");
    out[0] = (int32_t)p.npix;
    out[1] = p.max_runs;
    out[2] = p.runs;
    out[3] = (int32_t)p.chunk;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_stats_plan(const y355_bntrain *h, int32_t k, int32_t batch, int32_t *out) {
    if (int rc = layer_arg("y355_bntrain_stats_plan", h, k, NBN)) return rc;
    if (!out) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_stats_plan: null argument");
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_stats_plan: batch must be 1..max_batch");
    const StatsPlan p = stats_plan(batch, h->H / kDiv[k - 1], h->W / kDiv[k - 1]);
    if (p.N > (size_t)INT32_MAX) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_stats_plan: more than 2^31 - 1 pixels");
    out[0] = (int32_t)p.N;
    out[1] = p.runs;
    out[2] = (int32_t)p.chunk;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_sgd_step(y355_bntrain *h, float lr, float momentum, float weight_decay, void *stream) {
    if (!h) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_sgd_step: null handle");
    if (!(lr == lr) || !(momentum == momentum) || !(weight_decay == weight_decay))
        return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_sgd_step: lr, momentum and weight_decay must be numbers");
    if (!h->have_grad) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_sgd_step: no backward pass has run");
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    const int first = h->steps == 0 ? 1 : 0;
    HIPCHK(launch_pack(h, lr, momentum, weight_decay, first, 1, (hipStream_t)stream));
    hipLaunchKernelGGL(bn_sgd_kernel, dim3((unsigned)((2 * h->cs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, 2 * h->cs, h->bnp, h->bng, h->bnm, lr,
                       momentum, weight_decay, first);
    HIPCHK(hipGetLastError());
    ++h->steps;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_tensor_shape(const y355_bntrain *h, int32_t kind, int32_t t, int32_t *shape) {
    if (!h || !shape) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_tensor_shape: null argument");
    if (!tensor_dims(h, kind, t, shape)) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_tensor_shape: no such tensor");
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_get_tensor(y355_bntrain *h, int32_t kind, int32_t t, void *out) {
    if (!h || !out) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_get_tensor: null argument");
    int shape[4];
    if (!tensor_dims(h, kind, t, shape)) return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_get_tensor: no such tensor");
    if (h->batch == 0) return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_get_tensor: no forward pass has run at this size");
    if ((kind == Y355_BNTRAIN_GRAD || kind == Y355_BNTRAIN_DY) && !h->have_grad)
        return y355_fail(Y355_BNTRAIN_ENOTREADY, "y355_bntrain_get_tensor: no backward pass has run");
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * shape[3];
    const void *src = kind == Y355_BNTRAIN_ACT   ? (const void *)h->act[t]
                      : kind == Y355_BNTRAIN_IDX ? (const void *)h->idx[t]
                      : kind == Y355_BNTRAIN_Z   ? (const void *)h->z[t]
                      : kind == Y355_BNTRAIN_DY  ? (const void *)h->dy[t]
                                                 : (const void *)h->grad[t];
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, src, n * (kind == Y355_BNTRAIN_IDX ? 1 : 2), hipMemcpyDeviceToHost));
    return Y355_BNTRAIN_OK;
}

}  // extern "C"
