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
//
// The handle's common state, the create rules, the common device memory, the bodies of the entry points yolo355_train.h has
// too and the convolutions' launches are train_host.h's (train.hip compiles it too).  This file owns the BatchNorm kernels,
// state, memory and entry points, the reductions' plan, and the two passes' loops with the BatchNorm launches between
// train_host.h's.
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

#define TRAIN_FAMILY "y355_bntrain"
#include "train_core.h"
#include "train_host.h"
static_assert(NL == Y355_BNTRAIN_LAYERS, "train_core.h's layer table");
static_assert(Y355_BNTRAIN_ACT == T_ACT && Y355_BNTRAIN_IDX == T_IDX && Y355_BNTRAIN_GRAD == T_GRAD, "train_host.h's tensor kinds");
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
struct BnDev {                       // BatchNorm's device memory, the owner's too: bntrain_buffers resets it in one assignment
    float *bnp = nullptr, *bng = nullptr, *bnm = nullptr;      // [gamma | beta], each cs
    float *rstat = nullptr;          // [running_mean | running_var]
    float *bstat = nullptr;          // [mean | var | invstd] of the last forward
    float *coef = nullptr;           // [m1 | m2 | gamma invstd] of the last backward
    double *sws = nullptr;           // the reductions' partials
    bf16_t *z[NL] = {};              // Z_1 .. Z_9 (index k)
    bf16_t *dy[NL] = {};             // dY_1 .. dY_9 (index k)
};
struct y355_bntrain : TrainCore, BnDev {
    bool have_stats = false;         // a forward since create (batch statistics exist, whatever the size)
    long long nbt[NBN] = {};         // num_batches_tracked
    size_t coff[NBN] = {}, cs = 0;   // of a layer's channels in the per-channel arrays; their sum
};

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

// The seams of bntrain_host_check.cpp, which does not see the struct.  y355_bntrain_create in two parts: train_host.h's rules
// and host state with the per-channel offsets on top, ...
int bntrain_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_bntrain **out) {
    if (int rc = core_open(max_h, max_w, num_classes, num_anchors, max_batch, mem, out)) return rc;
    y355_bntrain *h = *out;
    for (int k = 0; k < NBN; ++k) {
        h->coff[k] = h->cs;
        h->cs += h->d.L[k].cout;
    }
    return Y355_BNTRAIN_OK;
}
// ... and all of its device memory (on the current device) with BatchNorm2d's initial values, or none of it: the per-channel
// arrays and the partials follow the parameters, Z_k and dY_k follow G_k
int bntrain_buffers(y355_bntrain *h) {
    DevOwner &o = h->own;
    const size_t mark = y355_dev_mark(o);
    int rc = core_buffers(
        h,
        [&] {
            int r = y355_dev_get_all<true>(o, 2 * h->cs, &h->bnp, &h->bng, &h->bnm);
            r = r ? r : y355_dev_get_all<true>(o, 2 * h->cs, &h->rstat);
            r = r ? r : y355_dev_get_all<true>(o, 3 * h->cs, &h->bstat, &h->coef);
            return r ? r : y355_dev_get(o, &h->sws, (size_t)STAT_MAX_RUNS * 2 * 256, true);
        },
        [&](int k, size_t n) {
            if (k > NBN) return 0;
            const int r = y355_dev_get(o, &h->z[k], n, true);
            return r ? r : y355_dev_get(o, &h->dy[k], n, true);
        });
    if (!rc) {                                                // gamma = 1, running_var = 1
        const std::vector<float> ones(h->cs, 1.0f);
        rc = o.mem.upload(h->bnp, ones.data(), h->cs * sizeof(float), nullptr);
        rc = rc ? rc : o.mem.upload(h->rstat + h->cs, ones.data(), h->cs * sizeof(float), nullptr);
        if (rc) core_rollback(h, mark);
    }
    if (rc) static_cast<BnDev &>(*h) = BnDev{};
    return rc;
}
DevOwner &bntrain_owner(y355_bntrain *h) { return h->own; }
void bntrain_free(y355_bntrain *h) { core_free(h); }
void bntrain_state(const y355_bntrain *h, int *hw_batch) { core_state(h, hw_batch); }

// Z_t and dY_t, t = 1..9: the tensor kinds yolo355_train.h does not have
static OwnTensor bn_tensor(const TrainCore *hc, int kind, int t) {
    const y355_bntrain *h = static_cast<const y355_bntrain *>(hc);
    if ((kind != Y355_BNTRAIN_Z && kind != Y355_BNTRAIN_DY) || t < 1 || t > NBN) return OwnTensor{nullptr, 0, false};
    return kind == Y355_BNTRAIN_Z ? OwnTensor{h->z[t], h->d.L[t - 1].cout, false} : OwnTensor{h->dy[t], h->d.L[t - 1].cout, true};
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

// BatchNorm of layer k = 1..9 in the forward, Z_k -> A_k (and I_k): the batch statistics, the running ones, the normalisation
static int bn_forward(y355_bntrain *h, int k, int batch, hipStream_t s) {
    const LayerDesc &L = h->d.L[k - 1];
    const int H = h->H / kDiv[k - 1], W = h->W / kDiv[k - 1];
    const size_t off = h->coff[k - 1], cs = h->cs;
    const int cgl = ilog2_(L.cout / 8);
    const StatsPlan plan = stats_plan(batch, H, W);
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
    na.H = H;
    na.W = W;
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
    return Y355_BNTRAIN_OK;
}

// ... and in the backward, dY_k -> dgamma_k, dbeta_k, G_k
static int bn_backward(y355_bntrain *h, int k, hipStream_t s) {
    const LayerDesc &L = h->d.L[k - 1];
    const size_t off = h->coff[k - 1], cs = h->cs;
    const int cgl = ilog2_(L.cout / 8);
    const StatsPlan plan = stats_plan(h->batch, h->H / kDiv[k - 1], h->W / kDiv[k - 1]);
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
    return Y355_BNTRAIN_OK;
}
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_bntrain_last_error(void) { return g_err.c_str(); }

// what yolo355_train.h has too: train_host.h's bodies
int y355_bntrain_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_bntrain **out) {
    return core_create(max_h, max_w, num_classes, num_anchors, max_batch, out, bntrain_open, bntrain_buffers);
}
void y355_bntrain_destroy(y355_bntrain *h) { core_destroy(h); }
int y355_bntrain_set_size(y355_bntrain *h, int32_t height, int32_t width) { return core_set_size(h, height, width); }
int y355_bntrain_layer_shape(const y355_bntrain *h, int32_t k, int32_t *shape) { return core_layer_shape(h, k, shape); }
int y355_bntrain_load_layer(y355_bntrain *h, int32_t k, const float *w, const float *b) { return core_load_layer(h, k, w, b); }
int y355_bntrain_get_layer(y355_bntrain *h, int32_t k, float *w, float *b) { return core_get_layer(h, k, w, b); }
int y355_bntrain_get_grad(y355_bntrain *h, int32_t k, float *dw, float *db) { return core_get_grad(h, k, dw, db); }
int y355_bntrain_get_momentum(y355_bntrain *h, int32_t k, float *mw, float *mb) { return core_get_momentum(h, k, mw, mb); }
int y355_bntrain_get_packed(y355_bntrain *h, int32_t k, uint16_t *w_bf16) { return core_get_packed(h, k, w_bf16); }
int y355_bntrain_pred(y355_bntrain *h, void **out) { return core_pred(h, out); }
int y355_bntrain_wgrad_plan(const y355_bntrain *h, int32_t k, int32_t batch, int32_t *out) { return core_wgrad_plan(h, k, batch, out); }
int y355_bntrain_tensor_shape(const y355_bntrain *h, int32_t kind, int32_t t, int32_t *shape) { return core_tensor_shape(h, kind, t, shape, bn_tensor); }
int y355_bntrain_get_tensor(y355_bntrain *h, int32_t kind, int32_t t, void *out) { return core_get_tensor(h, kind, t, out, bn_tensor); }
int y355_bntrain_sgd_step(y355_bntrain *h, float lr, float momentum, float weight_decay, void *stream) {
    return core_sgd_step(h, lr, momentum, weight_decay, stream, [=](int first) {      // gamma and beta of every layer
        hipLaunchKernelGGL(bn_sgd_kernel, dim3((unsigned)((2 * h->cs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, 2 * h->cs, h->bnp, h->bng, h->bnm, lr,
                           momentum, weight_decay, first);
        return hipGetLastError();
    });
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

int y355_bntrain_forward(y355_bntrain *h, const void *x_dev, int32_t batch, void *stream) {
    if (int rc = forward_args(h, x_dev, batch)) return rc;
    if ((long long)batch * (h->H / 16) * (h->W / 16) < 2)
        return y355_fail(Y355_BNTRAIN_EINVAL, "y355_bntrain_forward: BatchNorm in training mode needs more than one value per channel: batch * H/16 * W/16 >= 2");
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_input(h, x_dev, batch, s));
    for (int k = 1; k < NL; ++k) {
        HIPCHK(launch_forward<M_Z>(h, k, batch, h->z[k], nullptr, s));
        if (int rc = bn_forward(h, k, batch, s)) return rc;
    }
    HIPCHK(launch_forward<M_PRED>(h, NL, batch, h->pred, nullptr, s));
    h->batch = batch;
    return Y355_BNTRAIN_OK;
}

int y355_bntrain_backward(y355_bntrain *h, const void *dpred_dev, void *stream) {
    if (int rc = backward_args(h, dpred_dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_dpred(h, dpred_dev, s));
    for (int k = NL; k >= 1; --k) {
        if (k <= NBN)
            if (int rc = bn_backward(h, k, s)) return rc;
        HIPCHK(launch_wgrad(h, k, s));
        if (k > 1) HIPCHK(launch_dgrad(h, k, h->dy[k - 1], s));       // the gradient with respect to the image is not computed
    }
    h->have_grad = true;
    return Y355_BNTRAIN_OK;
}

}  // extern "C"

