// yolo355 -- C ABI (include/yolo355.h): engine object, weight packing, layer schedule.
//
// Layer schedule = models/slim_yolo_v2.py:212-328 / c_embedding/yolo_forward.c:1202-1262:
//   conv1(3->16)+pool, conv2(16->32)+pool, conv3_1(32->64), conv3_2(64->64)+pool,
//   conv4_1(64->128), conv4_2(128->128)+pool, conv5(128->256), conv6, conv7, pred (no act).
#include "../../include/yolo355.h"
#include "y355_common.h"
#include "handle_core.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
static int fail(int code, const std::string &msg) { return y355_fail(code, msg); }
static_assert(Y355_RQ_ERANGE == Y355_ERANGE, "y355_requant.h refuses with Y355_ERANGE");

extern "C" const char *y355_last_error(void) { return g_err.c_str(); }
extern "C" int y355_version(void) { return 2; }       // 2: round 6 (y355_pipeline_*, y355_calibrate, y355_conv_op, *_dev operators)

// throughput mode: a layer's launch runs on Y355_OPT_RING_WORKGROUPS x pct / 100 workgroups (A/B builds: -DY355_GL_TAB="{..10 values..}")
#ifndef Y355_GL_TAB
#define Y355_GL_TAB {100, 100, 100, 100, 100, 100, 100, 100, 100, 100}
#endif
static const int kGridLimitPct[10] = Y355_GL_TAB;
#ifndef Y355_TPUT_PAIRS_WGS
#define Y355_TPUT_PAIRS_WGS 1       // workgroups per image of the NMS pair walk while several handles share the GPU (alone: 2)
#endif
namespace {
struct LayerDef { int cin, cout, pool, leaky, kid; };
const LayerDef kLayers[10] = {
    {3, 16, 1, 1, -1},
    {16, 32, 1, 1, Y355_K_CONV2},
    {32, 64, 0, 1, Y355_K_CONV3_1},
    {64, 64, 1, 1, Y355_K_CONV3_2},
    {64, 128, 0, 1, Y355_K_CONV4_1},
    {128, 128, 1, 1, Y355_K_CONV4_2},
    {128, 256, 0, 1, Y355_K_CONV5},
    {256, 256, 0, 1, Y355_K_CONV67},
    {256, 256, 0, 1, Y355_K_CONV67},
    {256, 0, 0, 0, Y355_K_PRED},
};
const int kRetuneDefault[10] = {11, 10, 10, 11, 11, 10, 11, 11, 11, 10};  // yolo_forward.c:35

struct Layer {
    int cin = 0, cout = 0, cout_pad = 0, pool = 0, leaky = 0, kid = -1;
    int Hin = 0, Win = 0, Hout = 0, Wout = 0, halo = 1;
    int e_w = 0, e_b = 0;
    bool loaded = false, bias_dirty = true;
    std::vector<int32_t> q_b;
    int8_t *w_dev = nullptr;
    int8_t *wpx_dev = nullptr;      // conv3_1 .. conv4_2: the same weights in convpx.hip's fragment order
    long long wabs = 0;             // max over output channels of sum |q_w| (0: not loaded): the tight bound of |acc| / 127
    int *bias_dev = nullptr;
    long long *bias_w_dev = nullptr;
    int8_t *out_dev = nullptr;
    size_t out_bytes = 0;
    Requant rq{};
    int frac_bits = 0;
};

int kernels_prepared = 0;
}  // namespace
int y355_prepare_kernels() {
    if (kernels_prepared) return 0;
    for (int i = 0; i < Y355_K_COUNT; ++i) {
        int e = y355_conv_kernel(i)->prepare();
        if (e) return fail(Y355_EHIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString((hipError_t)e));
    }
    if (int e = y355_prepare_head())
        return fail(Y355_EHIP, std::string("hipFuncSetAttribute(head): ") + hipGetErrorString((hipError_t)e));
    if (int e = y355_prepare_conv_ring())
        return fail(Y355_EHIP, std::string("hipFuncSetAttribute(ring): ") + hipGetErrorString((hipError_t)e));
    if (int e = y355_prepare_pair3())
        return fail(Y355_EHIP, std::string("hipFuncSetAttribute(pair3): ") + hipGetErrorString((hipError_t)e));
    if (int e = y355_prepare_conv_px())
        return fail(Y355_EHIP, std::string("hipFuncSetAttribute(px): ") + hipGetErrorString((hipError_t)e));
    if (int e = y355_prepare_convg())
        return fail(Y355_EHIP, std::string("hipFuncSetAttribute(convg): ") + hipGetErrorString((hipError_t)e));
    kernels_prepared = 1;
    return 0;
}
// compute units of the current device: the grid of the one-workgroup-per-CU launches (not the literal 256, so that a
// partitioned or smaller part does not serialise 157 KiB-of-LDS workgroups in waves)
int y355_cu_count(void) {
    static int cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}
struct y355_engine {
    y355_config cfg{};              // anchors and classes; the rest of it lives in the core
    HandleCore core;
    Layer L[10];
    int sa[11];
    bool sa_set[11];
    int retune[10];
    float trk_scale[11] = {};       // AveragedRangeTracker.scale / first_a of the 11 trackers (models/slim_yolo_v2.py:13-14), y355_calibrate
    int trk_first[11] = {};
    const uint8_t *x_u8 = nullptr;  // uint8 frames of the forward being enqueued (y355_forward_u8)
    int8_t *w0_dev = nullptr;       // conv1 fragment
    int8_t *wf_dev = nullptr;       // weight fragments of the fused front end (y355_pack_front)
    int8_t *sink_dev = nullptr;
    unsigned long long *stamps_dev = nullptr;
    int Hs = 0, Ws = 0;
    float *x_stage = nullptr;       // host-call staging
    int stamp_layer = -1;
    int fuse_front = 1;             // conv1 + pool1 + conv2 + pool2 as one launch (front.hip) where eligible
    int fuse_pairs = 1;             // conv3_1 -> conv3_2 + pool3 as one launch (pxpair.hip) where eligible
    int l2_batch = 0;               // images of conv3_1's map that the last launches left valid in L[2].out_dev (the fused pair writes none)
    int l0_batch = 0;               // images of conv1's pooled map that the last launches left valid in L[0].out_dev (the fused
                                    // front end keeps that map on chip: 0 after a fused forward)
    int ring_wgs = 0;               // persistent workgroups per ring launch (0 = one per CU)
    // kernel start / stop timestamps of the launches themselves (profile mode 2): 0..9 layers (the fused front end in slot 0),
    // 10 decode, 11 candidate sort, 12 pair walk, 13 rounds + output
    hipEvent_t kev[Y355_NUM_KERNEL_TIMERS][2] = {};       // (null: not created)
    bool kev_set[Y355_NUM_KERNEL_TIMERS] = {};
};

extern "C" void y355_destroy(y355_engine *h) {
    if (!h) return;
    y355_core_close(&h->core);
    for (auto &e : h->kev)
        for (hipEvent_t k : e)
            if (k) (void)hipEventDestroy(k);
    delete h;
}

extern "C" int y355_create(const y355_config *cfg, y355_engine **out) {
    if (!cfg || !out) return fail(Y355_EINVAL, "null argument");
    const int predc = cfg->num_anchors * (5 + cfg->num_classes);
    const int Hs = cfg->height / 16, Ws = cfg->width / 16, N = Hs * Ws * cfg->num_anchors;
    if (int rc = y355_core_check_config(cfg->height, cfg->width, 16, cfg->num_anchors, Y355_MAX_ANCHORS, cfg->num_classes, cfg->max_batch, N))
        return rc;
    HIPCHK(hipSetDevice(cfg->device_id));
    if (int e = y355_prepare_kernels()) return e;
    y355_engine *h = new y355_engine();
    h->cfg = *cfg;
    h->Hs = Hs;
    h->Ws = Ws;
    for (int i = 0; i < 11; ++i) { h->sa[i] = 0; h->sa_set[i] = false; }
    for (int i = 0; i < 10; ++i) h->retune[i] = kRetuneDefault[i];
    const int B = cfg->max_batch;
    int Hc = cfg->height, Wc = cfg->width;
    int rc = y355_core_open(&h->core, cfg->device_id, cfg->stream, cfg->own_stream != 0, Hc, Wc, B, N, cfg->conf_thresh, cfg->nms_thresh,
                            y355_hip_mem());
    for (int k = 0; k < 10 && !rc; ++k) {
        Layer &L = h->L[k];
        const LayerDef &d = kLayers[k];
        L.cin = d.cin;
        L.cout = d.cout ? d.cout : predc;
        L.pool = d.pool;
        L.leaky = d.leaky;
        L.kid = d.kid;
        L.Hin = Hc;
        L.Win = Wc;
        L.Hout = d.pool ? Hc / 2 : Hc;
        L.Wout = d.pool ? Wc / 2 : Wc;
        L.halo = (k == 9) ? 0 : 1;
        if (k == 0) L.cout_pad = 16;
        else {
            const int bn = y355_conv_kernel(L.kid)->bn;
            L.cout_pad = (L.cout + bn - 1) / bn * bn;
        }
        // slack rows so that clamped / masked tile reads of the next layer stay inside
        L.out_bytes = ((size_t)B * (L.Hout + 2 * L.halo) * (L.Wout + 2 * L.halo) + 64) * L.cout_pad;
        rc = y355_core_alloc(&h->core, &L.out_dev, L.out_bytes, true);
        if (!rc) rc = y355_core_alloc(&h->core, &L.bias_dev, sizeof(int) * L.cout_pad, true);
        if (!rc) rc = y355_core_alloc(&h->core, &L.bias_w_dev, sizeof(long long) * L.cout_pad, true);
        if (!rc && k > 0) rc = y355_core_alloc(&h->core, &L.w_dev, y355_packed_bytes(*y355_conv_kernel(L.kid), L.cout_pad), true);
        Hc = L.Hout;
        Wc = L.Wout;
    }
    if (!rc) rc = y355_core_alloc(&h->core, &h->w0_dev, 1024, true);
    if (!rc) rc = y355_core_alloc(&h->core, &h->wf_dev, 16384, true);
    if (!rc) rc = y355_core_alloc(&h->core, &h->sink_dev, 16384, true);
    if (!rc) rc = y355_core_state(&h->core, 10, cfg->max_det, true);
    if (!rc) rc = y355_core_events(&h->core, Y355_NUM_TIMERS);
    for (auto &e : h->kev)
        for (hipEvent_t &k : e)
            if (!rc && hipEventCreate(&k) != hipSuccess) rc = fail(Y355_EHIP, "hipEventCreate failed");
    if (rc) return y355_core_unwind(rc, [h] { y355_destroy(h); });
    *out = h;
    return 0;
}

extern "C" int y355_set_option(y355_engine *h, int option, int value) {
    if (!h) return fail(Y355_EINVAL, "null engine");
    switch (option) {
    case Y355_OPT_FUSE_FRONT:
        if (value != 0 && value != 1) return fail(Y355_EINVAL, "Y355_OPT_FUSE_FRONT takes 0 or 1");
        h->fuse_front = value;
        return 0;
    case Y355_OPT_FUSE_PAIRS:
        if (value != 0 && value != 1) return fail(Y355_EINVAL, "Y355_OPT_FUSE_PAIRS takes 0 or 1");
        h->fuse_pairs = value;
        return 0;
    case Y355_OPT_RING_WORKGROUPS:
        if (value < 0 || value > 4096) return fail(Y355_EINVAL, "workgroups per launch out of range");
        h->ring_wgs = value;
        return 0;
    case Y355_OPT_MAX_CANDIDATES:
    case Y355_OPT_HEAD_ROUTE: {
        const bool is_cap = option == Y355_OPT_MAX_CANDIDATES;
        return y355_core_head_option(&h->core, is_cap, value,
                                     is_cap ? "Y355_OPT_MAX_CANDIDATES: 4096 .. min(anchors per image, 65536)"
                                            : "Y355_OPT_HEAD_ROUTE takes 0 (auto) or 1 (large)");
    }
    default: return fail(Y355_EINVAL, "unknown option");
    }
}

// heads with more than 4096 anchors per image, or with the large route forced: *overflow = 1 if, in a forward since the last call,
// more anchors of an image passed conf_thresh than the candidate capacity holds (the excess was dropped); synchronous; clears the flag
extern "C" int y355_overflow(y355_engine *h, int *overflow) {
    return (!h || !overflow) ? fail(Y355_EINVAL, "null argument") : y355_core_overflow(&h->core, overflow);
}
// pipeline.hip: the flags of the forwards enqueued so far move to dst_dev [max_batch] on the handle's stream and are cleared
// behind the copy, so a ticket carries the overflow of its own forward (only for handles that have the flags)
bool y355_has_overflow_flags(y355_engine *h) { return h->core.head.wk.ovf != nullptr; }
int y355_overflow_take(y355_engine *h, int *dst_dev) {
    HIPCHK(y355_head_overflow_take(h->core.head, dst_dev, h->core.stream));
    return 0;
}
extern "C" int y355_max_candidates(y355_engine *h) { return h ? y355_head_capacity(h->core.head) : Y355_EINVAL; }

extern "C" int y355_set_thresholds(y355_engine *h, float conf, float nms) {
    return !h ? fail(Y355_EINVAL, "null engine") : y355_core_set_thresholds(&h->core, conf, nms);
}

extern "C" int y355_load_layer(y355_engine *h, int idx, const int8_t *q_w, const int32_t *q_b, int cout, int cin,
                               int e_w, int e_b) {
    if (!h || !q_w || !q_b) return fail(Y355_EINVAL, "null argument");
    if (idx < 0 || idx >= 10) return fail(Y355_EINVAL, "layer index out of range");
    Layer &L = h->L[idx];
    if (cout != L.cout || cin != L.cin) {
        char buf[128];
        snprintf(buf, sizeof buf, "layer %d expects [%d,%d,3,3], got [%d,%d,3,3]", idx, L.cout, L.cin, cout, cin);
        return fail(Y355_EINVAL, buf);
    }
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(hipStreamSynchronize(h->core.stream));
    if (idx == 0) {
        int8_t frag[1024];
        y355_pack_conv1(q_w, frag);
        HIPCHK(hipMemcpy(h->w0_dev, frag, 1024, hipMemcpyHostToDevice));
        std::vector<int8_t> ff(16384);
        y355_pack_front(q_w, nullptr, ff.data());
        HIPCHK(hipMemcpy(h->wf_dev, ff.data(), 4096, hipMemcpyHostToDevice));
    } else {
        const ConvKernelInfo &ki = *y355_conv_kernel(L.kid);
        std::vector<int8_t> packed(y355_packed_bytes(ki, L.cout_pad));
        y355_pack_weights(ki, q_w, cout, cin, L.cout_pad, packed.data());
        HIPCHK(hipMemcpy(L.w_dev, packed.data(), packed.size(), hipMemcpyHostToDevice));
        if (idx == 1) {
            std::vector<int8_t> ff(16384);
            y355_pack_front(nullptr, q_w, ff.data());
            HIPCHK(hipMemcpy(h->wf_dev + 4096, ff.data() + 4096, 12288, hipMemcpyHostToDevice));
        }
    }
    {
        long long best = 0;
        const size_t per = (size_t)cin * 9;
        for (int c = 0; c < cout; ++c) {
            long long sum = 0;
            for (size_t i = 0; i < per; ++i) sum += std::abs((int)q_w[(size_t)c * per + i]);
            best = std::max(best, sum);
        }
        L.wabs = best;
    }
    if (const size_t pxb = idx > 0 ? y355_px_packed_bytes(L.kid) : 0) {
        std::vector<int8_t> px(pxb);
        if (y355_pack_px(L.kid, q_w, cout, cin, px.data())) {
            if (!L.wpx_dev) {
                if (int rc = y355_core_alloc(&h->core, &L.wpx_dev, px.size(), false)) return rc;
            }
            HIPCHK(hipMemcpy(L.wpx_dev, px.data(), px.size(), hipMemcpyHostToDevice));
        }
    }
    L.q_b.assign(q_b, q_b + cout);
    L.e_w = e_w;
    L.e_b = e_b;
    L.loaded = true;
    L.bias_dirty = true;
    return 0;
}

// only what changes makes a layer's epilogue stale (callers set the same frozen exponents before every forward: that must
// not cost ten bias uploads and stream synchronisations per call)
static int set_one_exponent(y355_engine *h, int i, int v) {
    if (h->sa_set[i] && h->sa[i] == v) return 0;
    h->sa[i] = v;
    h->sa_set[i] = true;
    if (i < 10) h->L[i].bias_dirty = true;
    if (i > 0) h->L[i - 1].bias_dirty = true;
    return 0;
}

extern "C" int y355_set_act_exponents(y355_engine *h, const int32_t *sa) {
    if (!h || !sa) return fail(Y355_EINVAL, "null argument");
    for (int i = 0; i < 11; ++i)
        if (sa[i] < -64 || sa[i] > 64) return fail(Y355_EINVAL, "activation exponent out of range");
    for (int i = 0; i < 11; ++i) set_one_exponent(h, i, sa[i]);
    return 0;
}

extern "C" int y355_set_act_exponent(y355_engine *h, int i, int v) {
    if (!h || i < 0 || i > 10 || v < -64 || v > 64) return fail(Y355_EINVAL, "bad exponent");
    return set_one_exponent(h, i, v);
}

extern "C" int y355_get_act_exponents(y355_engine *h, int32_t *sa) {
    if (!h || !sa) return fail(Y355_EINVAL, "null argument");
    for (int i = 0; i < 11; ++i) sa[i] = h->sa[i];
    return 0;
}

extern "C" int y355_set_retune(y355_engine *h, const int32_t *r) {
    if (!h || !r) return fail(Y355_EINVAL, "null argument");
    for (int i = 0; i < 10; ++i) {
        if (h->retune[i] == r[i]) continue;
        h->retune[i] = r[i];
        h->L[i].bias_dirty = true;
    }
    return 0;
}

// (re)derive the integer epilogue of layer k and upload its pre-shifted biases
static int refresh_layer(y355_engine *h, int k, bool need_out) {
    Layer &L = h->L[k];
    if (!L.loaded) return fail(Y355_ENOTREADY, "layer weights not loaded");
    if (!h->sa_set[k]) return fail(Y355_ENOTREADY, "input activation exponent not set (calibrate first)");
    if (need_out && !h->sa_set[k + 1]) return fail(Y355_ENOTREADY, "output activation exponent not set (calibrate first)");
    if (!L.bias_dirty) return 0;
    Y355RqLayer q;              // the tight bound of the layer's own weights (L.wabs) goes into tmax_log2 / negsafe alone
    if (int rc = y355_rq_fail(y355_rq_layer(L.cin, 9, h->sa[k], L.e_w, L.e_b, h->sa[k + 1], h->sa_set[k + 1], L.leaky, h->retune[k],
                                            L.q_b.data(), L.cout, L.cout_pad, L.wabs, &q)))
        return rc;
    L.rq = q.rq;
    L.frac_bits = q.frac_bits;
    HIPCHK(hipMemcpyAsync(L.bias_dev, q.bias_t.data(), sizeof(int) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipMemcpyAsync(L.bias_w_dev, q.bias_w.data(), sizeof(long long) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));   // q's vectors are stack-owned
    L.bias_dirty = !h->sa_set[k + 1];
    return 0;
}

static int refresh_layers(y355_engine *h) {        // what a forward needs: every layer, with its output exponent
    for (int k = 0; k < 10; ++k)
        if (int rc = refresh_layer(h, k, true)) return rc;
    return 0;
}

static int launch_layer(y355_engine *h, int k, int B, int mode, int guard, const float *x_dev) {
    Layer &L = h->L[k];
    if (k == 0) {
        Conv1Params p{};
        p.x = x_dev;
        p.x_u8 = x_dev ? nullptr : h->x_u8;
        for (int c = 0; c < 3; ++c) { p.nmean[c] = h->core.stage.norm.mean[c]; p.nstd[c] = h->core.stage.norm.sd[c]; }
        p.out = L.out_dev;
        p.w = h->w0_dev;
        p.bias_t = L.bias_dev;
        p.bias_w = L.bias_w_dev;
        p.ctr = h->core.ctr_dev;
        p.B = B;
        p.H = L.Hin;
        p.W = L.Win;
        y355_conv1_tiles(L.Hin, L.Win, &p.tiles_x, &p.tiles_y);
        p.in_scale = std::ldexp(1.0f, h->sa[0]);
        p.rq = L.rq;
        p.mode = mode;
        p.guard = guard;
        y355_launch_conv1(p, h->core.stream);
        if (mode == 0) h->l0_batch = B;
    } else {
        const ConvKernelInfo &ki = *y355_conv_kernel(L.kid);
        ConvParams p{};
        p.in = h->L[k - 1].out_dev;
        p.out = L.out_dev;
        p.w = L.w_dev;
        p.bias_t = L.bias_dev;
        p.bias_w = L.bias_w_dev;
        p.ctr = h->core.ctr_dev + k;
        p.sink = h->sink_dev;
        p.stamps = (h->stamp_layer == k) ? h->stamps_dev : nullptr;
        h->kev_set[k] = false;
        if (h->core.profile == 2 && mode == 0) { p.ev_start = h->kev[k][0]; p.ev_stop = h->kev[k][1]; }
        p.grid_limit = h->ring_wgs * kGridLimitPct[k] / 100;
        p.B = B;
        p.H = L.Hin;
        p.W = L.Win;
        p.cstride = L.cout_pad;
        p.out_halo = L.halo;
        p.tiles_x = (L.Win + ki.tw - 1) / ki.tw;
        p.tiles_y = (L.Hin + ki.th - 1) / ki.th;
        p.nblk = L.cout_pad / ki.bn;
        p.rq = L.rq;
        p.mode = mode;
        p.guard = guard;
        // one production kernel per layer, then ONE fallback family (conv3x3.hip: statistics mode, head-room guard, 64-bit
        // epilogue, any shape).  conv3_1 .. conv4_2: weights in registers, pixels as the B operand (convpx.hip); conv3_2 .. pred:
        // LDS-DMA rings (conv3x3_ring.hip); conv2 (only when the fused front end is off) and whatever those two refuse: conv3x3.hip.
        // (Round 4: the resident-weight family conv3x3_v2.hip is gone -- it only ever ran where the fused front end or convpx refused.)
#ifdef Y355_EXPERIMENTS
        static const int no_ring_mask = getenv("Y355_NO_RING_MASK") ? atoi(getenv("Y355_NO_RING_MASK")) : 0;
        static const int no_px_mask = getenv("Y355_NO_PX_MASK") ? atoi(getenv("Y355_NO_PX_MASK")) : 0;
#else
        constexpr int no_ring_mask = 0, no_px_mask = 0;
#endif
        if (k == 2 && mode == 0) h->l2_batch = B;
        if (L.wpx_dev && !((no_px_mask >> k) & 1)) {
            ConvParams q = p;
            q.w = L.wpx_dev;
            if (y355_launch_conv_px(L.kid, q, h->core.stream)) {
                HIPCHK(hipGetLastError());
                h->kev_set[k] = p.ev_start != nullptr;
                return 0;
            }
        }
        if (!((no_ring_mask >> k) & 1) && y355_launch_conv_ring(L.kid, p, h->core.stream)) {
            HIPCHK(hipGetLastError());
            h->kev_set[k] = p.ev_start != nullptr;
            return 0;
        }
        ki.launch(p, p.tiles_x * p.tiles_y * p.nblk * B, h->core.stream);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int y355_input_absmax(y355_engine *h, const float *x_dev, int batch, float *out_max) {
    if (!h || !x_dev || !out_max) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    HIPCHK(hipMemsetAsync(h->core.absmax_dev, 0, 16, h->core.stream));
    y355_launch_absmax(x_dev, (size_t)batch * 3 * h->core.H * h->core.W, h->core.absmax_dev, h->core.stream);
    return y355_core_absmax_read(&h->core, out_max);
}

extern "C" int y355_run_layer(y355_engine *h, int idx, int batch, int mode, const float *x_dev) {
    if (!h) return fail(Y355_EINVAL, "null engine");
    if (idx < 0 || idx >= 10 || (mode != 0 && mode != 1)) return fail(Y355_EINVAL, "bad layer / mode");
    if (int rc = y355_core_range(&h->core, batch)) return rc;
    if (idx == 0 && !x_dev) return fail(Y355_EINVAL, "layer 0 needs the network input");
    if (int rc = y355_core_enter(&h->core)) return rc;
    if (int rc = refresh_layer(h, idx, mode == 0)) return rc;
    HIPCHK(hipMemsetAsync(h->core.ctr_dev + idx, 0, sizeof(Counters), h->core.stream));
    return launch_layer(h, idx, batch, mode, 1, x_dev);
}

extern "C" int y355_layer_stats_get(y355_engine *h, int idx, y355_layer_stats *out) {
    if (!h || !out || idx < 0 || idx >= 10) return fail(Y355_EINVAL, "bad argument");
    if (int rc = y355_core_enter(&h->core)) return rc;
    Counters c;
    HIPCHK(hipMemcpyAsync(&c, h->core.ctr_dev + idx, sizeof c, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));
    out->absmax_t = (int64_t)c.absmax;
    out->frac_bits = h->L[idx].frac_bits;
    out->reserved = (int32_t)c.in_sat;
    out->saturated = (int64_t)c.sat + (idx == 0 ? c.in_sat : 0);
    out->guard = (int64_t)c.guard;
    return 0;
}

// ---- AveragedRangeTracker.quantize_activation's state machine (models/slim_yolo_v2.py:16-38) for the 11 trackers of the
// path, in the reference's float32 arithmetic:
//   _max = activation.abs().max(); scale = 127 / _max        -- Python int / tensor = Tensor.__rtruediv__ = reciprocal() * 127: TWO
//                                                               fp32 roundings, reproduced here
//   first call ever (first_a == 0, even when frozen, :25-27): first_a = 1, self.scale += scale
//   frozen (:28-29): unchanged;  else (:30-31) self.scale = self.scale * (1 - momentum) + scale * momentum, the Python doubles
//   1 - momentum and momentum each rounded to fp32 by the tensor-scalar ops
//   exponent = floor(log2(self.scale)) (:33), log2 in fp32
static int tracker_update(float *scale, int *first, int i, float max_abs, int freeze, double momentum, int *exp_out) {
    const float s = (1.0f / max_abs) * 127.0f;
    if (!*first) {
        *first = 1;
        *scale = *scale + s;
    } else if (!freeze) {
        const float keep = (float)(1.0 - momentum), mom = (float)momentum;
        *scale = *scale * keep + s * mom;
    }
    const int bad = y355_tracker_exponent(*scale, exp_out);
    if (bad == 1) {
        char buf[160];
        snprintf(buf, sizeof buf, "tracker %d: scale %g is not a positive finite number (max|activation| = %g)", i, (double)*scale, (double)max_abs);
        return fail(Y355_ERANGE, buf);
    }
    return bad ? fail(Y355_ERANGE, "tracker exponent out of range") : 0;
}

// the update of ONE tracker as a host utility (no GPU): the arithmetic y355_calibrate applies, testable against torch on the CPU
extern "C" int y355_tracker_step(float *scale, int32_t *first_a, float max_abs, int freeze, double momentum, int32_t *exponent) {
    if (!scale || !first_a || !exponent) return fail(Y355_EINVAL, "null argument");
    int first = *first_a ? 1 : 0, e = 0;
    const int rc = tracker_update(scale, &first, 0, max_abs, freeze, momentum, &e);
    *first_a = first;
    if (!rc) *exponent = e;
    return rc;
}

extern "C" int y355_set_trackers(y355_engine *h, const float *scale, const int32_t *first_a) {
    if (!h || !scale || !first_a) return fail(Y355_EINVAL, "null argument");
    y355_trackers_set(h->trk_scale, h->trk_first, 11, scale, first_a);
    return 0;
}

extern "C" int y355_get_trackers(y355_engine *h, float *scale, int32_t *first_a) {
    if (!h || !scale || !first_a) return fail(Y355_EINVAL, "null argument");
    y355_trackers_get(h->trk_scale, h->trk_first, 11, scale, first_a);
    return 0;
}

// One calibration step on a batch: what forward(x, quantization=True) does to the trackers (:212-328), layer by layer on the
// GPU -- every tracker sees max|activation| of its layer computed with the exponents just updated in front of it, and the
// layer then runs for real so that the next one reads the reference's fake-quantised map.  Leaves the engine's exponents set.
extern "C" int y355_calibrate(y355_engine *h, const float *x_dev, int batch, int freeze, double momentum, int32_t *sa_out,
                              float *max_out) {
    if (!h || !x_dev) return fail(Y355_EINVAL, "null argument");
    if (batch < 1 || batch > h->core.max_batch) return fail(Y355_EINVAL, "batch out of range");
    if (!(momentum >= 0.0 && momentum <= 1.0)) return fail(Y355_EINVAL, "momentum outside [0, 1]");
    float m = 0.f;
    if (int rc = y355_input_absmax(h, x_dev, batch, &m)) return rc;
    int e = 0;
    if (int rc = tracker_update(&h->trk_scale[0], &h->trk_first[0], 0, m, freeze, momentum, &e)) return rc;
    if (max_out) max_out[0] = m;
    if (sa_out) sa_out[0] = e;
    set_one_exponent(h, 0, e);
    for (int k = 0; k < 10; ++k) {
        const float *xp = k == 0 ? x_dev : nullptr;
        if (int rc = y355_run_layer(h, k, batch, 1, xp)) return rc;
        y355_layer_stats st;
        if (int rc = y355_layer_stats_get(h, k, &st)) return rc;
        // max|y| as the fp32 value the reference's activation.abs().max() returns: t' / 2^F' is exact in fp32 wherever the
        // reference's own fp32 convolution is
        const float ymax = (float)st.absmax_t * std::ldexp(1.0f, -st.frac_bits);
        if (int rc = tracker_update(&h->trk_scale[k + 1], &h->trk_first[k + 1], k + 1, ymax, freeze, momentum, &e)) return rc;
        if (max_out) max_out[k + 1] = ymax;
        if (sa_out) sa_out[k + 1] = e;
        set_one_exponent(h, k + 1, e);
        if (int rc = y355_run_layer(h, k, batch, 0, xp)) return rc;
    }
    return 0;
}

extern "C" int y355_get_feature(y355_engine *h, int idx, int batch, int8_t *dst) {
    if (!h || !dst || idx < 0 || idx >= 10) return fail(Y355_EINVAL, "bad argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    if (idx == 0 && batch > h->l0_batch)
        return fail(Y355_ENOTREADY, "conv1's map of the last forward was not written (fused front end): "
                                    "run with y355_set_option(h, Y355_OPT_FUSE_FRONT, 0) to tap it");
    if (idx == 2 && batch > h->l2_batch)
        return fail(Y355_ENOTREADY, "conv3_1's map of the last forward was not written (fused conv3_1 -> conv3_2 + pool): "
                                    "run with y355_set_option(h, Y355_OPT_FUSE_PAIRS, 0) to tap it");
    const Layer &L = h->L[idx];
    const int Hp = L.Hout + 2 * L.halo, Wp = L.Wout + 2 * L.halo, CS = L.cout_pad;
    std::vector<int8_t> tmp((size_t)batch * Hp * Wp * CS);
    HIPCHK(hipStreamSynchronize(h->core.stream));
    HIPCHK(hipMemcpy(tmp.data(), L.out_dev, tmp.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < L.cout; ++c)
            for (int y = 0; y < L.Hout; ++y)
                for (int x = 0; x < L.Wout; ++x)
                    dst[(((size_t)b * L.cout + c) * L.Hout + y) * L.Wout + x] =
                        tmp[(((size_t)b * Hp + y + L.halo) * Wp + x + L.halo) * CS + c];
    return 0;
}

static HeadParams head_params(y355_engine *h, int sa_pred, float *ob, float *os, int *oc, int *on, bool tap) {
    HeadParams p{};
    const Layer &L = h->L[9];
    p.nlev = 1;
    HeadLevel &lv = p.lev[0];
    lv.pred = L.out_dev;
    lv.pred_f = nullptr;
    lv.cstride = L.cout_pad;
    lv.Hs = h->Hs;
    lv.Ws = h->Ws;
    lv.stride = 16.0f;                       // models/slim_yolo_v2.py:52
    lv.dq = std::ldexp(1.0f, -sa_pred);
    for (int i = 0; i < 2 * h->cfg.num_anchors; ++i) lv.anchors[i] = h->cfg.anchors[i];
    p.A = h->cfg.num_anchors;
    p.C = h->cfg.num_classes;
    p.wh_mul = 16.0f;                        // anchors in grid units (:126)
    // int8 logits keep exp(tw) in a narrow range: the anchor is a good size class (measured: pairs 52 us
    // vs 80 us with area octaves on the benchmark batch)
    p.group_by_area = 0;
    p.Hb = h->Hs;
    p.Wb = h->Ws;
    // more than 4096 anchors: the candidates arrive thresholded and compacted, their position says nothing about the anchor, and
    // one bin per cell and anchor (N bins) would not fit the sort's 4096-entry tables -- area octaves do
    if (h->core.N > Y355_NMS_CAP) y355_head_area_bins(p, h->Hs, h->Ws);
    p.pairs_wgs = h->ring_wgs > 0 ? Y355_TPUT_PAIRS_WGS : 0;    // throughput mode (Y355_OPT_RING_WORKGROUPS set): the pair walk holds one CU per image
    y355_head_fill(p, h->core.head, h->core.conf_thresh, h->core.nms_thresh, h->core.H, h->core.W, ob, os, oc, on, tap);
    return p;
}

// conv1 + pool1 + conv2 + pool2 in one launch (front.hip); the 16-channel map never reaches HBM
static int launch_front(y355_engine *h, int B, const float *x_dev) {
    Layer &L0 = h->L[0], &L1 = h->L[1];
    FrontParams p{};
    p.x = x_dev;
    p.x_u8 = x_dev ? nullptr : h->x_u8;
    for (int c = 0; c < 3; ++c) { p.nmean[c] = h->core.stage.norm.mean[c]; p.nstd[c] = h->core.stage.norm.sd[c]; }
    p.out = L1.out_dev;
    p.wf = h->wf_dev;
    p.bias1 = L0.bias_dev;
    p.bias2 = L1.bias_dev;
    p.ctr = h->core.ctr_dev;
    p.zero_next = (unsigned long long *)h->core.ctrs.other_zeroed_by_front();
    p.zero_n = 10 * (int)(sizeof(Counters) / 8);
    p.B = B;
    p.H = L0.Hin;
    p.W = L0.Win;
    y355_front_tiles(L0.Hin, L0.Win, &p.tiles_x, &p.tiles_y);
    p.in_scale = std::ldexp(1.0f, h->sa[0]);
    p.rq1 = L0.rq;
    p.rq2 = L1.rq;
    p.stamps = (h->stamp_layer == 0) ? h->stamps_dev : nullptr;
    h->kev_set[0] = h->kev_set[1] = false;
    if (h->core.profile == 2) { p.ev_start = h->kev[0][0]; p.ev_stop = h->kev[0][1]; h->kev_set[0] = true; }
    y355_launch_front(p, h->core.stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// The per-forward reset of the saturation counters as an ordinary kernel launch instead of hipMemsetAsync (whose fill goes down
// the runtime's blit path).  Measured equal to the memset in the three-handle regime (299.7 k against 300.0 k img/s); under
// rocprofv3 the memset shows a 280 us gap in front of it, which is the profiler's own per-dispatch cost, not the runtime's.
__global__ void y355_zero_u64_kernel(unsigned long long *p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0ull;
}
int y355_zero_counters(Counters *c, int n, hipStream_t s) {
    hipLaunchKernelGGL(y355_zero_u64_kernel, dim3(1), dim3(64), 0, s, (unsigned long long *)c, n * (int)(sizeof(Counters) / 8));
    return (int)hipGetLastError();                   // a failed launch must not leave the previous forward's counts in place
}

// conv3_1 -> conv3_2 + pool3 as one launch (pxpair.hip): 1 = launched, 0 = not eligible (the caller runs the two layers), < 0 error
static int launch_pair3(y355_engine *h, int B) {
    Layer &A = h->L[2], &Bl = h->L[3];
    if (!A.wpx_dev || !Bl.wpx_dev || A.cin != 32 || A.cout_pad != 64 || Bl.cout_pad != 64 || !Bl.pool || A.pool) return 0;
#ifdef Y355_EXPERIMENTS
    static const bool no_pair = getenv("Y355_NO_PAIR3") != nullptr;
    if (no_pair) return 0;
#endif
    PairParams p{};
    p.in = h->L[1].out_dev;
    p.out = Bl.out_dev;
    p.w1 = A.wpx_dev;
    p.w2 = Bl.wpx_dev;
    p.bias1 = A.bias_dev;
    p.bias2 = Bl.bias_dev;
    p.ctr1 = h->core.ctr_dev + 2;
    p.ctr2 = h->core.ctr_dev + 3;
    p.rq1 = A.rq;
    p.rq2 = Bl.rq;
    p.B = B;
    p.H = A.Hin;
    p.W = A.Win;
    p.grid_limit = h->ring_wgs * kGridLimitPct[2] / 100;
    p.stamps = (h->stamp_layer == 2) ? h->stamps_dev : nullptr;
    h->kev_set[2] = h->kev_set[3] = false;
    if (h->core.profile == 2) { p.ev_start = h->kev[2][0]; p.ev_stop = h->kev[2][1]; }
    if (!y355_launch_pair3(p, h->core.stream)) return 0;
    HIPCHK(hipGetLastError());
    h->kev_set[2] = p.ev_start != nullptr;
    h->l2_batch = 0;
    return 1;
}

// enqueue one forward on `s` (refresh_layer must have run)
static int enqueue_forward(y355_engine *h, const float *x_dev, int batch, int flags, float *boxes_dev, float *scores_dev,
                           int32_t *cls_dev, int32_t *count_dev, bool prof) {
    if (int rc = y355_core_begin_counters(&h->core)) return rc;
    const int guard = (flags & Y355_F_GUARD) ? 1 : 0;
    // the fused front end covers the 32-bit epilogue without the head-room guard; conv2's packed weights must be the
    // resident-weight layout (one n-block of 32 channels), which they are for this network
    const bool fused = h->fuse_front && !guard && y355_front_eligible(h->L[0].rq, h->L[1].rq) && h->L[1].cout_pad == 32;
    bool pair3 = false;
    for (int k = 0; k < 10; ++k) {
        if (prof) HIPCHK(hipEventRecord(h->core.ev[k], h->core.stream));
        if (fused && k == 0) {
            h->l0_batch = 0;
            if (int rc = launch_front(h, batch, x_dev)) return rc;
            continue;
        }
        if (fused && k == 1) continue;                    // timer slot 1 reads ~0: slot 0 holds conv1 + conv2
        if (k == 2 && h->fuse_pairs && !guard) {          // conv3_1 -> conv3_2 + pool3 in one launch; slot 3 then reads ~0
            const int rc = launch_pair3(h, batch);
            if (rc < 0) return rc;
            pair3 = rc == 1;
            if (pair3) continue;
        }
        if (pair3 && k == 3) continue;
        if (int rc = launch_layer(h, k, batch, 0, guard, x_dev)) return rc;
    }
    if (prof) HIPCHK(hipEventRecord(h->core.ev[10], h->core.stream));
    const HeadParams hp = head_params(h, h->sa[10], boxes_dev, scores_dev, cls_dev, count_dev, (flags & Y355_F_TAP) != 0);
    const bool kprof = prof && h->core.profile == 2;
    for (int i = 10; i < Y355_NUM_KERNEL_TIMERS; ++i) h->kev_set[i] = kprof;
    y355_launch_head_nms(hp, batch, h->core.head, h->core.stream, prof ? h->core.ev[11] : nullptr, kprof ? &h->kev[10] : nullptr);
    HIPCHK(hipGetLastError());
    if (prof) HIPCHK(hipEventRecord(h->core.ev[12], h->core.stream));
    return 0;
}

extern "C" int y355_forward(y355_engine *h, const float *x_dev, int batch, int flags, float *boxes_dev,
                            float *scores_dev, int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !x_dev || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    if (int rc = refresh_layers(h)) return rc;
    const bool prof = h->core.profile != 0;
    // (rounds 2-5 carried a hipGraph replay of the step's launches behind -DY355_EXPERIMENTS: measured, no gain; removed with the
    // alternating counter sets, which a captured graph would freeze)
    return enqueue_forward(h, x_dev, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev, prof);
}

// the fp32 staging tensor [max_batch][3][H][W] of the host call and of the uint8 forwards that take the fp32 route
static int need_x_stage(y355_engine *h) {
    return h->x_stage ? 0 : y355_core_alloc(&h->core, &h->x_stage, sizeof(float) * 3 * h->core.H * h->core.W * h->core.max_batch, false);
}

// BaseTransform constants of the uint8 path, in the reference's BGR order (data/__init__.py:50)
extern "C" int y355_set_normalization(y355_engine *h, const float *mean_bgr, const float *std_bgr) {
    if (!h || !mean_bgr || !std_bgr) return fail(Y355_EINVAL, "null argument");
    return y355_stage_set_normalization(h->core.stage, mean_bgr, std_bgr);
}

// The step in front of the path: frames as cv2 delivers them, uint8 HWC BGR [B][H][W][3]
// already at the network size; BaseTransform + BGR->RGB + HWC->CHW (data/__init__.py:30-56, test.py:79)
// are fused into the first layer's load (4x fewer input bytes than the fp32 tensor).  Same outputs as
// y355_forward on the normalised tensor, bit for bit.
extern "C" int y355_forward_u8(y355_engine *h, const uint8_t *frames_dev, int batch, int flags, float *boxes_dev,
                               float *scores_dev, int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !frames_dev || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    if (int rc = refresh_layers(h)) return rc;
    const bool fused = !h->L[0].rq.wide && !(flags & Y355_F_GUARD);
    if (!fused) {
        // 64-bit epilogue / guard runs take the fp32 tensor: normalise into the staging buffer first
        if (int rc = need_x_stage(h)) return rc;
        y355_launch_normalize_u8(frames_dev, h->x_stage, batch, h->core.H, h->core.W, h->core.stage.norm.mean, h->core.stage.norm.sd, h->core.stream);
        HIPCHK(hipGetLastError());
        return enqueue_forward(h, h->x_stage, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev, h->core.profile != 0);
    }
    h->x_u8 = frames_dev;
    const int rc = enqueue_forward(h, nullptr, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev, h->core.profile != 0);
    h->x_u8 = nullptr;
    return rc;
}

// frames of any size: cv2.resize to the network size on the GPU, then y355_forward_u8.  frames_dev uint8 [B][src_h][src_w][3].
// `resized_out_dev` (optional, [B][H][W][3]) receives the resized frames (parity tap).
extern "C" int y355_forward_u8_resized(y355_engine *h, const uint8_t *frames_dev, int src_h, int src_w, int batch, int flags,
                                       float *boxes_dev, float *scores_dev, int32_t *cls_dev, int32_t *count_dev,
                                       uint8_t *resized_out_dev) {
    if (!h || !frames_dev) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch, src_h, src_w)) return rc;
    FrameStage &st = h->core.stage;
    if (int rc = y355_stage_need_frames(st)) return rc;
    if (int rc = y355_core_resize_u8(&h->core, frames_dev, src_h, src_w, batch, st.frames)) return rc;
    if (resized_out_dev)
        HIPCHK(hipMemcpyAsync(resized_out_dev, st.frames, (size_t)batch * st.H * st.W * 3, hipMemcpyDeviceToDevice, h->core.stream));
    if (!boxes_dev && !scores_dev && !cls_dev && !count_dev) return 0;      // resize only
    return y355_forward_u8(h, st.frames, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev);
}

// ---- frame lists: every frame with its own pointer, size and row pitch (the reference's callers: one image at a time, each
// of its own size).  All frames, those at the network size included, go through the ragged stage of resize.hip into
// the stage's frames buffer; the forward then is y355_forward_u8 on that buffer.  The stage builds its tables on the device
// (FrameStage::tabs, one set per frame) and takes the descriptors as kernel arguments: nothing is uploaded, nothing waits, and
// the same-size route's cached table stays what it was.

// everything of a list forward that can fail, in front of its first launch (and, for y355_pipeline_submit_frames, in front
// of the pipeline's own state): the list rules and the handle's readiness (weights, exponents) without a HIP call, then the
// epilogue tables of layers whose exponents changed and the stage's buffers.  What follows it are launches only.
int y355_frames_prepare(y355_engine *h, const y355_frame *frames, int batch) {
    if (int rc = y355_frames_check(frames, batch, h->core.max_batch)) return rc;
    for (int k = 0; k < 10; ++k) {
        if (!h->L[k].loaded) return fail(Y355_ENOTREADY, "layer weights not loaded");
        if (!h->sa_set[k] || !h->sa_set[k + 1]) return fail(Y355_ENOTREADY, "activation exponent not set (calibrate first)");
    }
    if (int rc = y355_core_enter(&h->core)) return rc;
    if (int rc = refresh_layers(h)) return rc;
    if (int rc = y355_stage_need_list(h->core.stage)) return rc;
    return y355_stage_need_frames(h->core.stage);
}

extern "C" int y355_forward_frames(y355_engine *h, const y355_frame *frames, int batch, int flags, float *boxes_dev,
                                   float *scores_dev, int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !frames || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_frames_prepare(h, frames, batch)) return rc;
    y355_launch_resize_frames(frames, batch, h->core.stage.frames, h->core.stage.tabs, h->core.H, h->core.W, h->core.stream);
    HIPCHK(hipGetLastError());
    return y355_forward_u8(h, h->core.stage.frames, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev);
}

// parity tap of the ragged stage: the list -> out_dev [batch][H][W][3] at the network size, on the engine's stream
extern "C" int y355_resize_frames(y355_engine *h, const y355_frame *frames, int batch, uint8_t *out_dev) {
    return (!h || !frames || !out_dev) ? fail(Y355_EINVAL, "null argument") : y355_core_resize_frames(&h->core, frames, batch, out_dev);
}

// the host calls' outputs (HeadState::o_*) of a forward just enqueued, to the caller's arrays; waits for the stream
static int outputs_to_host(y355_engine *h, int batch, float *boxes, float *scores, int32_t *cls, int32_t *count) {
    const HeadState &hd = h->core.head;
    const size_t md = hd.max_det;
    HIPCHK(hipMemcpyAsync(boxes, hd.o_box, sizeof(float) * 4 * md * batch, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipMemcpyAsync(scores, hd.o_score, sizeof(float) * md * batch, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipMemcpyAsync(cls, hd.o_cls, sizeof(int) * md * batch, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipMemcpyAsync(count, hd.o_count, sizeof(int) * batch, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));
    return 0;
}

extern "C" int y355_forward_host(y355_engine *h, const float *x_host, int batch, int flags, float *boxes,
                                 float *scores, int32_t *cls, int32_t *count) {
    if (!h || !x_host || !boxes || !scores || !cls || !count) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    if (int rc = need_x_stage(h)) return rc;
    HIPCHK(hipMemcpyAsync(h->x_stage, x_host, sizeof(float) * 3 * h->core.H * h->core.W * batch, hipMemcpyHostToDevice, h->core.stream));
    if (int rc = y355_forward(h, h->x_stage, batch, flags, h->core.head.o_box, h->core.head.o_score, h->core.head.o_cls, h->core.head.o_count)) return rc;
    return outputs_to_host(h, batch, boxes, scores, cls, count);
}

extern "C" int y355_forward_counters(y355_engine *h, int64_t *saturated, int64_t *guard) {
    return !h ? fail(Y355_EINVAL, "null engine") : y355_core_counters(&h->core, saturated, guard);      // (the guard counts too)
}

extern "C" int y355_get_candidates(y355_engine *h, int batch, float *boxes, float *scores, int32_t *cls) {
    if (!h || !boxes || !scores || !cls) return fail(Y355_EINVAL, "null argument");
    return y355_core_get_candidates(&h->core, batch, boxes, scores, cls);
}

extern "C" int y355_head_nms(y355_engine *h, const int8_t *pred_q, int batch, int sa_pred, float *boxes,
                             float *scores, int32_t *cls, int32_t *count) {
    if (!h || !pred_q || !boxes || !scores || !cls || !count) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    const Layer &L = h->L[9];
    const int CS = L.cout_pad, Hs = h->Hs, Ws = h->Ws, PC = L.cout;
    std::vector<int8_t> tmp((size_t)batch * Hs * Ws * CS, 0);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < PC; ++c)
            for (int y = 0; y < Hs; ++y)
                for (int x = 0; x < Ws; ++x)
                    tmp[(((size_t)b * Hs + y) * Ws + x) * CS + c] = pred_q[(((size_t)b * PC + c) * Hs + y) * Ws + x];
    HIPCHK(hipStreamSynchronize(h->core.stream));
    HIPCHK(hipMemcpy(L.out_dev, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    const HeadState &hd = h->core.head;
    y355_launch_head_nms(head_params(h, sa_pred, hd.o_box, hd.o_score, hd.o_cls, hd.o_count, true), batch, hd, h->core.stream, nullptr);
    HIPCHK(hipGetLastError());
    return outputs_to_host(h, batch, boxes, scores, cls, count);
}

extern "C" int y355_max_det(y355_engine *h) { return h ? h->core.head.max_det : Y355_EINVAL; }
extern "C" int y355_num_anchors_total(y355_engine *h) { return h ? h->core.N : Y355_EINVAL; }

// Evaluator-side step right after the path: `bboxes *= [[w, h, w, h]]` of every image
// (test.py:88-90, utils/vocapi_evaluator_mask.py:71-72, utils/cocoapi_evaluator.py:77-85) for a whole batch on
// the GPU, on the engine's stream, in place.  The reference's float32 *= int64 computes the product in float64
// and rounds once to float32; box (24-bit) x size (< 2^24) is exact in float64, so one fp32 multiply is identical.
__global__ void scale_boxes_kernel(float *boxes, const int32_t *count, const float *wh, int max_det) {
    const int b = blockIdx.y;
    const int n = count[b];
    const float w = wh[2 * b], h = wh[2 * b + 1];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 *p = (float4 *)(boxes + ((size_t)b * max_det + i) * 4);
        float4 v = *p;
        v.x *= w; v.y *= h; v.z *= w; v.w *= h;
        *p = v;
    }
}
// (also y355_net_scale_boxes)
void y355_launch_scale_boxes(float *boxes, const int32_t *count, const float *wh, int batch, int max_det, hipStream_t s) {
    hipLaunchKernelGGL(scale_boxes_kernel, dim3((max_det + 255) / 256, batch), dim3(256), 0, s, boxes, count, wh, max_det);
}
extern "C" int y355_scale_boxes(y355_engine *h, float *boxes_dev, const int32_t *count_dev, const float *wh_dev, int batch) {
    if (!h || !boxes_dev || !count_dev || !wh_dev) return fail(Y355_EINVAL, "null argument");
    return y355_core_scale_boxes(&h->core, boxes_dev, count_dev, wh_dev, batch);
}

extern "C" int y355_pack_front_weights(const int8_t *q_w1, const int8_t *q_w2, int8_t *dst) {
    if (!dst) return fail(Y355_EINVAL, "null argument");
    y355_pack_front(q_w1, q_w2, dst);
    return 0;
}

// diagnostic: record s_memtime stamps of the production conv kernel of `layer` (-1 = off)
extern "C" int y355_debug_stamps(y355_engine *h, int layer, unsigned long long *out_host, int nwg) {
    if (!h) return fail(Y355_EINVAL, "null engine");
    if (int rc = y355_core_enter(&h->core)) return rc;
    if (!h->stamps_dev) {
        if (int rc = y355_core_alloc(&h->core, &h->stamps_dev, 8 * 32 * Y355_STAMP_ROWS, true)) return rc;
    }
    if (out_host) {
        HIPCHK(hipStreamSynchronize(h->core.stream));
        HIPCHK(hipMemcpy(out_host, h->stamps_dev, 8 * 32 * (size_t)(nwg > Y355_STAMP_ROWS ? Y355_STAMP_ROWS : nwg), hipMemcpyDeviceToHost));
    }
    h->stamp_layer = layer;
    HIPCHK(hipMemset(h->stamps_dev, 0, 8 * 32 * Y355_STAMP_ROWS));
    return 0;
}

extern unsigned long long *y355_nms_stamps_dev;
// diagnostics: s_memtime stamps of the head / pairs / resolve kernels of the last run (Y355_NMS_STAMPS=1)
extern "C" int y355_debug_nms_stamps(unsigned long long *out_host) {
    if (!out_host || !y355_nms_stamps_dev) return fail(Y355_ENOTREADY, "set Y355_NMS_STAMPS=1 before the first forward");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_host, y355_nms_stamps_dev, 8 * 8 * 256 * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void *y355_stream(y355_engine *h) { return h ? (void *)h->core.stream : nullptr; }

extern "C" int y355_sync(y355_engine *h) {
    return !h ? fail(Y355_EINVAL, "null engine") : y355_core_sync(&h->core);
}

extern "C" int y355_profile(y355_engine *h, int enable) {
    if (!h) return fail(Y355_EINVAL, "null engine");
    h->core.profile = enable;
    return 0;
}

extern "C" int y355_profile_get(y355_engine *h, float *ms) {
    return (!h || !ms) ? fail(Y355_EINVAL, "null argument") : y355_core_profile_get(&h->core, Y355_NUM_TIMERS, ms);
}

// ms [n]: the first n kernel timers of the last forward (0 where the launch recorded none)
static int kernel_timers(y355_engine *h, int n, float *ms) {
    if (!h || !ms) return fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(hipEventSynchronize(h->core.ev[12]));
    for (int k = 0; k < n; ++k) {
        ms[k] = 0.f;
        if (h->kev_set[k]) HIPCHK(hipEventElapsedTime(&ms[k], h->kev[k][0], h->kev[k][1]));
    }
    return 0;
}
extern "C" int y355_profile_kernel_get(y355_engine *h, float *ms) { return kernel_timers(h, 10, ms); }
extern "C" int y355_profile_kernels_get(y355_engine *h, float *ms) { return kernel_timers(h, Y355_NUM_KERNEL_TIMERS, ms); }
