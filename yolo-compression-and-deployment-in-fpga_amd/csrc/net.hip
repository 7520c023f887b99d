// yolo355 -- table-driven network executor behind the y355_net_* C ABI (include/yolo355.h):
//   Y355_ARCH_SLIM_V2  models/slim_yolo_v2.py:386-422, forward :549-622  (SlimYOLOv2, the fp32 model)
//   Y355_ARCH_TINY_V3  models/tiny_yolo_v3.py:9-273 + backbone/darknet.py:211-255 (YOLOv3tiny)
//   Y355_ARCH_YOLO_V2, _YOLO_V3, _YOLO_V3_SPP  models/yolo_v2.py, yolo_v3.py, yolo_v3_spp.py (DarkNet-19 / DarkNet-53)
// in two arithmetic types: bf16 (BN-folded fp32 weights, bf16 MFMA, fp32 accumulate) and int8
// (per-tensor power-of-two quantisation, the recipe of retune_bias_quantize.py:73-119 applied
// to these graphs).  The op tables are net_arch.h; every conv is convg.hip; the ops between the convs are the small
// kernels of netops.hip.
#include "../../include/yolo355.h"
#include "y355_common.h"
#include "handle_core.h"
#include "net_arch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Tensor {
    int C = 0, Cpad = 0, H = 0, W = 0, halo = 1, pred = 0;
    size_t pb = 0;          // bytes per pixel
    char *dev = nullptr;
    size_t bytes = 0;
};
struct NLayer {
    int cin = 0, cout = 0, cout_pad = 0, ksize = 3, kid = -1, op = -1;
    bool loaded = false;
    char *w_dev = nullptr;
    float *bias_dev = nullptr;
    size_t w_bytes = 0;
    // int8 nets
    std::vector<int32_t> q_b;
    int e_w = 0, e_b = 0;     // e_w: the largest of e_wc
    // weight exponent and sum |q_w| of every output channel (y355_net_load_layer_i8_pc; one value repeated by the per-tensor
    // load), pc: they differ.  shl_dev [cout_pad]: shl[c] = F - sa_in - e_wc[c] for the 64-bit epilogues and conv1.hip
    std::vector<int> e_wc;
    std::vector<long long> wabs_c;
    bool pc = false;
    int *shl_dev = nullptr;
    int route = 0;            // y355_net_layer_route: the kernel the last forward ran this layer on
    long long *bias_w_dev = nullptr;
    RequantG rq{};
    ResQ rr{};                // residual layers (OpDef::res1)
    Requant rq1{};            // first layer (conv1.hip epilogue)
    bool dirty = true;
    // 3x3 layers that have a ring instantiation (convr.hip): its id and the weights in its fragment order
    int rid = -1;
    char *wr_dev = nullptr;
    size_t wr_bytes = 0;
    // bf16 thin 3x3 layers with the weights in registers (convpxb.hip): its id and the weights in its fragment order
    int pbid = -1;
    char *wpb_dev = nullptr;
};
NetMap map_of(const Tensor &t) { return NetMap{t.dev, t.H, t.W, (int)t.pb}; }
}  // namespace

#ifndef Y355_USE_CONVPXB
#define Y355_USE_CONVPXB 1          // 0 (A/B builds): no convpxb.hip instantiation is ever selected
#endif
#ifndef Y355_USE_CONVR
#define Y355_USE_CONVR 1            // 0 (A/B builds): every layer of the generic nets on convg.hip
#endif
struct y355_net {
    y355_net_config cfg{};            // arch, anchors and classes; the rest of it lives in the core
    HandleCore core;
    const ArchDef *arch = nullptr;
    bool bf = true;
    int es = 2;
    std::vector<Tensor> T;
    std::vector<NLayer> L;
    char *w0_dev = nullptr;           // first-layer fragments
    int predc = 0;
    // int8 nets: activation exponents (value = q / 2^sa) of the input and of every tensor
    int sa_in = 0;
    bool sa_ok = false;
    std::vector<int> sa;
    // int8 nets whose graph starts with conv(3 -> 16) + pool, conv(16 -> 32) + pool (SlimYOLOv2, YOLOv3tiny:
    // models/slim_yolo_v2.py:549-575, backbone/darknet.py:216-220): both layers in ONE launch of the q_bf engine's fused front
    // end (front.hip) when their epilogues are exact in fp32 (y355_front_eligible); tap forwards run the layers one by one
    bool front_graph = false, front_ok = false, front_dirty = true;
    bool t0_skipped = false;                            // the last forward ran the fused front end: tensor 0 (conv1's map) was not written
    int8_t *wf_dev = nullptr;         // 16 KiB of front-end weight fragments (y355_pack_front)
    int *fb1_dev = nullptr, *fb2_dev = nullptr;   // pre-shifted int32 biases of the two layers
    Requant frq1{}, frq2{};
    int no_pxb = 0;                   // Y355_NET_OPT_THIN_RESIDENT = 0: the thin 3x3 layers of the bf16 graphs on convr.hip instead of convpxb.hip
    int tput_wgs = 0;                 // Y355_NET_OPT_WORKGROUPS: persistent workgroups per convr launch while several handles share the GPU (0 = one per CU)
    // calibration on the int8 graph (y355_net_calibrate): AveragedRangeTracker state of the network input [0] and of every
    // tensor [1 + t] (models/slim_yolo_v2.py:13-14), and one slot of maxima per op ([nops]: the input) on the device
    std::vector<float> trk_scale;
    std::vector<int> trk_first;
    Counters *cal_dev = nullptr;
};

// the network input of one forward: an fp32 NCHW tensor, or uint8 HWC BGR frames (u8) of src_h x src_w with the resize tables
// (tab, null when the frames are at the network size).  stage: frames [B][sh][sw][3] the forward first resizes into u8 (the
// net-owned buffer) with tab, inside the first op's profile interval.  list: a frame list (host array [batch]) the forward
// first resizes into u8 (the net-owned buffer, then frames at the network size: tab null) in the same place
struct NetInput {
    const float *x = nullptr;
    const uint8_t *u8 = nullptr;
    const int *tab = nullptr;
    int sh = 0, sw = 0;
    const uint8_t *stage = nullptr;
    const y355_frame *list = nullptr;
};

static int in_kbytes(const y355_net *h, const OpDef &o);

extern "C" void y355_net_destroy(y355_net *h) {
    if (!h) return;
    y355_core_close(&h->core);
    delete h;
}

extern "C" int y355_net_create(const y355_net_config *cfg, y355_net **out) {
    if (!cfg || !out) return y355_fail(Y355_EINVAL, "null argument");
    if (cfg->arch < 0 || cfg->arch > Y355_ARCH_YOLO_V3_SPP) return y355_fail(Y355_EINVAL, "unknown arch");
    if (cfg->dtype != Y355_DT_BF16 && cfg->dtype != Y355_DT_INT8) return y355_fail(Y355_EINVAL, "unknown dtype");
    // SlimYOLOv2 has four 2x2 pools (stride 16: models/slim_yolo_v2.py:52); the other graphs reach stride 32
    const int mult = cfg->arch == Y355_ARCH_SLIM_V2 ? 16 : 32;
    const ArchDef &A = kArch[cfg->arch];
    const int predc = cfg->num_anchors * (5 + cfg->num_classes);
    int N = 0;
    for (int l = 0; l < A.nlev; ++l) N += (cfg->height / (int)A.stride[l]) * (cfg->width / (int)A.stride[l]) * cfg->num_anchors;
    // (the candidate sort of these heads bins by area octave or class on a grid of at most 16 x 16: 16 x 256 bins fit its
    // 4096-entry tables whatever the number of anchors; heads of more than 4096 anchors are thresholded and compacted first)
    if (int rc = y355_core_check_config(cfg->height, cfg->width, mult, cfg->num_anchors, Y355_HEAD_MAXA / A.nlev, cfg->num_classes,
                                        cfg->max_batch, N))
        return rc;
    HIPCHK(hipSetDevice(cfg->device_id));
    if (int e = y355_prepare_kernels()) return e;
    if (y355_prepare_convr(cfg->device_id)) return y355_fail(Y355_EHIP, "hipFuncSetAttribute(convr) / sink allocation failed");
    if (y355_prepare_convpxb()) return y355_fail(Y355_EHIP, "hipFuncSetAttribute(convpxb) failed");
    y355_net *h = new y355_net();
    h->cfg = *cfg;
    h->arch = &A;
    h->bf = cfg->dtype == Y355_DT_BF16;
    h->es = h->bf ? 2 : 1;
    h->predc = predc;
    h->sa.assign(A.ntensors, 0);
    const int B = cfg->max_batch;
    int rc = y355_core_open(&h->core, cfg->device_id, cfg->stream, cfg->own_stream != 0, cfg->height, cfg->width, B, N, cfg->conf_thresh,
                            cfg->nms_thresh, y355_hip_mem());
    h->T.resize(A.ntensors);
    for (int i = 0; i < A.ntensors && !rc; ++i) {
        Tensor &t = h->T[i];
        t.C = A.t[i].C ? A.t[i].C : predc;
        t.pred = A.t[i].pred;
        t.halo = t.pred ? 0 : 1;
        t.H = cfg->height / A.t[i].div;
        t.W = cfg->width / A.t[i].div;
        // a pixel is at least 32 bytes (the thin path of convg.hip)
        const int cq = h->bf ? 16 : 32;
        t.Cpad = t.pred ? y355_pred_channels(t.C) : (t.C + cq - 1) / cq * cq;
        t.pb = (size_t)t.Cpad * ((t.pred && h->bf) ? 4 : h->es);
        t.bytes = ((size_t)B * (t.H + 2 * t.halo) * (t.W + 2 * t.halo) + 64) * t.pb;
        rc = y355_core_alloc(&h->core, &t.dev, t.bytes, true);
    }
    h->L.resize(A.nlayers);
    for (int i = 0; i < A.nops && !rc; ++i) {
        const OpDef &o = A.ops[i];
        // the int8 bilinear x2 has one kernel, sixteen channels per thread: every such op of the graph must meet its conditions
        if (o.type == OP_UPSAMPLE && !h->bf && !y355_upsample_i8_ok(map_of(h->T[o.in]), map_of(h->T[o.out]), B, o.cin, o.choff))
            rc = y355_fail(Y355_EINVAL, "no int8 upsampling kernel for an op of this graph at this size");
        if (o.type != OP_CONV1 && o.type != OP_CONV) continue;
        NLayer &L = h->L[o.layer];
        L.op = i;
        L.cin = o.cin;
        L.cout = o.cout ? o.cout : predc;
        L.ksize = o.ksize;
        if (o.type == OP_CONV1) {
            L.cout_pad = 16;
            rc = y355_core_alloc(&h->core, &h->w0_dev, 2048, true);
        } else {
            const Tensor &ti = h->T[o.in];
            L.kid = y355_convg_select(in_kbytes(h, o), L.cout, o.pool, ti.H, ti.W, o.stride2 ? 2 : 1, h->core.max_batch);
            if (L.kid < 0) { rc = y355_fail(Y355_EINVAL, "no convolution kernel for a layer of this graph"); break; }
            const ConvGInfo &ki = *y355_convg_kernel(h->bf, L.kid);
            if (in_kbytes(h, o) % ki.chb) { rc = y355_fail(Y355_EINVAL, "input channels not a multiple of the kernel's chunk"); break; }
            L.cout_pad = (L.cout + ki.bn - 1) / ki.bn * ki.bn;
            if (!h->T[o.out].pred && o.choff + L.cout_pad > h->T[o.out].Cpad) { rc = y355_fail(Y355_EINVAL, "layer wider than its output buffer"); break; }
            if (h->T[o.out].pred && L.cout_pad > h->T[o.out].Cpad) {
                rc = y355_fail(Y355_EINVAL, "prediction map wider than its buffer");
                break;
            }
            L.w_bytes = y355_convg_packed_bytes(ki, in_kbytes(h, o), o.ksize * o.ksize, L.cout_pad);
            rc = y355_core_alloc(&h->core, &L.w_dev, L.w_bytes, true);
            // (the pointwise launcher derives its k-steps from the input buffer's pixel pitch and has no pool: only an op that
            // consumes the WHOLE buffer, unpooled, may take it -- ADVICE r3)
            if (!rc && !h->bf && o.ksize == 1 && !o.stride2 && !o.res1 && !o.pool && ti.pb == in_kbytes(h, o) && L.cout_pad % 64 == 0 &&
                in_kbytes(h, o) % 64 == 0 && in_kbytes(h, o) <= 1024 && Y355_USE_CONVR) {                              // int8 1x1: pointwise kernel of convr.hip (when the epilogue fits 32 bits)
                L.rid = -2;
                L.wr_bytes = (size_t)(in_kbytes(h, o) / 64) * (L.cout_pad / 16) * 1024;
                rc = y355_core_alloc(&h->core, &L.wr_dev, L.wr_bytes, true);
            }
            if (!rc && h->bf && o.ksize == 3 && !o.stride2 && !o.res1 && !h->T[o.out].pred && Y355_USE_CONVPXB) {
                L.pbid = y355_convpxb_select(in_kbytes(h, o), L.cout, o.pool);
                if (L.pbid >= 0 && ((int)ti.pb != in_kbytes(h, o) || L.cout_pad != L.cout)) L.pbid = -1;     // whole-pixel inputs only
                if (L.pbid >= 0) rc = y355_core_alloc(&h->core, &L.wpb_dev, y355_convpxb_packed_bytes(L.pbid), true);
            }
            if (!rc && o.ksize == 3 && !o.stride2 && !o.res1 && Y355_USE_CONVR) {
                L.rid = y355_convr_select(h->bf ? 1 : 0, in_kbytes(h, o), L.cout_pad, o.pool, ti.H, ti.W);
                if (L.rid >= 0) {
                    L.wr_bytes = (size_t)(in_kbytes(h, o) / 64) * 9 * (L.cout_pad / 16) * 1024;
                    rc = y355_core_alloc(&h->core, &L.wr_dev, L.wr_bytes, true);
                }
            }
        }
        if (!rc) rc = y355_core_alloc(&h->core, &L.bias_dev, sizeof(float) * L.cout_pad, true);
        if (!rc) rc = y355_core_alloc(&h->core, &L.bias_w_dev, sizeof(long long) * L.cout_pad, true);
        if (!rc && !h->bf) rc = y355_core_alloc(&h->core, &L.shl_dev, sizeof(int) * L.cout_pad, true);
    }
    if (!rc && A.nops >= 2) {
        const OpDef &o0 = A.ops[0], &o1 = A.ops[1];
        bool fg = o0.type == OP_CONV1 && o0.cout == 16 && o0.pool == 1 && o1.type == OP_CONV && o1.in == o0.out && o1.cin == 16 &&
                  o1.cout == 32 && o1.ksize == 3 && o1.pool == 1 && !o1.stride2 && !o1.res1 && o1.choff == 0 &&
                  h->T[o1.out].pb == (size_t)(32 * h->es) && h->T[o1.out].halo == 1 && !h->T[o1.out].pred && cfg->height % 4 == 0 &&
                  cfg->width % 4 == 0;
        for (int i = 2; fg && i < A.nops; ++i)                     // nobody else reads conv1's map
            if (A.ops[i].in == o0.out || A.ops[i].res1 - 1 == o0.out) fg = false;
        if (fg) {
            h->front_graph = true;
            rc = y355_core_alloc(&h->core, &h->wf_dev, h->bf ? 32768 : 16384, true);      // y355_pack_frontb / y355_pack_front
            if (!rc && !h->bf) rc = y355_core_alloc(&h->core, &h->fb1_dev, sizeof(int) * 16, true);
            if (!rc && !h->bf) rc = y355_core_alloc(&h->core, &h->fb2_dev, sizeof(int) * 32, true);
        }
    }
    if (!rc && !h->bf) rc = y355_core_alloc(&h->core, &h->cal_dev, sizeof(Counters) * (A.nops + 1), true);
    h->trk_scale.assign(A.ntensors + 1, 0.f);
    h->trk_first.assign(A.ntensors + 1, 0);
    if (!rc) rc = y355_core_state(&h->core, A.nops + 1, cfg->max_det, false);
    if (!rc) rc = y355_core_events(&h->core, A.nops + 2);
    if (rc) return y355_core_unwind(rc, [h] { y355_net_destroy(h); });
    *out = h;
    return 0;
}

extern "C" int y355_net_set_option(y355_net *h, int option, int value) {
    if (!h) return y355_fail(Y355_EINVAL, "null net");
    if (option == Y355_NET_OPT_MAX_CANDIDATES || option == Y355_NET_OPT_HEAD_ROUTE) {
        const bool is_cap = option == Y355_NET_OPT_MAX_CANDIDATES;
        return y355_core_head_option(&h->core, is_cap, value,
                                     is_cap ? "Y355_NET_OPT_MAX_CANDIDATES: 4096 .. min(anchors per image, 65536)"
                                            : "Y355_NET_OPT_HEAD_ROUTE takes 0 (auto) or 1 (large)");
    }
    if (option == Y355_NET_OPT_WORKGROUPS) {
        if (value < 0 || value > 256) return y355_fail(Y355_EINVAL, "workgroups per launch: 0 .. 256");
        h->tput_wgs = value;
        return 0;
    }
    if (option == Y355_NET_OPT_THIN_RESIDENT) {
        if (value != 0 && value != 1) return y355_fail(Y355_EINVAL, "Y355_NET_OPT_THIN_RESIDENT takes 0 or 1");
        h->no_pxb = !value;
        return 0;
    }
    return y355_fail(Y355_EINVAL, "unknown option");
}

extern "C" int y355_net_set_thresholds(y355_net *h, float conf, float nms) {
    return !h ? y355_fail(Y355_EINVAL, "null net") : y355_core_set_thresholds(&h->core, conf, nms);
}

extern "C" int y355_net_num_layers(y355_net *h) { return h ? h->arch->nlayers : Y355_EINVAL; }
extern "C" int y355_net_num_tensors(y355_net *h) { return h ? h->arch->ntensors : Y355_EINVAL; }
extern "C" int y355_net_max_candidates(y355_net *h) { return h ? y355_head_capacity(h->core.head) : Y355_EINVAL; }
extern "C" int y355_net_max_det(y355_net *h) { return h ? h->core.head.max_det : Y355_EINVAL; }
extern "C" int y355_net_num_anchors_total(y355_net *h) { return h ? h->core.N : Y355_EINVAL; }

extern "C" int y355_net_layer_shape(y355_net *h, int idx, int32_t *shape) {
    if (!h || !shape || idx < 0 || idx >= h->arch->nlayers) return y355_fail(Y355_EINVAL, "bad argument");
    const NLayer &L = h->L[idx];
    shape[0] = L.cout; shape[1] = L.cin; shape[2] = L.ksize; shape[3] = L.ksize;
    return 0;
}

extern "C" int y355_net_tensor_shape(y355_net *h, int idx, int32_t *shape) {
    if (!h || !shape || idx < 0 || idx >= h->arch->ntensors) return y355_fail(Y355_EINVAL, "bad argument");
    const Tensor &t = h->T[idx];
    shape[0] = t.C; shape[1] = t.H; shape[2] = t.W;
    return 0;
}

extern "C" int y355_net_load_layer_f32(y355_net *h, int idx, const float *w, const float *b, int cout, int cin, int ksize) {
    if (!h || !w) return y355_fail(Y355_EINVAL, "null argument");
    if (idx < 0 || idx >= h->arch->nlayers) return y355_fail(Y355_EINVAL, "layer index out of range");
    if (!h->bf) return y355_fail(Y355_EINVAL, "fp32 weights go to a bf16 net");
    NLayer &L = h->L[idx];
    if (cout != L.cout || cin != L.cin || ksize != L.ksize) {
        char buf[160];
        snprintf(buf, sizeof buf, "layer %d expects [%d,%d,%d,%d], got [%d,%d,%d,%d]", idx, L.cout, L.cin, L.ksize, L.ksize,
                 cout, cin, ksize, ksize);
        return y355_fail(Y355_EINVAL, buf);
    }
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(hipStreamSynchronize(h->core.stream));
    const OpDef &o = h->arch->ops[L.op];
    if (o.type == OP_CONV1) {
        char frag[2048];
        y355_pack_conv1f(w, frag);
        HIPCHK(hipMemcpy(h->w0_dev, frag, 2048, hipMemcpyHostToDevice));
    } else {
        const ConvGInfo &ki = *y355_convg_kernel(1, L.kid);
        std::vector<char> packed(L.w_bytes);
        y355_convg_pack(ki, w, nullptr, cout, cin, ksize, in_kbytes(h, o), L.cout_pad, packed.data());
        HIPCHK(hipMemcpy(L.w_dev, packed.data(), packed.size(), hipMemcpyHostToDevice));
        if (L.rid >= 0) {                                      // the same fragments in the ring kernel's (bn, wn, nt) order
            const Y355ConvRInfo &ri = *y355_convr_info(L.rid);
            ConvGInfo kr{};
            kr.bf = 1; kr.chb = 64; kr.bn = ri.bn; kr.wn = ri.wn; kr.nt = ri.nt;
            std::vector<char> pr(L.wr_bytes);
            y355_convg_pack(kr, w, nullptr, cout, cin, ksize, in_kbytes(h, o), L.cout_pad, pr.data());
            HIPCHK(hipMemcpy(L.wr_dev, pr.data(), pr.size(), hipMemcpyHostToDevice));
        }
        if (L.pbid >= 0) {                                     // ... and in convpxb.hip's (weights stay in registers)
            std::vector<char> pb(y355_convpxb_packed_bytes(L.pbid));
            if (y355_convpxb_pack(L.pbid, w, cout, cin, pb.data())) HIPCHK(hipMemcpy(L.wpb_dev, pb.data(), pb.size(), hipMemcpyHostToDevice));
            else L.pbid = -1;
        }
    }
    if (h->front_graph && (L.op == 0 || L.op == 1)) {         // the same weights as the bf16 front end's fragments (frontb.hip)
        std::vector<char> wf(32768);
        y355_pack_frontb(L.op == 0 ? w : nullptr, L.op == 1 ? w : nullptr, wf.data());
        if (L.op == 0) HIPCHK(hipMemcpy(h->wf_dev, wf.data(), 8192, hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy(h->wf_dev + 8192, wf.data() + 8192, 32768 - 8192, hipMemcpyHostToDevice));
    }
    std::vector<float> bias(L.cout_pad, 0.f);
    if (b) memcpy(bias.data(), b, sizeof(float) * cout);
    HIPCHK(hipMemcpy(L.bias_dev, bias.data(), sizeof(float) * L.cout_pad, hipMemcpyHostToDevice));
    L.loaded = true;
    return 0;
}

// replaces load_state_dict of a checkpoint written by quantize_layers (retune_bias_quantize.py:111-119)
// for one conv of an int8 net: q_w int8 [cout][cin][k][k] (value q_w / 2^e_w), q_b int32 [cout]
// e_wc: one weight exponent per output channel, or null: e_w for all of them
static int load_layer_i8(y355_net *h, int idx, const int8_t *q_w, const int32_t *q_b, int cout, int cin, int ksize,
                         const int32_t *e_wc, int e_w, int e_b) {
    if (!h || !q_w || !q_b) return y355_fail(Y355_EINVAL, "null argument");
    if (idx < 0 || idx >= h->arch->nlayers) return y355_fail(Y355_EINVAL, "layer index out of range");
    if (h->bf) return y355_fail(Y355_EINVAL, "int8 weights go to an int8 net");
    NLayer &L = h->L[idx];
    if (cout != L.cout || cin != L.cin || ksize != L.ksize) {
        char buf[160];
        snprintf(buf, sizeof buf, "layer %d expects [%d,%d,%d,%d], got [%d,%d,%d,%d]", idx, L.cout, L.cin, L.ksize, L.ksize,
                 cout, cin, ksize, ksize);
        return y355_fail(Y355_EINVAL, buf);
    }
    for (int c = 0; e_wc && c < cout; ++c)                     // (cout is the layer's own by now)
        if (e_wc[c] < -128 || e_wc[c] > 128) return y355_fail(Y355_EINVAL, "weight exponent out of range");
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(hipStreamSynchronize(h->core.stream));
    const OpDef &o = h->arch->ops[L.op];
    if (o.type == OP_CONV1) {
        int8_t frag[1024];
        y355_pack_conv1(q_w, frag);
        HIPCHK(hipMemcpy(h->w0_dev, frag, 1024, hipMemcpyHostToDevice));
    } else {
        const ConvGInfo &ki = *y355_convg_kernel(0, L.kid);
        std::vector<char> packed(L.w_bytes);
        y355_convg_pack(ki, nullptr, q_w, cout, cin, ksize, in_kbytes(h, o), L.cout_pad, packed.data());
        HIPCHK(hipMemcpy(L.w_dev, packed.data(), packed.size(), hipMemcpyHostToDevice));
        if (L.rid >= 0 || L.rid == -2) {                       // the same fragments in the ring / pointwise kernel's (bn, wn, nt) order
            ConvGInfo kr{};
            kr.bf = 0; kr.chb = 64; kr.bn = 64; kr.wn = 1; kr.nt = 4;
            if (L.rid >= 0) {
                const Y355ConvRInfo &ri = *y355_convr_info(L.rid);
                kr.bn = ri.bn; kr.wn = ri.wn; kr.nt = ri.nt;
            }
            std::vector<char> pr(L.wr_bytes);
            y355_convg_pack(kr, nullptr, q_w, cout, cin, ksize, in_kbytes(h, o), L.cout_pad, pr.data());
            HIPCHK(hipMemcpy(L.wr_dev, pr.data(), pr.size(), hipMemcpyHostToDevice));
        }
    }
    if (h->front_graph && (L.op == 0 || L.op == 1)) {
        std::vector<int8_t> wf(16384);
        y355_pack_front(L.op == 0 ? q_w : nullptr, L.op == 1 ? q_w : nullptr, wf.data());
        if (L.op == 0) HIPCHK(hipMemcpy(h->wf_dev, wf.data(), 4096, hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy(h->wf_dev + 4096, wf.data() + 4096, 16384 - 4096, hipMemcpyHostToDevice));
        h->front_dirty = true;
    }
    L.q_b.assign(q_b, q_b + cout);
    L.e_wc.assign(cout, e_w);
    if (e_wc) L.e_wc.assign(e_wc, e_wc + cout);
    L.e_w = *std::max_element(L.e_wc.begin(), L.e_wc.end());
    L.pc = *std::min_element(L.e_wc.begin(), L.e_wc.end()) != L.e_w;
    L.e_b = e_b;
    {   // sum |q_w| of every output channel: the layer's own bound on |acc| (127 * wabs_c) for the 32-bit-epilogue test (all zero = unknown)
        const size_t per = (size_t)cin * ksize * ksize;
        L.wabs_c.assign(cout, 0);
        for (int c = 0; c < cout; ++c)
            for (size_t k = 0; k < per; ++k) L.wabs_c[c] += std::abs((int)q_w[(size_t)c * per + k]);
    }
    L.loaded = true;
    L.dirty = true;
    return 0;
}

extern "C" int y355_net_load_layer_i8(y355_net *h, int idx, const int8_t *q_w, const int32_t *q_b, int cout, int cin,
                                      int ksize, int e_w, int e_b) {
    return load_layer_i8(h, idx, q_w, q_b, cout, cin, ksize, nullptr, e_w, e_b);
}

// the same with one power-of-two weight scale per output channel (quantize_tensor(channel_level=True),
// retune_bias_quantize.py:73-86): value of a weight of channel c = q_w / 2^e_w[c]; the bias keeps one exponent
extern "C" int y355_net_load_layer_i8_pc(y355_net *h, int idx, const int8_t *q_w, const int32_t *q_b, int cout, int cin,
                                         int ksize, const int32_t *e_w, int e_b) {
    if (!e_w) return y355_fail(Y355_EINVAL, "null argument");
    return load_layer_i8(h, idx, q_w, q_b, cout, cin, ksize, e_w, 0, e_b);
}

static void act_fixed(int act, int *lk, int *neg_mul) {
    // LeakyReLU slope as neg_mul / 2^lk: 0.125 exactly; 0.1 ~ 205 / 2048 (build-defined)
    if (act == ACT_L125) { *lk = 3; *neg_mul = 1; }
    else if (act == ACT_L100) { *lk = 11; *neg_mul = 205; }
    else { *lk = 0; *neg_mul = 1; }
}

// y355_rq_fixed (y355_requant.h) of the convolution of op o: the exponent in front of it, the layer's exponents, biases and sums |q_w|
static Y355RqErr conv_fixed(const y355_net *h, const OpDef &o, const NLayer &L, Y355RqFixed *cf) {
    int lk, nm;
    act_fixed(o.act, &lk, &nm);
    return y355_rq_fixed(o.in < 0 ? h->sa_in : h->sa[o.in], L.e_wc.data(), L.wabs_c.data(), L.cout, L.e_b, L.q_b.data(), L.cout, L.cout_pad, lk, nm,
                         (long long)o.ksize * o.ksize * o.cin, Y355_RQ_SHL_MAX_NET, cf);
}

// the range proof of every loaded residual layer for the handle's exponents: the 64-bit sum u must provably fit
static int res_range_check(const y355_net *h) {
    for (int i = 0; i < h->arch->nops; ++i) {
        const OpDef &o = h->arch->ops[i];
        if (o.type != OP_CONV || !o.res1 || !h->L[o.layer].loaded) continue;
        Y355RqFixed cf;
        ResQ rr{};
        int narrow = 0;
        if (conv_fixed(h, o, h->L[o.layer], &cf).code || y355_rq_res(cf, h->sa[o.out], h->sa[o.res1 - 1], &rr, &narrow).code)
            return y355_fail(Y355_ERANGE, "residual layer: the 64-bit sum of the residual epilogue is not provably in range "
                                          "for these exponents");
    }
    return 0;
}

// activation exponents of an int8 net: sa_in for the fp32 network input, sa[t] for tensor t (graph
// order of net_arch.h).  A max-pool output takes its input's exponent and the network-input tensor sa_in (the entries
// given for them are overridden); a concat buffer (and the in-place SPP buffer) has ONE exponent that every producer
// requantises to.  Y355_ERANGE (nothing changed) when a loaded residual layer's epilogue is not provably in range.
// (arguments checked) installs the exponents with the aliasing and the range proof of y355_net_set_act_exponents
static int install_act_exponents(y355_net *h, int sa_in, const int32_t *sa, int n, bool all_set) {
    const int keep_in = h->sa_in;
    const std::vector<int> keep = h->sa;
    h->sa_in = sa_in;
    h->sa.assign(sa, sa + n);
    for (int i = 0; i < h->arch->nops; ++i) {
        const OpDef &o = h->arch->ops[i];
        if (o.type == OP_POOL) h->sa[o.out] = h->sa[o.in];      // max-pool does not requantise
        if (o.type == OP_INPUT) h->sa[o.out] = sa_in;            // the quantised network input
    }
    if (int rc = res_range_check(h)) {                           // (layers loaded later: checked again at the forward)
        h->sa_in = keep_in;
        h->sa = keep;
        return rc;
    }
    if (all_set) h->sa_ok = true;
    for (auto &L : h->L) L.dirty = true;
    return 0;
}

extern "C" int y355_net_set_act_exponents(y355_net *h, int sa_in, const int32_t *sa, int n) {
    if (!h || !sa) return y355_fail(Y355_EINVAL, "null argument");
    if (h->bf) return y355_fail(Y355_EINVAL, "bf16 nets have no activation exponents");
    if (n != h->arch->ntensors) return y355_fail(Y355_EINVAL, "one exponent per tensor expected");
    for (int i = 0; i < n; ++i)
        if (sa[i] < -64 || sa[i] > 64) return y355_fail(Y355_EINVAL, "activation exponent out of range");
    if (sa_in < -64 || sa_in > 64) return y355_fail(Y355_EINVAL, "activation exponent out of range");
    return install_act_exponents(h, sa_in, sa, n, true);
}

extern "C" int y355_net_layer_route(y355_net *h, int idx, int32_t *route) {
    if (!h || !route) return y355_fail(Y355_EINVAL, "null argument");
    if (idx < 0 || idx >= h->arch->nlayers) return y355_fail(Y355_EINVAL, "layer index out of range");
    *route = h->L[idx].route;
    return 0;
}

extern "C" int y355_net_get_act_exponents(y355_net *h, int32_t *sa_in, int32_t *sa, int n) {
    if (!h || !sa_in || !sa || n != h->arch->ntensors) return y355_fail(Y355_EINVAL, "bad argument");
    *sa_in = h->sa_in;
    for (int i = 0; i < n; ++i) sa[i] = h->sa[i];
    return 0;
}

// epilogue constants of the convolution of op i for the handle's current exponents (dirty layers only)
static int refresh_layer_i8(y355_net *h, int i) {
    const OpDef &o = h->arch->ops[i];
    if (o.type != OP_CONV1 && o.type != OP_CONV) return 0;
    NLayer &L = h->L[o.layer];
    if (!L.loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
    if (!L.dirty) return 0;
    Y355RqFixed cf;
    if (int rc = y355_rq_fail(conv_fixed(h, o, L, &cf))) return rc;
    if (int rc = y355_rq_fail(y355_rq_net(cf, h->sa[o.out], &L.rq))) return rc;
    const int sh = L.rq.sh;
    if (o.res1) {                  // residual: its own 64-bit bound, and its own 32-bit form (no split)
        int narrow = 0;
        if (int rc = y355_rq_fail(y355_rq_res(cf, h->sa[o.out], h->sa[o.res1 - 1], &L.rr, &narrow))) return rc;
        L.rq.narrow = narrow;
        L.rq.split = 0;
    }
    if (o.type == OP_CONV1) {
        // int8 nets have no float bias: the layer's bias_dev (4 bytes per channel) holds the 32-bit copy conv1.hip's fast kernel reads
        L.rq1 = y355_rq_first(cf, sh);
        const std::vector<int32_t> bt = L.rq1.gen32 ? y355_rq_bias32(cf) : std::vector<int32_t>(L.cout_pad, 0);
        HIPCHK(hipMemcpyAsync(L.bias_dev, bt.data(), sizeof(int32_t) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    }
    if (h->front_graph && (i == 0 || i == 1)) {                  // the same epilogue for front.hip
        Requant &fr = i == 0 ? h->frq1 : h->frq2;
        fr = y355_rq_front(cf, sh);
        std::vector<int32_t> fb = fr.wide ? std::vector<int32_t>() : y355_rq_bias32(cf);
        fb.resize(i == 0 ? 16 : 32, 0);
        HIPCHK(hipMemcpyAsync(i == 0 ? h->fb1_dev : h->fb2_dev, fb.data(), sizeof(int32_t) * fb.size(), hipMemcpyHostToDevice, h->core.stream));
        h->front_dirty = true;
    }
    // every output channel's own accumulator shift: in the upper half of the bias word for the 32-bit epilogues of
    // convg.hip / convr.hip (y355_pc_word; the bias fits 32 bits there), in shl_dev for the 64-bit ones and for conv1.hip
    if (o.type == OP_CONV && L.rq.narrow)
        for (int c = 0; c < L.cout; ++c) cf.bw[c] = y355_pc_word(cf.shc[c], (int)cf.bw[c]);
    HIPCHK(hipMemcpyAsync(L.shl_dev, cf.shc.data(), sizeof(int) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipMemcpyAsync(L.bias_w_dev, cf.bw.data(), sizeof(long long) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));
    L.dirty = false;
    return 0;
}

static int refresh_i8(y355_net *h) {
    if (h->bf) return 0;                                         // (bf16 nets have no epilogue constants)
    if (!h->sa_ok) return y355_fail(Y355_ENOTREADY, "activation exponents not set (calibrate first)");
    for (int i = 0; i < h->arch->nops; ++i)
        if (int rc = refresh_layer_i8(h, i)) return rc;
    if (h->front_graph && h->front_dirty) {
        // front.hip's epilogue has ONE accumulator shift per layer: a per-channel layer runs on conv1.hip / convg.hip instead
        const bool pc = h->L[h->arch->ops[0].layer].pc || h->L[h->arch->ops[1].layer].pc;
        h->front_ok = !pc && y355_front_eligible(h->frq1, h->frq2);
        h->front_dirty = false;
    }
    return 0;
}

// bytes of input channels a convolution consumes per pixel (its K extent): o.cin rounded up to the channel quantum --
// the whole pixel for ordinary tensors, a leading channel range for concat buffers read before they are complete
static int in_kbytes(const y355_net *h, const OpDef &o) {
    const int cq = h->bf ? 16 : 32;
    int c = (o.cin + cq - 1) / cq * cq;
    if (h->bf && c > 16) c = (c + 31) / 32 * 32;          // 64-byte k-steps beyond the thin (16-channel) path
    // int8 stride 2 has no thin form: 64-byte chunks (DarkNet-53's first down-sampling reads 32 real channels of a 64-channel
    // map, whose upper half its producer wrote as zeros)
    if (!h->bf && o.stride2) c = (c + 63) / 64 * 64;
    return c * h->es;
}

static float act_slope(int act) { return act == ACT_L125 ? 0.125f : act == ACT_L100 ? 0.1f : 1.0f; }

// the network-input fields the first-layer launch structs share (Conv1Params, Conv1FParams, FrontParams, FrontBParams);
// the u8 routes of these kernels get frames at the network size
template <class P>
static void fill_input(P &p, const y355_net *h, const NetInput &in, int B) {
    p.x = in.x;
    p.x_u8 = in.u8;
    for (int c = 0; c < 3; ++c) { p.nmean[c] = h->core.stage.norm.mean[c]; p.nstd[c] = h->core.stage.norm.sd[c]; }
    p.B = B;
    p.H = h->core.H;
    p.W = h->core.W;
}

// what a launch of run_op is for.  The two passes of a calibration step (y355_net_calibrate) run on the generic kernels:
// PASS_CAL_STAT takes a convolution's maximum |t'| with the constants of cal_conv_max and writes nothing (other ops: no such
// pass), PASS_CAL_WRITE writes the op's output as a forward does
enum Pass { PASS_FORWARD = 0, PASS_CAL_STAT, PASS_CAL_WRITE };

static int run_op(y355_net *h, int i, int B, const NetInput &in, Pass pass) {
    const OpDef &o = h->arch->ops[i];
    hipStream_t s = h->core.stream;
    const bool stat = pass == PASS_CAL_STAT, generic_only = pass != PASS_FORWARD;
    const bool bf = h->bf;
    if (o.type == OP_CONV1) {
        NLayer &L = h->L[o.layer];
        if (!L.loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
        if (!bf) {
            L.route = Y355_ROUTE_FIRST | (L.rq1.gen32 ? 0 : Y355_ROUTE_EPI64) | (L.pc ? Y355_ROUTE_PER_CHANNEL : 0);
            Conv1Params p{};
            fill_input(p, h, in, B);
            p.out = (int8_t *)h->T[o.out].dev;
            p.out_pb = (int)h->T[o.out].pb;
            p.w = (const int8_t *)h->w0_dev;
            p.bias_w = L.bias_w_dev;
            p.bias_t = L.rq1.gen32 ? (const int *)L.bias_dev : nullptr;          // (never in a statistics pass)
            p.shl_c = L.pc || stat ? L.shl_dev : nullptr;
            p.ctr = (stat ? h->cal_dev : h->core.ctr_dev) + i;
            y355_conv1_tiles(p.H, p.W, &p.tiles_x, &p.tiles_y);
            p.in_scale = std::ldexp(1.0f, h->sa_in);
            p.rq = L.rq1;
            p.mode = stat ? 1 : 0;                             // 1: max |t'| only
            y355_launch_conv1(p, s);
            HIPCHK(hipGetLastError());
            return 0;
        }
        Conv1FParams p{};
        fill_input(p, h, in, B);
        p.out = h->T[o.out].dev;
        p.w = h->w0_dev;
        p.bias = L.bias_dev;
        y355_conv1f_tiles(p.H, p.W, &p.tiles_x, &p.tiles_y);
        p.slope = act_slope(o.act);
        L.route = Y355_ROUTE_FIRST;
        y355_launch_conv1f(p, s);
    } else if (o.type == OP_CONV) {
        NLayer &L = h->L[o.layer];
        if (!L.loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
        const Tensor &ti = h->T[o.in], &to = h->T[o.out];
        const ConvGInfo &ki = *y355_convg_kernel(bf, L.kid);
        ConvGParams p{};
        p.in = ti.dev;
        p.out = to.dev;
        p.w = L.w_dev;
        p.bias_f = L.bias_dev;
        p.bias_w = L.bias_w_dev;
        p.shl_w = L.shl_dev;
        p.pc = L.pc ? 1 : 0;
        p.ctr = (stat ? h->cal_dev : h->core.ctr_dev) + i;
        p.rq = L.rq;
        const int rflags = bf ? 0 : ((L.rq.narrow ? 0 : Y355_ROUTE_EPI64) | (o.res1 ? Y355_ROUTE_RESIDUAL : 0) | (L.pc ? Y355_ROUTE_PER_CHANNEL : 0));
        p.B = B;
        p.H = ti.H;
        p.W = ti.W;
        p.in_pb = (int)ti.pb;
        p.nchunks = in_kbytes(h, o) / ki.chb;
        p.out_pb = (int)to.pb;
        p.out_off = o.choff * ((to.pred && bf) ? 4 : h->es);
        p.out_halo = to.halo;
        const int Ho = o.stride2 ? (ti.H + 1) / 2 : ti.H, Wo = o.stride2 ? (ti.W + 1) / 2 : ti.W;
        p.tiles_x = (Wo + ki.tw - 1) / ki.tw;
        p.tiles_y = (Ho + ki.th - 1) / ki.th;
        if (o.res1) {
            const Tensor &tr = h->T[o.res1 - 1];
            p.res = tr.dev;
            p.res_pb = (int)tr.pb;
            p.res_off = 0;
            p.rr = L.rr;
        }
        p.nblk = L.cout_pad / ki.bn;
        p.taps = o.ksize * o.ksize;
        p.slope = act_slope(o.act);
        p.out_f32 = to.pred && bf;
        p.grid_limit = h->tput_wgs;
        if (stat) {
            ki.launch_stat(p, p.tiles_x * p.tiles_y * p.nblk * B, s);
            HIPCHK(hipGetLastError());
            return 0;
        }
        if (L.rid == -2 && !generic_only) {                    // int8 1x1: pointwise kernel (convr.hip)
            ConvGParams q = p;
            q.w = L.wr_dev;
            q.nblk = L.cout_pad / 64;
            if (y355_launch_pw_i8(q, s)) {
                L.route = Y355_ROUTE_POINTWISE | rflags;
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        if (L.pbid >= 0 && !h->no_pxb) {                        // bf16 thin 3x3: weights in registers, pixels as the B operand (convpxb.hip)
            ConvGParams q = p;
            q.w = L.wpb_dev;
            if (y355_launch_convpxb(L.pbid, q, s)) {
                L.route = Y355_ROUTE_THIN;
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        if (L.rid >= 0 && !generic_only) {                     // 3x3: weights through an LDS ring (convr.hip)
            ConvGParams q = p;
            q.w = L.wr_dev;
            q.nblk = L.cout_pad / y355_convr_info(L.rid)->bn;
            if (y355_launch_convr(L.rid, q, h->core.device_id, s)) {
                L.route = Y355_ROUTE_RING | rflags;
                HIPCHK(hipGetLastError());
                return 0;
            }
        }
        L.route = (ki.wm * ki.wn == 8 ? Y355_ROUTE_GENERIC8 : Y355_ROUTE_GENERIC4) | rflags;
        ki.launch(p, p.tiles_x * p.tiles_y * p.nblk * B, s);
    } else if (o.type == OP_INPUT) {
        y355_launch_input(bf, in.x, in.u8, in.tab, in.sh, in.sw, h->core.stage.norm, map_of(h->T[o.out]), B, bf ? 1.0f : std::ldexp(1.0f, h->sa_in),
                          h->core.ctr_dev + i, s);
    } else if (o.type == OP_POOL) {
        y355_launch_pool(bf, map_of(h->T[o.in]), map_of(h->T[o.out]), B, o.cin * h->es, o.pool ? 1 : 2, s);
    } else if (o.type == OP_SPP) {
        y355_launch_spp(bf, map_of(h->T[o.in]), B, o.cin, s);
    } else if (o.type == OP_REORG) {
        y355_launch_reorg(bf, map_of(h->T[o.in]), map_of(h->T[o.out]), B, o.cin, o.choff * h->es, o.ksize,
                          bf ? 0 : h->sa[o.out] - h->sa[o.in], h->core.ctr_dev + i, s);
    } else {                                                   // OP_UPSAMPLE (int8: y355_net_create checked y355_upsample_i8_ok)
        y355_launch_upsample(bf, map_of(h->T[o.in]), map_of(h->T[o.out]), B, o.cin, o.choff * h->es,
                             bf ? 1.0f : std::ldexp(1.0f, h->sa[o.out] - h->sa[o.in]), s);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static HeadParams net_head_params(y355_net *h, float *ob, float *os, int *oc, int *on, bool tap) {
    HeadParams p{};
    const ArchDef &A = *h->arch;
    p.nlev = A.nlev;
    for (int l = 0; l < A.nlev; ++l) {
        const Tensor &t = h->T[A.pred_t[l]];
        HeadLevel &lv = p.lev[l];
        lv.pred = h->bf ? nullptr : (const int8_t *)t.dev;
        lv.pred_f = h->bf ? (const float *)t.dev : nullptr;
        lv.cstride = t.Cpad;
        lv.Hs = t.H;
        lv.Ws = t.W;
        lv.stride = A.stride[l];
        lv.dq = h->bf ? 1.0f : std::ldexp(1.0f, -h->sa[A.pred_t[l]]);
        for (int i = 0; i < 2 * h->cfg.num_anchors; ++i) lv.anchors[i] = h->cfg.anchors[l * 2 * h->cfg.num_anchors + i];
    }
    p.A = h->cfg.num_anchors;
    p.C = h->cfg.num_classes;
    // slim-YOLOv2 anchors are in grid units (models/slim_yolo_v2.py:126), tiny-v3's in pixels (tiny_yolo_v3.py:85)
    p.wh_mul = h->cfg.arch == Y355_ARCH_SLIM_V2 ? 16.0f : (h->cfg.arch == Y355_ARCH_YOLO_V2 ? 32.0f : 1.0f);
    // fp32 / multi-level heads: box sizes spread over many octaves per anchor -> group by area
    // (YOLOv3tiny int8, B = 128: NMS 1.08 -> 0.50 ms; SlimYOLOv2 bf16: 0.45 -> 0.32 ms)
    y355_head_area_bins(p, h->T[A.pred_t[0]].H, h->T[A.pred_t[0]].W);
    p.pairs_wgs = h->tput_wgs > 0 ? 1 : 0;        // throughput mode: the pair walk holds one CU per image
    y355_head_fill(p, h->core.head, h->core.conf_thresh, h->core.nms_thresh, h->core.H, h->core.W, ob, os, oc, on, tap);
    return p;
}

// the stage in front of the first op: frames of another size (in.stage), or a frame list (every frame through the ragged
// stage), resized into the net-owned buffer the first op reads
static int pre_stage(y355_net *h, const NetInput &in, int batch) {
    if (in.stage) y355_launch_resize_u8(in.stage, h->core.stage.frames, in.tab, batch, in.sh, in.sw, h->core.H, h->core.W, h->core.stream);
    if (in.list) y355_launch_resize_frames(in.list, batch, h->core.stage.frames, h->core.stage.tabs, h->core.H, h->core.W, h->core.stream);
    if (in.stage || in.list) HIPCHK(hipGetLastError());
    return 0;
}

// the forward behind y355_net_forward and y355_net_forward_u8 (arguments checked, device set, int8 exponents refreshed)
static int net_forward(y355_net *h, const NetInput &in, int batch, int flags, float *boxes_dev, float *scores_dev, int32_t *cls_dev,
                       int32_t *count_dev) {
    const bool prof = h->core.profile != 0;
    const int nops = h->arch->nops;
    if (!h->bf)
        if (int rc = y355_core_begin_counters(&h->core)) return rc;
    // tap forwards (parity tests read every tensor) run the first two layers one by one: the fused launch does not write conv1's map
    const bool fuse_front = h->front_graph && (h->bf || h->front_ok) && !(flags & Y355_F_TAP);
    h->t0_skipped = fuse_front;
    for (int i = 0; i < nops; ++i) {
        if (prof) HIPCHK(hipEventRecord(h->core.ev[i], h->core.stream));
        if (i == 0)                                     // (inside the first op's profile interval)
            if (int rc = pre_stage(h, in, batch)) return rc;
        if (fuse_front && i < 2) {
            if (i == 1) continue;
            const OpDef &o0 = h->arch->ops[0], &o1 = h->arch->ops[1];
            if (!h->L[o0.layer].loaded || !h->L[o1.layer].loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
            if (h->bf) {
                FrontBParams fb{};
                fill_input(fb, h, in, batch);
                fb.out = h->T[o1.out].dev;
                fb.out_pb = (int)h->T[o1.out].pb;
                fb.wf = (const char *)h->wf_dev;
                fb.bias1 = h->L[o0.layer].bias_dev;
                fb.bias2 = h->L[o1.layer].bias_dev;
                y355_frontb_tiles(fb.H, fb.W, &fb.tiles_x, &fb.tiles_y);
                fb.slope1 = act_slope(o0.act);
                fb.slope2 = act_slope(o1.act);
                y355_launch_frontb(fb, h->core.stream);
            } else {
                FrontParams fp{};
                fill_input(fp, h, in, batch);
                fp.out = (int8_t *)h->T[o1.out].dev;
                fp.wf = h->wf_dev;
                fp.bias1 = h->fb1_dev;
                fp.bias2 = h->fb2_dev;
                fp.ctr = h->core.ctr_dev;                                // [0] conv1 (+ input), [1] conv2: the two ops' own counters
                fp.zero_next = (unsigned long long *)h->core.ctrs.other_zeroed_by_front();
                fp.zero_n = (nops + 1) * (int)(sizeof(Counters) / 8);
                y355_front_tiles(fp.H, fp.W, &fp.tiles_x, &fp.tiles_y);
                fp.in_scale = std::ldexp(1.0f, h->sa_in);
                fp.rq1 = h->frq1;
                fp.rq2 = h->frq2;
                y355_launch_front(fp, h->core.stream);
            }
            h->L[o0.layer].route = h->L[o1.layer].route = Y355_ROUTE_FRONT;
            HIPCHK(hipGetLastError());
            continue;
        }
        if (int rc = run_op(h, i, batch, in, PASS_FORWARD)) return rc;
    }
    if (prof) HIPCHK(hipEventRecord(h->core.ev[nops], h->core.stream));
    const HeadParams hp = net_head_params(h, boxes_dev, scores_dev, cls_dev, count_dev, (flags & Y355_F_TAP) != 0);
    y355_launch_head_nms(hp, batch, h->core.head, h->core.stream, prof ? h->core.ev[nops + 1] : nullptr);
    HIPCHK(hipGetLastError());
    if (prof) HIPCHK(hipEventRecord(h->core.ev[nops + 2], h->core.stream));
    return 0;
}

extern "C" int y355_net_forward(y355_net *h, const float *x_dev, int batch, int flags, float *boxes_dev, float *scores_dev,
                                int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !x_dev || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch)) return rc;
    if (int rc = refresh_i8(h)) return rc;
    NetInput in;
    in.x = x_dev;
    return net_forward(h, in, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev);
}

// BaseTransform constants of the uint8 input, in the reference's BGR order (data/__init__.py:50), as y355_set_normalization
extern "C" int y355_net_set_normalization(y355_net *h, const float *mean_bgr, const float *std_bgr) {
    if (!h || !mean_bgr || !std_bgr) return y355_fail(Y355_EINVAL, "null argument");
    return y355_stage_set_normalization(h->core.stage, mean_bgr, std_bgr);
}

// Camera frames as cv2 delivers them, uint8 HWC BGR [B][src_h][src_w][3], as the network's first input: BaseTransform
// (data/__init__.py:30-56: resize, /255, -mean, /std), BGR->RGB and HWC->CHW (test.py:79-85) run inside the op that reads the
// network input -- the input op of the DarkNet graphs (with the resize fused into its load), the first layer or the fused front
// end of the slim / tiny graphs (behind the resize stage when the frames are not at the network size).  Same outputs, bit for
// bit, as y355_net_forward on the normalised tensor of the resized frames.
// align4: the fused front ends load a frame row in 12-byte pieces (4 pixels), dword-aligned only when the frames pointer is:
// slim / tiny frames at an address that is not a multiple of 4 then go through the resize stage (the identity at equal sizes)
// into the net-owned, aligned buffer.  The input op of the DarkNet graphs and the conv1 kernels (all a calibration step runs)
// read single bytes.
static int u8_input(y355_net *h, const uint8_t *frames_dev, int src_h, int src_w, bool align4, NetInput *in) {
    in->u8 = frames_dev;
    in->sh = src_h;
    in->sw = src_w;
    const bool fused = h->arch->ops[0].type == OP_INPUT;              // the input op resizes in its own load
    if (src_h == h->core.H && src_w == h->core.W && (fused || !align4 || ((uintptr_t)frames_dev & 3) == 0)) return 0;
    if (int rc = y355_stage_tables_for(h->core.stage, src_h, src_w, h->core.stream)) return rc;
    in->tab = h->core.stage.tab;
    if (!fused) {                                                   // staged: pre_stage resizes into the stage's frames first
        if (int rc = y355_stage_need_frames(h->core.stage)) return rc;
        in->stage = frames_dev;
        in->u8 = h->core.stage.frames;
    }
    return 0;
}

extern "C" int y355_net_forward_u8(y355_net *h, const uint8_t *frames_dev, int src_h, int src_w, int batch, int flags,
                                   float *boxes_dev, float *scores_dev, int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !frames_dev || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch, src_h, src_w)) return rc;
    if (int rc = refresh_i8(h)) return rc;
    NetInput in;
    if (int rc = u8_input(h, frames_dev, src_h, src_w, true, &in)) return rc;
    return net_forward(h, in, batch, flags, boxes_dev, scores_dev, cls_dev, count_dev);
}

// parity tap of the resize stage: frames [B][src_h][src_w][3] -> out_dev [B][H][W][3] at the network size, on the net's stream
extern "C" int y355_net_resize_u8(y355_net *h, const uint8_t *frames_dev, int src_h, int src_w, int batch, uint8_t *out_dev) {
    if (!h || !frames_dev || !out_dev) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = y355_core_enter(&h->core, batch, src_h, src_w)) return rc;
    return y355_core_resize_u8(&h->core, frames_dev, src_h, src_w, batch, out_dev);
}

// ---- frame lists: every frame with its own pointer, size and pitch (the reference's callers: one image at a time, each of
// its own size).  All frames, those at the network size included, go through the ragged stage of resize.hip into the stage's frames;
// the forward / calibration step then is the same-size uint8 path on that buffer (in.u8 = the frames, no table, no stage).
// The stage builds its tables on the device and takes the descriptors as kernel arguments: nothing is uploaded, nothing
// waits, whatever the sizes of the previous call were.
// the stage's buffers, allocated at the first list call of a handle
static int net_list_buffers(y355_net *h) {
    if (int rc = y355_stage_need_list(h->core.stage)) return rc;
    return y355_stage_need_frames(h->core.stage);
}

static NetInput list_input(const y355_net *h, const y355_frame *frames) {
    NetInput in;
    in.u8 = h->core.stage.frames;
    in.sh = h->core.H;
    in.sw = h->core.W;
    in.list = frames;
    return in;
}

extern "C" int y355_net_forward_frames(y355_net *h, const y355_frame *frames, int batch, int flags, float *boxes_dev,
                                       float *scores_dev, int32_t *cls_dev, int32_t *count_dev) {
    if (!h || !frames || !boxes_dev || !scores_dev || !cls_dev || !count_dev) return y355_fail(Y355_EINVAL, "null argument");
    if (int rc = y355_frames_check(frames, batch, h->core.max_batch)) return rc;
    if (int rc = y355_core_enter(&h->core)) return rc;
    if (int rc = refresh_i8(h)) return rc;
    if (int rc = net_list_buffers(h)) return rc;
    return net_forward(h, list_input(h, frames), batch, flags, boxes_dev, scores_dev, cls_dev, count_dev);
}

// parity tap of the ragged stage: the list -> out_dev [batch][H][W][3] at the network size, on the net's stream
extern "C" int y355_net_resize_frames(y355_net *h, const y355_frame *frames, int batch, uint8_t *out_dev) {
    return (!h || !frames || !out_dev) ? y355_fail(Y355_EINVAL, "null argument") : y355_core_resize_frames(&h->core, frames, batch, out_dev);
}

// the evaluators' `bboxes *= [[w, h, w, h]]` (test.py:88-90) on a forward's outputs, on the net's stream, in place (as
// y355_scale_boxes): boxes_dev [B][max_det][4], count_dev [B], wh_dev [B][2] (width, height)
extern "C" int y355_net_scale_boxes(y355_net *h, float *boxes_dev, const int32_t *count_dev, const float *wh_dev, int batch) {
    if (!h || !boxes_dev || !count_dev || !wh_dev) return y355_fail(Y355_EINVAL, "null argument");
    return y355_core_scale_boxes(&h->core, boxes_dev, count_dev, wh_dev, batch);
}

extern "C" int y355_net_get_candidates(y355_net *h, int batch, float *boxes, float *scores, int32_t *cls) {
    if (!h || !boxes || !scores || !cls) return y355_fail(Y355_EINVAL, "null argument");
    return y355_core_get_candidates(&h->core, batch, boxes, scores, cls);
}

// parity tap: tensor idx as fp32 NCHW [B][C][H][W] on the host (halo and channel padding stripped)
extern "C" int y355_net_get_tensor(y355_net *h, int idx, int batch, float *dst) {
    if (!h || !dst || idx < 0 || idx >= h->arch->ntensors) return y355_fail(Y355_EINVAL, "bad argument");
    if (int rc = y355_core_range(&h->core, batch)) return rc;
    if (idx == h->arch->ops[0].out && h->t0_skipped)
        return y355_fail(Y355_ENOTREADY, "the first layer's map of the last forward was not written (fused front end): "
                                         "run the forward with Y355_F_TAP to read it");
    if (int rc = y355_core_enter(&h->core)) return rc;
    const Tensor &t = h->T[idx];
    const int Hp = t.H + 2 * t.halo, Wp = t.W + 2 * t.halo;
    std::vector<char> tmp((size_t)batch * Hp * Wp * t.pb);
    HIPCHK(hipStreamSynchronize(h->core.stream));
    HIPCHK(hipMemcpy(tmp.data(), t.dev, tmp.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < t.C; ++c)
            for (int y = 0; y < t.H; ++y)
                for (int x = 0; x < t.W; ++x) {
                    const char *src = tmp.data() + (((size_t)b * Hp + y + t.halo) * Wp + x + t.halo) * t.pb;
                    float v;
                    if (!h->bf) {
                        v = std::ldexp((float)*(const signed char *)(src + c), -h->sa[idx]);
                    } else if (t.pred) {
                        memcpy(&v, src + (size_t)c * 4, 4);
                    } else {
                        unsigned short hbits;
                        memcpy(&hbits, src + (size_t)c * 2, 2);
                        const unsigned int u = (unsigned int)hbits << 16;
                        memcpy(&v, &u, 4);
                    }
                    dst[(((size_t)b * t.C + c) * t.H + y) * t.W + x] = v;
                }
    return 0;
}

// max |value| of tensor idx (calibration tap for the int8 recipe); synchronous
extern "C" int y355_net_tensor_absmax(y355_net *h, int idx, int batch, float *out_max) {
    if (!h || !out_max || idx < 0 || idx >= h->arch->ntensors) return y355_fail(Y355_EINVAL, "bad argument");
    if (int rc = y355_core_range(&h->core, batch)) return rc;
    const Tensor &t = h->T[idx];
    if (!h->bf) return y355_fail(Y355_EINVAL, "absmax taps exist on bf16 nets (the calibration run)");
    if (t.pred) return y355_fail(Y355_EINVAL, "prediction maps are fp32: read them with y355_net_get_tensor");
    if (idx == h->arch->ops[0].out && h->t0_skipped)
        return y355_fail(Y355_ENOTREADY, "the first layer's map of the last forward was not written (fused front end): "
                                         "calibrate from a forward with Y355_F_TAP");
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(hipMemsetAsync(h->core.absmax_dev, 0, 16, h->core.stream));
    const size_t n = (size_t)batch * (t.H + 2) * (t.W + 2) * t.Cpad;
    y355_launch_absmax_bf16(t.dev, n, h->core.absmax_dev, h->core.stream);
    return y355_core_absmax_read(&h->core, out_max);
}

// values clamped to +-127 in the last forward of an int8 net (input quantisation included); synchronous
extern "C" int y355_net_counters(y355_net *h, int64_t *saturated) {
    return (!h || !saturated) ? y355_fail(Y355_EINVAL, "null argument") : y355_core_counters(&h->core, saturated, nullptr);
}

// heads with more than 4096 anchors per image: 1 if, in any forward since the last call, more than 4096 anchors of an
// image passed conf_thresh (the excess was dropped); synchronous; clears the flags
extern "C" int y355_net_overflow(y355_net *h, int *overflow) {
    return (!h || !overflow) ? y355_fail(Y355_EINVAL, "null argument") : y355_core_overflow(&h->core, overflow);
}

// diagnostics: candidates and suppressing pairs per image of the last forward's NMS (count[batch], nedges[2 * batch]: list
// length, overflow / abort flag); synchronous
extern "C" int y355_net_debug_nms(y355_net *h, int batch, int32_t *count, int32_t *nedges) {
    if (!h || !count || !nedges || batch < 1 || batch > h->core.max_batch) return y355_fail(Y355_EINVAL, "bad argument");
    if (int rc = y355_core_enter(&h->core)) return rc;
    HIPCHK(y355_head_debug_counts(h->core.head, h->core.stream, batch, count, nedges));
    return 0;
}

extern "C" int y355_net_sync(y355_net *h) {
    return !h ? y355_fail(Y355_EINVAL, "null net") : y355_core_sync(&h->core);
}

extern "C" int y355_net_profile(y355_net *h, int enable) {
    if (!h) return y355_fail(Y355_EINVAL, "null net");
    h->core.profile = enable;
    return 0;
}

extern "C" int y355_net_num_timers(y355_net *h) { return h ? h->arch->nops + 2 : Y355_EINVAL; }

extern "C" int y355_net_profile_get(y355_net *h, float *ms) {
    return (!h || !ms) ? y355_fail(Y355_EINVAL, "null argument") : y355_core_profile_get(&h->core, h->arch->nops + 2, ms);
}

// ------------------------------------------------------------------------------------------
// Calibration on the int8 graph itself: the reference's forward(x, quantization=True) with freeze = not trainable
// (models/slim_yolo_v2.py:212-328, AveragedRangeTracker :9-38; the loop of retune_bias_quantize.py:357-369) as ONE pass over
// the op table.  Semantics: include/yolo355.h (y355_net_calibrate), DESIGN.md section 6.
extern "C" int y355_net_num_trackers(y355_net *h) { return h ? h->arch->ntensors + 1 : Y355_EINVAL; }

extern "C" int y355_net_get_trackers(y355_net *h, float *scale, int32_t *first_a, int n) {
    if (!h || !scale || !first_a) return y355_fail(Y355_EINVAL, "null argument");
    if (h->bf) return y355_fail(Y355_EINVAL, "bf16 nets have no trackers");
    if (n != h->arch->ntensors + 1) return y355_fail(Y355_EINVAL, "one tracker for the input and one per tensor expected");
    y355_trackers_get(h->trk_scale.data(), h->trk_first.data(), n, scale, first_a);
    return 0;
}

extern "C" int y355_net_set_trackers(y355_net *h, const float *scale, const int32_t *first_a, int n) {
    if (!h || !scale || !first_a) return y355_fail(Y355_EINVAL, "null argument");
    if (h->bf) return y355_fail(Y355_EINVAL, "bf16 nets have no trackers");
    if (n != h->arch->ntensors + 1) return y355_fail(Y355_EINVAL, "one tracker for the input and one per tensor expected");
    // exponents of the trackers that have seen a batch: floor(log2(scale)) (:33); the others keep the handle's
    int sa_in = h->sa_in;
    std::vector<int32_t> sa(h->sa.begin(), h->sa.end());
    bool all = true;
    for (int i = 0; i < n; ++i) {
        if (!first_a[i]) { all = false; continue; }
        int e = 0;
        if (const int bad = y355_tracker_exponent(scale[i], &e))
            return y355_fail(Y355_EINVAL, bad == 1 ? "tracker scale is not a positive finite number" : "tracker exponent out of range");
        if (i == 0) sa_in = e;
        else sa[i - 1] = e;
    }
    if (int rc = install_act_exponents(h, sa_in, sa.data(), n - 1, all)) return rc;
    y355_trackers_set(h->trk_scale.data(), h->trk_first.data(), n, scale, first_a);
    return 0;
}

// the statistics pass of the convolution of op i: its 64-bit epilogue up to t' (residual: up to the sum u) for the exponents in
// front of it, then max |.| as the fp32 value y355_calibrate forms from absmax_t / frac_bits (engine.hip).  The layer's
// constants (stale in a calibration step: net_calibrate_run) are the pass's afterwards; refresh_layer_i8 rebuilds them for the
// write pass.
static int cal_conv_max(y355_net *h, int i, int B, const NetInput &in, float *out_max) {
    const OpDef &o = h->arch->ops[i];
    NLayer &L = h->L[o.layer];
    if (!L.loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
    Y355RqFixed cf;
    if (int rc = y355_rq_fail(conv_fixed(h, o, L, &cf))) return rc;
    int fb = 0;                                                // exponent of the tracked integers
    if (int rc = y355_rq_fail(y355_rq_stat(cf, o.res1 != 0, o.res1 ? h->sa[o.res1 - 1] : 0, &L.rq, &L.rq1, &L.rr, &fb))) return rc;
    HIPCHK(hipMemcpyAsync(L.shl_dev, cf.shc.data(), sizeof(int) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipMemcpyAsync(L.bias_w_dev, cf.bw.data(), sizeof(long long) * L.cout_pad, hipMemcpyHostToDevice, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));                   // (the host vectors go out of scope)
    if (int rc = run_op(h, i, B, in, PASS_CAL_STAT)) return rc;
    unsigned long long m = 0;
    HIPCHK(hipMemcpyAsync(&m, &h->cal_dev[i].absmax, 8, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));
    *out_max = (float)(int64_t)m * std::ldexp(1.0f, -fb);
    return 0;
}

// the 32-bit maximum of slot i (fp32 bits or an unsigned int) back to the host
static int cal_read_u32(y355_net *h, int i, void *v) {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(v, &h->cal_dev[i].absmax, 4, hipMemcpyDeviceToHost, h->core.stream));
    HIPCHK(hipStreamSynchronize(h->core.stream));
    return 0;
}

static int net_calibrate_run(y355_net *h, const NetInput &in, int B, int freeze, double momentum, std::vector<float> &mx) {
    const ArchDef &A = *h->arch;
    const int nops = A.nops, nt = A.ntensors;
    hipStream_t s = h->core.stream;
    const std::vector<float> pre_scale = h->trk_scale;
    const std::vector<int> pre_first = h->trk_first;
    for (auto &L : h->L) L.dirty = true;                       // the step installs new exponents op by op: every layer's constants are stale
    HIPCHK(hipMemsetAsync(h->cal_dev, 0, sizeof(Counters) * (nops + 1), s));
    if (int rc = y355_core_begin_counters(&h->core)) return rc;         // the write passes count their clamps as a forward does
    h->t0_skipped = false;
    auto step = [&](int k, float m, int *e) -> int {           // tracker k sees m
        int32_t first = h->trk_first[k], ex = 0;
        if (int rc = y355_tracker_step(&h->trk_scale[k], &first, m, freeze, momentum, &ex)) return rc;
        h->trk_first[k] = first;
        mx[k] = m;
        *e = ex;
        return 0;
    };
    auto slot = [&](int i) { return (unsigned int *)&h->cal_dev[i].absmax; };
    // ---- tracker 0: max |x| of the fp32 input / of the normalised resized frames
    if (int rc = pre_stage(h, in, B)) return rc;
    if (in.x) {
        y355_launch_absmax(in.x, (size_t)B * 3 * h->core.H * h->core.W, slot(nops), s);
    } else {
        const bool staged = in.stage != nullptr || A.ops[0].type != OP_INPUT;      // in.u8 is at the network size
        y355_launch_absmax_u8(in.u8, staged ? nullptr : in.tab, B, in.sh, in.sw, h->core.H, h->core.W, h->core.stage.norm, slot(nops), s);
    }
    float m = 0.f;
    if (int rc = cal_read_u32(h, nops, &m)) return rc;
    int e = 0;
    if (int rc = step(0, m, &e)) return rc;
    h->sa_in = e;
    // ---- the op table in graph order; first[t]: the op that produced tensor t first, late[t]: a later producer was seen
    std::vector<int> first(nt, -1), late(nt, 0);
    NetInput run = in;
    run.stage = nullptr;                                       // (already resized)
    run.list = nullptr;
    for (int i = 0; i < nops; ++i) {
        const OpDef &o = A.ops[i];
        const bool inplace = o.type == OP_SPP;
        float mo = 0.f;
        if (o.type == OP_CONV1 || o.type == OP_CONV) {
            if (int rc = cal_conv_max(h, i, B, run, &mo)) return rc;
        } else if (o.type == OP_UPSAMPLE) {
            y355_launch_upsample_i8_max(map_of(h->T[o.in]), B, o.cin, slot(i), s);
            if (int rc = cal_read_u32(h, i, &mo)) return rc;
            mo *= std::ldexp(1.0f, -h->sa[o.in]);
        } else if (o.type == OP_REORG) {
            unsigned int q = 0;
            y355_launch_absmax_i8(map_of(h->T[o.in]), B, o.cin, slot(i), s);
            if (int rc = cal_read_u32(h, i, &q)) return rc;
            mo = (float)q * std::ldexp(1.0f, -h->sa[o.in]);
        }
        if (o.type == OP_INPUT || o.type == OP_POOL) {         // aliases: the entry mirrors its source's
            const int src = o.type == OP_INPUT ? 0 : o.in + 1;
            h->trk_scale[o.out + 1] = h->trk_scale[src];
            h->trk_first[o.out + 1] = h->trk_first[src];
            mx[o.out + 1] = mx[src];
            h->sa[o.out] = o.type == OP_INPUT ? h->sa_in : h->sa[o.in];
            first[o.out] = i;
        } else if (!inplace) {
            if (first[o.out] < 0) {                            // the tensor's first producer: its exponent for this step
                first[o.out] = i;
                if (int rc = step(o.out + 1, mo, &e)) return rc;
                h->sa[o.out] = e;
            } else {                                           // a later producer writes with that exponent
                late[o.out] = 1;
                mx[o.out + 1] = std::max(mx[o.out + 1], mo);
            }
        }
        if (int rc = refresh_layer_i8(h, i)) return rc;        // the write pass's constants
        if (int rc = run_op(h, i, B, run, PASS_CAL_WRITE)) return rc;
    }
    // ---- buffers with several producers: the update redone from the pre-step state with the maximum over all of them
    for (int t = 0; t < nt; ++t) {
        if (!late[t]) continue;
        h->trk_scale[t + 1] = pre_scale[t + 1];
        h->trk_first[t + 1] = pre_first[t + 1];
        if (int rc = step(t + 1, mx[t + 1], &e)) return rc;
        h->sa[t] = e;
    }
    for (int i = 0; i < nops; ++i) {
        const OpDef &o = A.ops[i];
        if (o.type != OP_POOL) continue;
        h->trk_scale[o.out + 1] = h->trk_scale[o.in + 1];
        h->trk_first[o.out + 1] = h->trk_first[o.in + 1];
        mx[o.out + 1] = mx[o.in + 1];
        h->sa[o.out] = h->sa[o.in];
    }
    // the exponents the handle keeps: the residual range proof of y355_net_set_act_exponents
    if (int rc = res_range_check(h)) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

static int net_calibrate(y355_net *h, const NetInput &in, int B, int freeze, double momentum, int32_t *sa_in_out, int32_t *sa_out,
                         float *max_out) {
    const int keep_in = h->sa_in;
    const bool keep_ok = h->sa_ok;
    const std::vector<int> keep = h->sa;
    const std::vector<float> keep_scale = h->trk_scale;
    const std::vector<int> keep_first = h->trk_first;
    std::vector<float> mx(h->arch->ntensors + 1, 0.f);
    const int rc = net_calibrate_run(h, in, B, freeze, momentum, mx);
    for (auto &L : h->L) L.dirty = true;
    h->front_dirty = true;
    if (rc) {                                                  // the handle keeps the pre-step state
        const std::string msg = y355_last_error();
        (void)hipStreamSynchronize(h->core.stream);
        h->sa_in = keep_in;
        h->sa = keep;
        h->sa_ok = keep_ok;
        h->trk_scale = keep_scale;
        h->trk_first = keep_first;
        return y355_fail(rc, msg);
    }
    h->sa_ok = true;
    if (sa_in_out) *sa_in_out = h->sa_in;
    for (int t = 0; sa_out && t < h->arch->ntensors; ++t) sa_out[t] = h->sa[t];
    for (int k = 0; max_out && k <= h->arch->ntensors; ++k) max_out[k] = mx[k];
    return 0;
}

static int cal_check(y355_net *h, const void *input, int batch, double momentum, int n) {
    if (!h || !input) return y355_fail(Y355_EINVAL, "null argument");
    if (h->bf) return y355_fail(Y355_EINVAL, "calibration steps run on int8 nets");
    if (n != h->arch->ntensors + 1) return y355_fail(Y355_EINVAL, "one tracker for the input and one per tensor expected");
    if (int rc = y355_core_range(&h->core, batch)) return rc;
    if (!(momentum >= 0.0 && momentum <= 1.0)) return y355_fail(Y355_EINVAL, "momentum outside [0, 1]");
    for (const auto &L : h->L)
        if (!L.loaded) return y355_fail(Y355_ENOTREADY, "layer weights not loaded");
    return 0;
}

extern "C" int y355_net_calibrate(y355_net *h, const float *x_dev, int batch, int freeze, double momentum, int32_t *sa_in_out,
                                  int32_t *sa_out, float *max_out, int n) {
    if (int rc = cal_check(h, x_dev, batch, momentum, n)) return rc;
    if (int rc = y355_core_enter(&h->core)) return rc;
    NetInput in;
    in.x = x_dev;
    return net_calibrate(h, in, batch, freeze, momentum, sa_in_out, sa_out, max_out);
}

extern "C" int y355_net_calibrate_u8(y355_net *h, const uint8_t *frames_dev, int src_h, int src_w, int batch, int freeze,
                                     double momentum, int32_t *sa_in_out, int32_t *sa_out, float *max_out, int n) {
    if (int rc = cal_check(h, frames_dev, batch, momentum, n)) return rc;
    if (int rc = y355_core_enter(&h->core, batch, src_h, src_w)) return rc;
    NetInput in;
    if (int rc = u8_input(h, frames_dev, src_h, src_w, false, &in)) return rc;      // conv1.hip reads single bytes: no alignment rule
    return net_calibrate(h, in, batch, freeze, momentum, sa_in_out, sa_out, max_out);
}

extern "C" int y355_net_calibrate_frames(y355_net *h, const y355_frame *frames, int batch, int freeze, double momentum,
                                         int32_t *sa_in_out, int32_t *sa_out, float *max_out, int n) {
    if (int rc = cal_check(h, frames, batch, momentum, n)) return rc;
    if (int rc = y355_frames_check(frames, batch, h->core.max_batch)) return rc;
    if (int rc = y355_core_enter(&h->core)) return rc;
    if (int rc = net_list_buffers(h)) return rc;
    return net_calibrate(h, list_input(h, frames), batch, freeze, momentum, sa_in_out, sa_out, max_out);
}

// ------------------------------------------------------------------------------------------
// Stand-alone detection head on fp32 prediction maps (operator API of the wider model families):
// models/yolo_v2.py:183-210 (one level, anchors in grid units: wh_mul = stride), models/tiny_yolo_v3.py /
// models/yolo_v3.py:207-262 (anchors in pixels: wh_mul = 1): decode, sigmoid(obj) * softmax(cls), threshold,
// per-class NMS, survivors in anchor-index order.  Host pointers, synchronous; pred[l] is NCHW
// [B][A*(5+C)][hs[l]][ws[l]] like the reference's tensors.
extern "C" int y355_head_f32_ex(int device_id, int nlev, const float *const *pred, const int *hs, const int *ws, const float *strides,
                                const float *anchors, int num_anchors, int num_classes, int in_h, int in_w, float wh_mul,
                                float conf_thresh, float nms_thresh, int batch, int max_det, int max_candidates, int route,
                                float *boxes, float *scores, int32_t *cls, int32_t *count, float *cand_box, float *cand_score,
                                int32_t *cand_cls) {
    if (!pred || !hs || !ws || !strides || !anchors || !boxes || !scores || !cls || !count) return y355_fail(Y355_EINVAL, "null argument");
    if (nlev < 1 || nlev > 3) return y355_fail(Y355_EINVAL, "1 to 3 prediction levels");
    if (num_anchors < 1 || num_anchors * nlev > Y355_HEAD_MAXA || num_classes < 1 || batch < 1 || max_det < 1)
        return y355_fail(Y355_EINVAL, "bad anchors / classes / batch / max_det");
    const int predc = num_anchors * (5 + num_classes);
    if (predc > 256) return y355_fail(Y355_EINVAL, "A*(5+C) > 256 not supported");
    int N = 0;
    for (int l = 0; l < nlev; ++l) {
        if (!pred[l] || hs[l] < 1 || ws[l] < 1) return y355_fail(Y355_EINVAL, "bad prediction level");
        N += hs[l] * ws[l] * num_anchors;
    }
    if (N > Y355_NMS_MAX_CAP) return y355_fail(Y355_EINVAL, "more than 65536 anchors per image not supported");
    if (int rc = y355_head_check_option(N, false, route, "head route: 0 (auto) or 1 (large)")) return rc;
    if (int rc = y355_head_check_option(N, true, max_candidates, "max_candidates: 4096 .. min(anchors per image, 65536)")) return rc;
    if ((cand_box || cand_score || cand_cls) && !(cand_box && cand_score && cand_cls))
        return y355_fail(Y355_EINVAL, "the candidate tap takes all three arrays or none");
    HIPCHK(hipSetDevice(device_id));
    if (int e = y355_prepare_kernels()) return e;
    const int B = batch, cpad = y355_pred_channels(predc);
    struct HeadScope {                              // the head's memory and the prediction maps go back whichever way this returns
        HeadState st;
        ~HeadScope() { y355_head_destroy(st); }
    } head;
    HeadState &st = head.st;
    DevScope tmp;
    if (int rc = y355_head_create(st, N, B, max_det, max_candidates, route, cand_box != nullptr, true, y355_hip_mem())) return rc;
    float *d_pred[3] = {nullptr, nullptr, nullptr};
    for (int l = 0; l < nlev; ++l) {
        // NCHW -> NHWC with cpad channels
        const size_t px = (size_t)hs[l] * ws[l];
        std::vector<float> t((size_t)B * px * cpad, 0.f);
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < predc; ++c) {
                const float *src = pred[l] + ((size_t)b * predc + c) * px;
                for (size_t i = 0; i < px; ++i) t[((size_t)b * px + i) * cpad + c] = src[i];
            }
        if (int rc = y355_dev_get(tmp, &d_pred[l], t.size() + 256)) return rc;       // 1024 bytes of slack behind each map
        HIPCHK(hipMemcpy(d_pred[l], t.data(), t.size() * 4, hipMemcpyHostToDevice));
    }
    HeadParams p{};
    p.nlev = nlev;
    for (int l = 0; l < nlev; ++l) {
        HeadLevel &lv = p.lev[l];
        lv.pred = nullptr;
        lv.pred_f = d_pred[l];
        lv.cstride = cpad;
        lv.Hs = hs[l];
        lv.Ws = ws[l];
        lv.stride = strides[l];
        lv.dq = 1.0f;
        for (int i = 0; i < 2 * num_anchors; ++i) lv.anchors[i] = anchors[l * 2 * num_anchors + i];
    }
    p.A = num_anchors;
    p.C = num_classes;
    p.wh_mul = wh_mul;
    y355_head_area_bins(p, hs[0], ws[0]);
    y355_head_fill(p, st, conf_thresh, nms_thresh, in_h, in_w, st.o_box, st.o_score, st.o_cls, st.o_count, true);
    y355_launch_head_nms(p, B, st, 0, nullptr);
    const size_t md = (size_t)st.max_det;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(boxes, st.o_box, sizeof(float) * 4 * md * B, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(scores, st.o_score, sizeof(float) * md * B, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cls, st.o_cls, sizeof(int) * md * B, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(count, st.o_count, sizeof(int) * B, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cand_box) e = y355_head_get_candidates(st, 0, B, cand_box, cand_score, cand_cls);
    int overflow = 0;
    if (e == hipSuccess) e = y355_head_overflow_read(st, 0, &overflow);
    if (overflow) return y355_fail(Y355_EINVAL, y355_head_overflow_message(max_candidates));
    if (e != hipSuccess) return y355_fail(Y355_EHIP, std::string("head: ") + hipGetErrorString(e));
    return 0;
}

extern "C" int y355_head_f32(int device_id, int nlev, const float *const *pred, const int *hs, const int *ws, const float *strides,
                             const float *anchors, int num_anchors, int num_classes, int in_h, int in_w, float wh_mul,
                             float conf_thresh, float nms_thresh, int batch, int max_det, float *boxes, float *scores,
                             int32_t *cls, int32_t *count) {
    return y355_head_f32_ex(device_id, nlev, pred, hs, ws, strides, anchors, num_anchors, num_classes, in_h, in_w, wh_mul, conf_thresh,
                            nms_thresh, batch, max_det, Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO, boxes, scores, cls, count, nullptr, nullptr,
                            nullptr);
}
