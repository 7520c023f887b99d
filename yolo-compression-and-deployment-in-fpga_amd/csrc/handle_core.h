// yolo355 -- host state of a model handle before it becomes a network (HandleCore): what y355_engine (engine.hip) and
// y355_net (net.hip) have in common -- the device, the stream, the sizes, the thresholds, the detection head's and the frame
// stage's state, the per-forward counter sets, the profile events, the device allocations -- and the bodies of the entry
// points the two families pair.  Each handle embeds one and adds its layers, tensors and options.  A plain struct and free
// functions, as HeadState and FrameStage; device memory through a DevMem, so host_state_check.cpp runs open / alloc / state /
// close on the CPU (stream and event creation need a device).  The functions take the core as `h`, so that the text of a
// failed HIP call (HIPCHK names the call) reads as it did when these lines stood in the two files.
#pragma once
#include "../../include/yolo355.h"
#include "head_nms.h"

#include <cmath>

struct HandleCore {
    int device_id = 0;
    hipStream_t stream = nullptr;   // the caller's (null: HIP's default stream) or, own_stream, a non-blocking one of the handle's
    bool own_stream = false;
    int max_batch = 0, H = 0, W = 0;    // the network size
    int N = 0;                      // anchors per image, all levels
    float conf_thresh = 0.f, nms_thresh = 0.f;
    HeadState head;                 // the head's workspace, max_det, candidate tap, outputs of the host calls
    FrameStage stage;               // BaseTransform constants, the resize routes' buffers
    Counters *ctr_dev = nullptr;    // [ctrs.n]: the set the last forward counted into (one of ctrs' two)
    CounterSets ctrs;
    unsigned int *absmax_dev = nullptr;
    int profile = 0;
    std::vector<hipEvent_t> ev;     // n + 1 events around the n profile intervals of a forward
    DevOwner own;                   // the layers' buffers, the counter sets, the absmax word
};

// the configuration rules the two creates share, in their order; mult: the size multiple, max_anchors: per level
inline int y355_core_check_config(int height, int width, int mult, int num_anchors, int max_anchors, int num_classes, int max_batch, int N) {
    if (height <= 0 || width <= 0 || height % mult || width % mult)
        return y355_fail(Y355_EINVAL, "input size must be a positive multiple of " + std::to_string(mult));
    if (num_anchors < 1 || num_anchors > max_anchors || num_classes < 1) return y355_fail(Y355_EINVAL, "bad anchors / classes");
    if (max_batch < 1) return y355_fail(Y355_EINVAL, "max_batch < 1");
    if (num_anchors * (5 + num_classes) > 256) return y355_fail(Y355_EINVAL, "A*(5+C) > 256 not supported");
    if (N > Y355_NMS_MAX_CAP) return y355_fail(Y355_EINVAL, "more than 65536 anchors per image not supported");
    return 0;
}

// adopts the caller's stream or creates the handle's own (the device is set)
inline int y355_core_open(HandleCore *h, int device_id, void *stream, bool own_stream, int H, int W, int max_batch, int N, float conf,
                          float nms, const DevMem &mem) {
    h->device_id = device_id;
    h->H = H;
    h->W = W;
    h->max_batch = max_batch;
    h->N = N;
    h->conf_thresh = conf;
    h->nms_thresh = nms;
    h->own.mem = mem;
    y355_stage_init(h->stage, H, W, max_batch, mem);
    h->stream = (hipStream_t)stream;                 // NULL = default stream (torch's default on ROCm)
    if (!own_stream) return 0;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        h->stream = nullptr;
        return y355_fail(Y355_EHIP, "hipStreamCreate failed");
    }
    h->own_stream = true;
    return 0;
}

// device memory the handle owns until y355_core_close
template <typename T>
inline int y355_core_alloc(HandleCore *h, T **p, size_t bytes, bool zero) {
    return y355_dev_get(h->own, p, bytes, zero, 1);
}

// the two counter sets of n_ctr each, the absmax word and the head's state
inline int y355_core_state(HandleCore *h, int n_ctr, int max_det, bool host_outputs) {
    if (int rc = y355_core_alloc(h, &h->ctr_dev, sizeof(Counters) * 2 * n_ctr, true)) return rc;
    h->ctrs.base = h->ctr_dev;
    h->ctrs.n = n_ctr;
    h->ctrs.clean[0] = h->ctrs.clean[1] = true;       // zeroed by the allocation
    if (int rc = y355_core_alloc(h, &h->absmax_dev, 16, true)) return rc;
    return y355_head_create(h->head, h->N, h->max_batch, max_det, Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO, true, host_outputs, h->own.mem);
}

// the events around n profile intervals
inline int y355_core_events(HandleCore *h, int n) {
    for (int i = 0; i <= n; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return y355_fail(Y355_EHIP, "hipEventCreate failed");
        h->ev.push_back(e);
    }
    return 0;
}

// waits for the stream, then returns everything; a second call does nothing
inline void y355_core_close(HandleCore *h) {
    (void)hipSetDevice(h->device_id);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    y355_dev_release_all(h->own);
    y355_head_destroy(h->head);
    y355_stage_destroy(h->stage);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear();
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->stream = nullptr;
    h->own_stream = false;
}

// a create that failed with rc: destroy() takes the half-built handle down, the failure's message stays
template <typename F>
inline int y355_core_unwind(int rc, F destroy) {
    const std::string keep = y355_last_error();
    destroy();
    return y355_fail(rc, keep);
}

// batch within the handle's; a frame size (none: 1 x 1) within the resize stage's
inline int y355_core_range(const HandleCore *h, int batch, int frame_h = 1, int frame_w = 1) {
    if (batch < 1 || batch > h->max_batch) return y355_fail(Y355_EINVAL, "batch out of range");
    if (frame_h < 1 || frame_w < 1 || frame_h > 16384 || frame_w > 16384) return y355_fail(Y355_EINVAL, "bad frame size");
    return 0;
}
// the top of a call: that check, then the handle's device
inline int y355_core_enter(const HandleCore *h, int batch = 1, int frame_h = 1, int frame_w = 1) {
    if (int rc = y355_core_range(h, batch, frame_h, frame_w)) return rc;
    HIPCHK(hipSetDevice(h->device_id));
    return 0;
}

// the start of a forward: the counter set it counts into (steady state: zeroed by the previous forward's front end, no launch here)
inline int y355_core_begin_counters(HandleCore *h) {
    bool need_zero = false;
    h->ctr_dev = h->ctrs.begin(&need_zero);
    if (need_zero) HIPCHK((hipError_t)y355_zero_counters(h->ctr_dev, h->ctrs.n, h->stream));
    return 0;
}
// the last forward's counts, summed over the set: clamped values (input quantisation included), head-room violations; synchronous
inline int y355_core_counters(const HandleCore *h, int64_t *saturated, int64_t *guard) {
    if (int rc = y355_core_enter(h)) return rc;
    std::vector<Counters> v(h->ctrs.n);
    HIPCHK(hipMemcpyAsync(v.data(), h->ctr_dev, sizeof(Counters) * v.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int64_t s = 0, g = 0;
    for (const Counters &k : v) {
        s += (int64_t)k.sat + (int64_t)k.in_sat;
        g += (int64_t)k.guard;
    }
    if (saturated) *saturated = s;
    if (guard) *guard = g;
    return 0;
}

// the maximum a kernel just enqueued leaves in the absmax word (bits of a non-negative fp32), back on the host; synchronous
inline int y355_core_absmax_read(const HandleCore *h, float *out_max) {
    HIPCHK(hipGetLastError());
    unsigned int bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, h->absmax_dev, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(out_max, &bits, 4);
    return 0;
}

// candidate capacity (is_cap) or route of the head; msg: the family's text for a value out of range
inline int y355_core_head_option(HandleCore *h, bool is_cap, int value, const char *msg) {
    if (int rc = y355_head_check_option(h->N, is_cap, value, msg)) return rc;
    if (int rc = y355_core_enter(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));          // nothing in flight reads the arrays that go
    if (y355_head_set_option(h->head, is_cap, value)) return y355_fail(Y355_EHIP, "device allocation failed");
    return 0;
}
inline int y355_core_set_thresholds(HandleCore *h, float conf, float nms) {
    h->conf_thresh = conf;
    h->nms_thresh = nms;
    return 0;
}
inline int y355_core_overflow(const HandleCore *h, int *overflow) {
    if (int rc = y355_core_enter(h)) return rc;
    HIPCHK(y355_head_overflow_read(h->head, h->stream, overflow));
    return 0;
}
inline int y355_core_get_candidates(const HandleCore *h, int batch, float *boxes, float *scores, int32_t *cls) {
    if (int rc = y355_core_enter(h, batch)) return rc;
    HIPCHK(y355_head_get_candidates(h->head, h->stream, batch, boxes, scores, cls));
    return 0;
}
inline int y355_core_scale_boxes(const HandleCore *h, float *boxes_dev, const int32_t *count_dev, const float *wh_dev, int batch) {
    if (int rc = y355_core_enter(h, batch)) return rc;
    y355_launch_scale_boxes(boxes_dev, count_dev, wh_dev, batch, h->head.max_det, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
// the ragged stage: a frame list -> out_dev [batch][H][W][3]
inline int y355_core_resize_frames(HandleCore *h, const y355_frame *frames, int batch, uint8_t *out_dev) {
    if (int rc = y355_frames_check(frames, batch, h->max_batch)) return rc;
    if (int rc = y355_core_enter(h)) return rc;
    if (int rc = y355_stage_need_list(h->stage)) return rc;
    y355_launch_resize_frames(frames, batch, out_dev, h->stage.tabs, h->H, h->W, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
// the same-size stage: frames [batch][src_h][src_w][3] -> out_dev [batch][H][W][3] (the device is set)
inline int y355_core_resize_u8(HandleCore *h, const uint8_t *frames_dev, int src_h, int src_w, int batch, uint8_t *out_dev) {
    if (int rc = y355_stage_tables_for(h->stage, src_h, src_w, h->stream)) return rc;
    y355_launch_resize_u8(frames_dev, out_dev, h->stage.tab, batch, src_h, src_w, h->H, h->W, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
inline int y355_core_sync(const HandleCore *h) {
    if (int rc = y355_core_enter(h)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
// ms [n]: the profile intervals of the last forward
inline int y355_core_profile_get(const HandleCore *h, int n, float *ms) {
    if (int rc = y355_core_enter(h)) return rc;
    HIPCHK(hipEventSynchronize(h->ev[n]));
    for (int i = 0; i < n; ++i) HIPCHK(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
    return 0;
}

// ---- AveragedRangeTracker state (models/slim_yolo_v2.py:13-14): scale / first_a arrays of n trackers
// exponent = floor(log2(scale)) (:33), log2 in fp32.  0, or what is wrong: 1 the scale is not a positive finite number, 2 the
// exponent is outside [-64, 64]
inline int y355_tracker_exponent(float scale, int *e) {
    if (!(scale > 0.f) || !std::isfinite(scale)) return 1;
    *e = (int)std::floor(std::log2(scale));
    return (*e < -64 || *e > 64) ? 2 : 0;
}
inline void y355_trackers_set(float *scale, int *first, int n, const float *scale_in, const int32_t *first_a) {
    for (int i = 0; i < n; ++i) {
        scale[i] = scale_in[i];
        first[i] = first_a[i] ? 1 : 0;
    }
}
inline void y355_trackers_get(const float *scale, const int *first, int n, float *scale_out, int32_t *first_a) {
    for (int i = 0; i < n; ++i) {
        scale_out[i] = scale[i];
        first_a[i] = first[i];
    }
}
