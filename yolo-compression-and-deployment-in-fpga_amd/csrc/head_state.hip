// yolo355 -- host state of the detection head (HeadState, head_nms.h): what y355_engine, y355_net and y355_head_f32_ex keep
// for head_nms.hip / nms_large.hip -- the workspace, max_det, the candidate capacity and route, the candidate tap, the host
// calls' outputs.  No kernels here; host_state_check.cpp runs this file's allocation logic on the CPU with an allocator that
// fails on demand.
#include "../../include/yolo355.h"
#include "head_nms.h"

namespace {
int max_det_for(int cfg_max_det, int N, int cap) {
    const int ncand = std::min(N, cap);
    return (cfg_max_det <= 0 || cfg_max_det > ncand) ? ncand : cfg_max_det;
}
}  // namespace

int y355_head_create(HeadState &st, int N, int B_, int cfg_max_det, int cap, int route, bool want_tap, bool want_host_outputs,
                     const DevMem &mem) {
    st = HeadState{};
    st.own.mem = mem;
    st.N = N;
    st.max_batch = B_;
    st.cfg_max_det = cfg_max_det;
    st.cap = Y355_NMS_CAP;
    st.max_det = max_det_for(cfg_max_det, N, Y355_NMS_CAP);
    const size_t B = (size_t)B_, c = Y355_NMS_CAP;
    HeadWork &w = st.wk;
    int rc = 0;             // the first failure; a failed create gives everything back below
    auto get = [&](auto **p, size_t count, bool zero = true) { rc = rc ? rc : y355_dev_get(st.own, p, count, zero); };
    // the small route's arrays (sizes per image: HeadWork); what a kernel reads before it writes starts at zero
    get(&w.cbox, 4 * c * B, false);
    get(&w.cscore, c * B, false);
    get(&w.ccls, c * B, false);
    get(&w.corig, c * B, false);
    get(&w.count, B);
    get(&w.edges, (size_t)Y355_HEAD_EDGE_CAP * B, false);
    get(&w.nedges, 2 * B);
    get(&w.binstart, (c + 8) * B);
    get(&w.astat, 4 * Y355_HEAD_MAXG * B);
    get(&w.tiny, c * B);
    get(&w.ntiny, B);
    get(&w.ctype, c * B);
    get(&w.dbox, 4 * c * B);
    get(&w.dscore, c * B);
    get(&w.dcls, c * B);
    if (want_tap) {
        get(&st.cand_box, 4 * (size_t)N * B, false);
        get(&st.cand_score, (size_t)N * B, false);
        get(&st.cand_cls, (size_t)N * B, false);
    }
    if (want_host_outputs) get(&st.o_count, B);
    if (!rc) rc = y355_head_resize(st, cap, route);     // the raw decode, the large route's lists, o_box / o_score / o_cls
    if (rc) y355_head_destroy(st);
    return rc;
}

void y355_head_destroy(HeadState &st) {
    y355_dev_release_all(st.own);
    const DevMem mem = st.own.mem;
    st = HeadState{};
    st.own.mem = mem;
}

int y355_head_resize(HeadState &st, int cap, int route) {
    static_assert(Y355_NMS_MAX_CAP <= 65536 && Y355_NMS_MAX_CLASSES <= 256, "sort_large_kernel packs class << 16 | rank, 8 + 16 bits");
    const size_t B = (size_t)st.max_batch, c = (size_t)cap;
    const int md = max_det_for(st.cfg_max_det, st.N, cap);
    HeadState nw = st;              // (the owner's list is copied too: small, and only on this cold path)
    HeadWork &w = nw.wk;
    w.lbox = w.lscore = nullptr;
    w.lcls = w.lcount = nullptr;
    w.lsort = nullptr;
    w.lkbox = nullptr;
    w.lkeep = nullptr;
    nw.cap = cap;
    nw.route = route;
    nw.max_det = md;
    const size_t mark = y355_dev_mark(nw.own);      // all or nothing: what is got below goes back if one of them fails
    int rc = 0;
    auto get = [&](auto **p, size_t count) { rc = rc ? rc : y355_dev_get(nw.own, p, count, true); };
    const bool raw = st.N > Y355_NMS_CAP || route == Y355_HEAD_ROUTE_LARGE, big = cap > Y355_NMS_CAP || route == Y355_HEAD_ROUTE_LARGE;
    if (raw && !w.rbox) {           // once there they stay: the launcher hides them from a small head on the automatic route
        w.rstride = (st.N + 3) / 4 * 4;
        get(&w.rbox, 4 * (size_t)w.rstride * B);
        get(&w.rscore, (size_t)w.rstride * B);
        get(&w.rcls, (size_t)w.rstride * B);
        get(&w.rcount, B);
        get(&w.ovf, B);
    }
    if (big) {
        get(&w.lbox, 4 * c * B);
        get(&w.lscore, c * B);
        get(&w.lcls, c * B);
        get(&w.lcount, B);
        get(&w.lsort, 2 * c * B);
        get(&w.lkbox, 4 * c * B);
        get(&w.lkeep, c * B);
    }
    if (st.o_count) {
        get(&nw.o_box, 4 * (size_t)md * B);
        get(&nw.o_score, (size_t)md * B);
        get(&nw.o_cls, (size_t)md * B);
    }
    if (rc) {
        y355_dev_rollback(nw.own, mark);
        return rc;
    }
    HeadWork &o = st.wk;            // what the new arrays replace (o_box .. o_cls are null without o_count)
    y355_dev_drop(nw.own, &o.lbox, &o.lscore, &o.lcls, &o.lcount, &o.lsort, &o.lkbox, &o.lkeep, &st.o_box, &st.o_score, &st.o_cls);
    st = std::move(nw);
    return 0;
}

int y355_head_check_option(int N, bool is_cap, int value, const char *msg) {
    const bool ok = is_cap ? value == Y355_NMS_CAP || (value >= Y355_NMS_CAP && value <= N)
                           : value == Y355_HEAD_ROUTE_AUTO || value == Y355_HEAD_ROUTE_LARGE;
    return ok ? 0 : y355_fail(Y355_EINVAL, msg);
}

hipError_t y355_head_overflow_read(const HeadState &st, hipStream_t s, int *overflow) {
    *overflow = 0;
    if (!st.wk.ovf) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    std::vector<int> v(st.max_batch, 0);
    if (e == hipSuccess) e = hipMemcpy(v.data(), st.wk.ovf, sizeof(int) * v.size(), hipMemcpyDeviceToHost);
    for (int x : v) *overflow |= x != 0;
    if (e == hipSuccess && *overflow) e = hipMemset(st.wk.ovf, 0, sizeof(int) * v.size());
    return e;
}

hipError_t y355_head_overflow_take(const HeadState &st, int *dst_dev, hipStream_t s) {
    const size_t bytes = sizeof(int) * (size_t)st.max_batch;
    const hipError_t e = hipMemcpyAsync(dst_dev, st.wk.ovf, bytes, hipMemcpyDeviceToDevice, s);
    return e != hipSuccess ? e : hipMemsetAsync(st.wk.ovf, 0, bytes, s);
}

hipError_t y355_head_get_candidates(const HeadState &st, hipStream_t s, int batch, float *boxes, float *scores, int32_t *cls) {
    const size_t n = (size_t)st.N * batch;
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(boxes, st.cand_box, sizeof(float) * 4 * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(scores, st.cand_score, sizeof(float) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cls, st.cand_cls, sizeof(int) * n, hipMemcpyDeviceToHost);
    return e;
}

hipError_t y355_head_debug_counts(const HeadState &st, hipStream_t s, int batch, int32_t *count, int32_t *nedges) {
    hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(count, st.wk.count, sizeof(int) * batch, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(nedges, st.wk.nedges, sizeof(int) * 2 * batch, hipMemcpyDeviceToHost);
    return e;
}

void y355_head_fill(HeadParams &p, const HeadState &st, float conf_thresh, float nms_thresh, int in_h, int in_w, float *out_box,
                    float *out_score, int *out_cls, int *out_count, bool tap) {
    p.in_w = (float)in_w;
    p.in_h = (float)in_h;
    p.conf_thresh = conf_thresh;
    p.nms_thresh = nms_thresh;
    p.cand_box = tap ? st.cand_box : nullptr;
    p.cand_score = tap ? st.cand_score : nullptr;
    p.cand_cls = tap ? st.cand_cls : nullptr;
    p.max_det = st.max_det;
    p.out_box = out_box;
    p.out_score = out_score;
    p.out_cls = out_cls;
    p.out_count = out_count;
}
