// Host-only check of the allocation logic in csrc/y355_host.h (DevOwner), csrc/head_state.hip (HeadState: create, resize's
// swap and rollback, destroy), csrc/resize.hip (FrameStage: lazy buffers, the cached same-size table), csrc/handle_core.h
// (HandleCore: a create's allocations and its unwinding; not its stream and events, which need a device), csrc/apeval.hip and
// csrc/cocoeval.hip (y355_apeval: create-time buffers, the two ground truths, the COCO workspaces, staging, close),
// csrc/pipeline_slot.h (a pipeline slot's outputs), csrc/conv_op_state.h (ConvOpMem of the operator layer's y355_conv_op:
// create-time buffers, the weight swap, the workspaces and the geometry each was last zeroed for, the close) and the two
// companion libraries' handles, csrc/loss.hip (y355_loss) and
// csrc/anchors.hip (y355_anchors): the device-free half of each create, its buffers, their unwinding, the close.  Device memory
// is the host heap here, through
// a DevMem whose k-th allocation (or whose upload) fails on demand, so the program needs no GPU.  Built with the address and
// undefined-behaviour sanitizers by `make -C csrc hostcheck`: a leak, a double free or a use after free ends it non-zero.
#include "../include/yolo355.h"
#include "../include/yolo355_anchors.h"
#include "../include/yolo355_loss.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/apeval_shared.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/conv_op_state.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/handle_core.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/pipeline_slot.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::string g_err;
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
extern "C" const char *y355_last_error(void) { return g_err.c_str(); }

// the companions' handles (loss.hip, anchors.hip; the structs stay theirs): the device-free half of a create, the buffers, the
// owner, and what a destroy does once the device is set
int loss_open(const y355_loss_config *cfg, const DevMem &mem, y355_loss **out);
int loss_buffers(y355_loss *h);
DevOwner &loss_owner(y355_loss *h);
void loss_free(y355_loss *h);
int anchors_open(int32_t device_id, int64_t max_boxes, int32_t max_restarts, int32_t max_k, const DevMem &mem, y355_anchors **out);
int anchors_buffers(y355_anchors *h);
DevOwner &anchors_owner(y355_anchors *h);
void anchors_free(y355_anchors *h);

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

namespace {
std::set<void *> live;
int n_alloc = 0, fail_at = -1, n_upload = 0;
size_t n_bytes = 0;                                 // asked for since it was last cleared
bool fail_upload = false;

DevMem host_mem() {
    DevMem m;
    m.alloc = [](void **p, size_t bytes, bool zero) -> int {
        if (n_alloc++ == fail_at) return y355_fail(Y355_EHIP, "injected allocation failure");
        n_bytes += bytes;
        *p = zero ? calloc(1, bytes ? bytes : 16) : malloc(bytes ? bytes : 16);
        live.insert(*p);
        return 0;
    };
    m.release = [](void *p) {
        CHECK(live.erase(p) == 1);          // released once, and only what alloc returned
        free(p);
    };
    m.upload = [](void *dst, const void *src, size_t bytes, hipStream_t) -> int {
        if (fail_upload) return y355_fail(Y355_EHIP, "injected upload failure");
        ++n_upload;
        memcpy(dst, src, bytes);
        return 0;
    };
    return m;
}

// everything of a HeadState a failed resize must leave alone
std::vector<uintptr_t> snapshot(const HeadState &s) {
    const HeadWork &w = s.wk;
    const void *ptrs[] = {w.cbox, w.cscore, w.ccls, w.corig, w.count, w.edges, w.nedges, w.binstart, w.astat, w.tiny, w.ntiny, w.ctype,
                          w.dbox, w.dscore, w.dcls, w.rbox, w.rscore, w.rcls, w.rcount, w.ovf, w.lbox, w.lscore, w.lcls, w.lcount, w.lsort,
                          w.lkbox, w.lkeep, s.cand_box, s.cand_score, s.cand_cls, s.o_box, s.o_score, s.o_cls, s.o_count};
    std::vector<uintptr_t> v;
    for (const void *p : ptrs) v.push_back((uintptr_t)p);
    for (int x : {w.rstride, s.N, s.max_batch, s.cfg_max_det, s.max_det, s.cap, s.route}) v.push_back((uintptr_t)x);
    for (void *p : s.own.allocs) v.push_back((uintptr_t)p);
    return v;
}
bool owns_exactly_live(const DevOwner &o) { return std::set<void *>(o.allocs.begin(), o.allocs.end()) == live && o.allocs.size() == live.size(); }
bool owns_exactly_live(const HeadState &s) { return owns_exactly_live(s.own); }

void check_head(int N, int B, int cfg_max_det, bool tap, bool outs) {
    const DevMem mem = host_mem();
    HeadState st;
    fail_at = -1;
    n_alloc = 0;
    CHECK(y355_head_create(st, N, B, cfg_max_det, Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO, tap, outs, mem) == 0);
    const int n_create = n_alloc;
    CHECK(owns_exactly_live(st) && (int)live.size() == n_create);
    CHECK((st.cand_box != nullptr) == tap && (st.o_box != nullptr) == outs && (st.o_count != nullptr) == outs);
    CHECK((st.wk.rbox != nullptr) == (N > Y355_NMS_CAP) && !st.wk.lbox);
    y355_head_destroy(st);
    CHECK(live.empty());
    for (int k = 0; k < n_create; ++k) {            // a create that fails at its k-th allocation frees what it took
        fail_at = k;
        n_alloc = 0;
        CHECK(y355_head_create(st, N, B, cfg_max_det, Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO, tap, outs, mem) != 0);
        CHECK(live.empty() && st.own.allocs.empty() && !st.wk.cbox);
    }
    fail_at = -1;
    CHECK(y355_head_create(st, N, B, cfg_max_det, Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO, tap, outs, mem) == 0);
    const int big = std::min(N, 2 * Y355_NMS_CAP);
    const int steps[][2] = {{big, Y355_HEAD_ROUTE_AUTO},          {Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO}, {Y355_NMS_CAP, Y355_HEAD_ROUTE_LARGE},
                            {big, Y355_HEAD_ROUTE_LARGE},         {big, Y355_HEAD_ROUTE_AUTO},          {Y355_NMS_CAP, Y355_HEAD_ROUTE_AUTO}};
    for (const auto &sp : steps) {
        const int cap = sp[0] < Y355_NMS_CAP ? Y355_NMS_CAP : sp[0], route = sp[1];
        const std::vector<uintptr_t> before = snapshot(st);
        const std::set<void *> live_before = live;
        // the step with its k-th allocation failing, k = 0, 1, ...: nothing may change; the first k it does not reach (a step
        // makes at most 15: 5 raw + 7 large + 3 outputs) is the step itself
        bool done = false;
        for (int k = 0; k <= 15 && !done; ++k) {
            fail_at = k;
            n_alloc = 0;
            done = y355_head_resize(st, cap, route) == 0;
            if (done) CHECK(n_alloc <= k);
            else CHECK(snapshot(st) == before && live == live_before);
        }
        CHECK(done);
        fail_at = -1;
        const int ncand = std::min(N, cap);
        CHECK(st.cap == cap && st.route == route && y355_head_capacity(st) == cap);
        CHECK(st.max_det == ((cfg_max_det <= 0 || cfg_max_det > ncand) ? ncand : cfg_max_det));
        CHECK((st.wk.lbox != nullptr) == (cap > Y355_NMS_CAP || route == Y355_HEAD_ROUTE_LARGE));
        CHECK(owns_exactly_live(st));
    }
    y355_head_destroy(st);
    CHECK(live.empty());
}

void check_stage() {
    const int H = 96, W = 160, B = 3;
    FrameStage st;
    y355_stage_init(st, H, W, B, host_mem());
    fail_at = -1;
    n_alloc = n_upload = 0;
    // set_normalization: all three channels are checked before one is assigned
    const NormU8 norm0 = st.norm;
    const float mean[3] = {0.1f, 0.2f, 0.3f}, bad[3] = {0.f, 1.f, 1.f}, good[3] = {0.5f, 0.6f, 0.7f};
    CHECK(y355_stage_set_normalization(st, mean, bad) == Y355_EINVAL && g_err == "std must be positive");
    CHECK(memcmp(&st.norm, &norm0, sizeof norm0) == 0);
    CHECK(y355_stage_set_normalization(st, mean, good) == 0 && st.norm.mean[0] == 0.3f && st.norm.sd[2] == 0.5f);
    // tables_for: one allocation, one upload per change of the source size
    std::vector<int> want(3 * (size_t)(H + W));
    CHECK(!st.tab && !st.frames && !st.tabs);
    fail_at = 0;
    CHECK(y355_stage_tables_for(st, 480, 640, nullptr) != 0 && !st.tab && st.src_h == 0 && live.empty());
    fail_at = -1;
    CHECK(y355_stage_tables_for(st, 480, 640, nullptr) == 0 && n_upload == 1 && st.src_h == 480 && st.src_w == 640);
    y355_resize_tables(480, 640, H, W, want.data());
    CHECK(memcmp(st.tab, want.data(), sizeof(int) * want.size()) == 0);
    CHECK(y355_stage_tables_for(st, 480, 640, nullptr) == 0 && n_upload == 1);       // cached
    CHECK(y355_stage_tables_for(st, 640, 480, nullptr) == 0 && n_upload == 2);       // (a swapped size is another size)
    y355_resize_tables(640, 480, H, W, want.data());
    CHECK(memcmp(st.tab, want.data(), sizeof(int) * want.size()) == 0);
    fail_upload = true;                             // a failed upload forgets the cached size: the next call uploads again
    CHECK(y355_stage_tables_for(st, 300, 300, nullptr) != 0 && st.src_h == 0 && st.src_w == 0);
    fail_upload = false;
    CHECK(y355_stage_tables_for(st, 640, 480, nullptr) == 0 && n_upload == 3);
    CHECK(live.size() == 1 && !st.frames && !st.tabs);          // each buffer only when its route needs it
    CHECK(y355_stage_need_list(st) == 0 && st.tabs && !st.frames && live.size() == 2);
    fail_at = n_alloc;
    CHECK(y355_stage_need_frames(st) != 0 && !st.frames && live.size() == 2);
    fail_at = -1;
    CHECK(y355_stage_need_frames(st) == 0 && st.frames && live.size() == 3);
    CHECK(y355_stage_need_frames(st) == 0 && y355_stage_need_list(st) == 0 && live.size() == 3);
    y355_stage_destroy(st);
    CHECK(live.empty() && !st.tab && !st.frames && !st.tabs);
    // the list rules, in order
    uint8_t px[12] = {};
    y355_frame f[2] = {{px, 1, 2, 0}, {px, 2, 1, 8}};
    CHECK(y355_frames_check(nullptr, 1, 2) == Y355_EINVAL && g_err == "null frame array");
    CHECK(y355_frames_check(f, 3, 2) == Y355_EINVAL && g_err == "batch out of range");
    CHECK(y355_frames_check(f, 2, 2) == 0);
    f[1].row_bytes = 2;
    CHECK(y355_frames_check(f, 2, 2) == Y355_EINVAL && g_err == "row_bytes below width * 3");
    f[1].width = 16385;
    CHECK(y355_frames_check(f, 2, 2) == Y355_EINVAL && g_err == "bad frame size");
    f[1].data_dev = nullptr;
    CHECK(y355_frames_check(f, 2, 2) == Y355_EINVAL && g_err == "null frame pointer");
}

// a create's worth of allocations on a HandleCore (a borrowed null stream: no HIP object is made), as y355_create and
// y355_net_create make them: layer buffers, then the counter sets, the absmax word and the head
int core_create(HandleCore &c, int N, bool outs) {
    int rc = y355_core_open(&c, 0, nullptr, false, 96, 160, 2, N, 0.01f, 0.5f, host_mem());
    char *layer[6] = {};
    for (int k = 0; k < 6 && !rc; ++k) rc = y355_core_alloc(&c, &layer[k], (size_t)1000 * k, k % 2 == 0);
    if (!rc) rc = y355_core_state(&c, 11, 0, outs);
    if (!rc) rc = y355_stage_need_frames(c.stage);
    return rc ? y355_core_unwind(rc, [&c] { y355_core_close(&c); }) : 0;
}
void check_core(int N, bool outs) {
    fail_at = -1;
    n_alloc = 0;
    {
        HandleCore c;
        CHECK(core_create(c, N, outs) == 0 && !c.own_stream && !c.stream && c.ev.empty());
        CHECK(c.ctrs.base == c.ctr_dev && c.ctrs.n == 11 && c.ctrs.clean[0] && c.ctrs.clean[1] && c.absmax_dev);
        CHECK(c.own.allocs.size() == 8 && c.own.allocs.size() + c.head.own.allocs.size() + c.stage.own.allocs.size() == live.size());
        CHECK(y355_core_range(&c, 0) == Y355_EINVAL && g_err == "batch out of range" && y355_core_range(&c, 3) == Y355_EINVAL);
        CHECK(y355_core_range(&c, 2, 16385, 1) == Y355_EINVAL && g_err == "bad frame size" && y355_core_range(&c, 2, 16384, 1) == 0);
        y355_core_close(&c);
        CHECK(live.empty() && c.own.allocs.empty());
        y355_core_close(&c);                        // a second close is harmless
    }
    const int n_create = n_alloc;
    for (int k = 0; k < n_create; ++k) {            // the k-th allocation fails: everything taken goes back once, the message stays
        HandleCore c;
        fail_at = k;
        n_alloc = 0;
        g_err.clear();
        CHECK(core_create(c, N, outs) == Y355_EHIP);
        CHECK(live.empty() && c.own.allocs.empty() && c.head.own.allocs.empty() && c.stage.own.allocs.empty() && !c.stage.frames);
        CHECK(g_err == "injected allocation failure" && std::string(y355_last_error()) == "injected allocation failure");
        y355_core_close(&c);
        CHECK(live.empty());
    }
    fail_at = -1;
}

// ---- DevOwner: get, drop, grow, group grow, mark / rollback, release all
void check_owner() {
    DevOwner o{host_mem(), {}};
    int dummy = 0, *a = &dummy;
    fail_at = 0, n_alloc = 0;
    CHECK(y355_dev_get(o, &a, 10) == Y355_EHIP && a == &dummy && live.empty() && o.allocs.empty());      // *p as it was
    fail_at = -1;
    CHECK(y355_dev_get(o, &a, 10, true) == 0 && a != &dummy && a[9] == 0 && owns_exactly_live(o) && live.size() == 1);
    double *none = nullptr;
    y355_dev_drop(o, &none);                        // null: nothing
    y355_dev_drop(o, &a);
    CHECK(!a && live.empty() && o.allocs.empty());
    // grow
    size_t have = 0;
    fail_at = 0, n_alloc = 0;
    CHECK(y355_dev_grow(o, &have, 10, &a) == Y355_EHIP && !a && have == 0 && live.empty());
    fail_at = -1;
    CHECK(y355_dev_grow(o, &have, 10, &a) == 0 && a && have == 10 && live.size() == 1);
    a[9] = 1;
    const int *a10 = a;
    n_alloc = 0;
    CHECK(y355_dev_grow(o, &have, 5, &a) == 0 && a == a10 && have == 10 && n_alloc == 0);       // smaller: nothing
    fail_at = 0;
    CHECK(y355_dev_grow(o, &have, 20, &a) == Y355_EHIP && !a && have == 0 && live.empty() && o.allocs.empty());
    fail_at = -1;
    CHECK(y355_dev_grow(o, &have, 20, &a) == 0 && have == 20 && owns_exactly_live(o));
    a[19] = 1;
    // group grow: three arrays of two element types, one capacity
    double *b = nullptr;
    char *c = nullptr;
    unsigned int *d = nullptr;
    size_t cap = 0;
    for (size_t need : {(size_t)7, (size_t)3000}) {
        for (int k = 0; k < 3; ++k) {
            fail_at = k, n_alloc = 0;
            CHECK(y355_dev_grow(o, &cap, need, &b, &c, &d) == Y355_EHIP && !b && !c && !d && cap == 0);
            CHECK(live.size() == 1 && owns_exactly_live(o));     // (a stays)
        }
        fail_at = -1, n_alloc = 0;
        CHECK(y355_dev_grow(o, &cap, need, &b, &c, &d) == 0 && b && c && d && cap == need && n_alloc == 3 && live.size() == 4);
        b[need - 1] = 1.0, c[need - 1] = 1, d[need - 1] = 1u;
        CHECK(y355_dev_grow(o, &cap, need - 1, &b, &c, &d) == 0 && cap == need && n_alloc == 3);
    }
    // all or nothing
    const size_t mark = y355_dev_mark(o);
    int *x = nullptr, *y = nullptr;
    CHECK(y355_dev_get(o, &x, 4) == 0 && y355_dev_get(o, &y, 4) == 0 && live.size() == 6);
    y355_dev_rollback(o, mark);
    CHECK(live.size() == 4 && owns_exactly_live(o));
    y355_dev_release_all(o);
    CHECK(live.empty() && o.allocs.empty());
    y355_dev_release_all(o);                        // a second one is harmless
}

// ---- the evaluator handle (no stream, no event: a null stream goes to the uploads)
bool ap_all_null(const y355_apeval &e) {
    const void *p[] = {e.gt_off, e.gt_box, e.gt_cls, e.gt_diff, e.gt_first, e.ctr, e.d_imgpos, e.d_cls, e.d_score, e.d_box, e.khi, e.perm[0],
                       e.perm[1], e.hist, e.dtot, e.jm, e.flag, e.rec, e.prec, e.start, e.ap, e.stage, e.coco};
    for (const void *q : p)
        if (q) return false;
    return e.own.allocs.empty() && !e.have_gt && !e.have_curve && e.stage_bytes == 0;
}
void ap_sizes(y355_apeval &e, long long max_dets) {
    e.C = 3, e.num_images = 2, e.cap = max_dets, e.own.mem = host_mem();
}
void check_apeval_buffers(long long max_dets) {
    y355_apeval e;
    ap_sizes(e, max_dets);
    fail_at = -1, n_alloc = 0;
    CHECK(ap_buffers(&e) == 0);
    const int n_create = n_alloc;
    const size_t n = (size_t)max_dets, tiles = (n + AP_TILE - 1) / AP_TILE;
    CHECK(n_create == 16 && (int)live.size() == n_create && owns_exactly_live(e.own));
    e.ctr[7] = 1, e.d_box[4 * n - 1] = 1.f, e.perm[1][n - 1] = 1u, e.hist[256 * tiles - 1] = 1u, e.dtot[255] = 1u, e.prec[n - 1] = 1.0;
    e.start[e.C] = 1, e.ap[e.C - 1] = 1.0;          // (the sanitizer sees a buffer that is too short)
    ap_close(&e);
    CHECK(live.empty() && ap_all_null(e) && e.C == 3 && e.cap == max_dets);
    for (int k = 0; k < n_create; ++k) {
        fail_at = k, n_alloc = 0;
        CHECK(ap_buffers(&e) == Y355_EHIP && live.empty() && ap_all_null(e) && g_err == "injected allocation failure");
    }
    fail_at = -1;
    CHECK(ap_buffers(&e) == 0 && owns_exactly_live(e.own));
    ap_close(&e);
    ap_close(&e);                                   // twice; the COCO part was never made
    CHECK(live.empty() && ap_all_null(e));
}

const int32_t kOff2[3] = {0, 1, 2}, kCls2[2] = {0, 1}, kOff5[3] = {0, 3, 5}, kCls5[5] = {2, 0, 2, 1, 1};
const uint8_t kDiff2[2] = {0, 1}, kDiff5[5] = {0, 0, 1, 0, 0};
const float kBox[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20};

void check_apeval_gt() {
    for (int k = 0; k < 5; ++k) {                   // the k-th allocation of the replacement fails
        y355_apeval e;
        ap_sizes(e, 8);
        fail_at = -1;
        CHECK(ap_buffers(&e) == 0 && ap_set_gt(&e, kOff2, kBox, kCls2, kDiff2) == 0 && e.have_gt && e.n_gt == 2);
        CHECK(e.npos == std::vector<int32_t>({1, 0, 0}) && memcmp(e.gt_box, kBox, 32) == 0 && memcmp(e.gt_off, kOff2, 12) == 0);
        CHECK(live.size() == 21 && owns_exactly_live(e.own));
        e.have_curve = true;
        for (int round = 0; round < 2; ++round) {
            fail_at = k, n_alloc = 0;
            CHECK(ap_set_gt(&e, kOff5, kBox, kCls5, kDiff5) == Y355_EHIP && !e.have_gt && !e.have_curve && e.n_gt != 5);
            CHECK(owns_exactly_live(e.own));
            if (round) break;
            fail_at = -1;                           // a retry
            CHECK(ap_set_gt(&e, kOff5, kBox, kCls5, kDiff5) == 0 && e.have_gt && e.n_gt == 5 && e.npos == std::vector<int32_t>({1, 2, 1}));
            CHECK(memcmp(e.gt_box, kBox, 80) == 0 && memcmp(e.gt_diff, kDiff5, 5) == 0 && live.size() == 21 && owns_exactly_live(e.own));
            e.gt_first[4] = 0;
        }
        fail_at = -1;
        if (k == 0) {                               // an upload that fails
            fail_upload = true;
            CHECK(ap_set_gt(&e, kOff2, kBox, kCls2, kDiff2) == Y355_EHIP && !e.have_gt && owns_exactly_live(e.own));
            fail_upload = false;
        }
        ap_close(&e);                               // close returns everything
        CHECK(live.empty() && ap_all_null(e));
    }
}

int coco_gt(y355_apeval &e, int n, std::vector<int32_t> *cls_left = nullptr) {
    const int32_t *off = n == 2 ? kOff2 : kOff5, rank[2] = {1, 0};
    std::vector<int32_t> h_cls(n == 2 ? kCls2 : kCls5, (n == 2 ? kCls2 : kCls5) + n);
    std::vector<double> h_box(kBox, kBox + 4 * n), h_area(n, 100.0);
    std::vector<uint8_t> h_crowd(n, 0);
    const int rc = coco_set_gt(&e, off, rank, h_box, h_cls, h_area, h_crowd);
    if (cls_left) *cls_left = h_cls;
    return rc;
}
void check_coco() {
    std::vector<int32_t> left;
    for (int k = 0; k < 6; ++k) {                   // the COCO ground truth, as the VOC one; the host copies move on success only
        y355_apeval e;
        ap_sizes(e, 8);
        fail_at = -1;
        CHECK(ap_buffers(&e) == 0 && coco_gt(e, 2, &left) == 0 && e.coco && e.coco->have_gt && e.coco->n_gt == 2 && left.empty());
        CHECK(e.coco->h_cls.size() == 2 && e.coco->h_area.size() == 2 && e.coco->h_crowd.size() == 2 && live.size() == 22);
        e.coco->have_result = true;
        fail_at = k, n_alloc = 0;
        CHECK(coco_gt(e, 5, &left) == Y355_EHIP && !e.coco->have_gt && !e.coco->have_result && e.coco->n_gt != 5);
        CHECK(left.size() == 5 && e.coco->h_cls.size() == 2 && e.coco->h_area.size() == 2 && e.coco->h_crowd.size() == 2 && owns_exactly_live(e.own));
        fail_at = -1;
        if (k % 2) {
            CHECK(coco_gt(e, 5, &left) == 0 && e.coco->have_gt && e.coco->n_gt == 5 && left.size() == 2 && e.coco->h_cls.size() == 5);
            CHECK(e.coco->h_crowd.size() == 5 && e.coco->img_rank[0] == 1 && e.coco->gt_box[19] == 20.0 && live.size() == 22 && owns_exactly_live(e.own));
        }
        ap_close(&e);
        CHECK(live.empty() && ap_all_null(e));
    }
    // the workspaces
    y355_apeval e;
    ap_sizes(e, 8);
    CHECK(ap_buffers(&e) == 0 && coco_gt(e, 5) == 0);
    e.coco->n_gt = 4;                               // (n 10, n_gt 4, A 4, T 10)
    y355_coco *c = e.coco;
    n_alloc = 0;
    CHECK(coco_workspaces(&e, 10, 10, 101, 4, 3) == 0 && n_alloc == 11 && c->n_cap == 10 && c->flags_cap == 400 && c->marks_cap == 160);
    CHECK(c->prec_cap == (size_t)10 * 101 * 3 * 4 * 3 && c->rec_cap == 360 && owns_exactly_live(e.own));
    c->npig[3 * COCO_MAX_A - 1] = 1, c->rec_thrs[COCO_MAX_R - 1] = 1.0, c->w0[9] = 1, c->gidx[9] = 1u, c->flags[399] = 1, c->marks[159] = 1;
    CHECK(coco_workspaces(&e, 5, 10, 101, 4, 3) == 0 && n_alloc == 11 && c->n_cap == 10);       // fewer detections: nothing
    bool done = false;
    for (int k = 0; k <= 6 && !done; ++k) {         // 3000 detections: the five arrays of n_cap and the flags, a failure at every k
        fail_at = k, n_alloc = 0;
        done = coco_workspaces(&e, 3000, 10, 101, 4, 3) == 0;
        const bool gone = !c->permA;
        CHECK(gone == !c->permB && gone == !c->gkey && gone == !c->gidx && gone == !c->w0 && gone == (c->n_cap == 0));
        CHECK(!c->flags == (c->flags_cap == 0) && owns_exactly_live(e.own) && (done || g_err == "injected allocation failure"));
    }
    fail_at = -1;
    CHECK(done && c->n_cap == 3000 && c->flags_cap == (size_t)40 * 3000 && c->marks_cap == 160 && live.size() == 22 + 11);
    c->permB[2999] = 1u, c->flags[40 * 3000 - 1] = 1;
    // the tap and the staging buffer
    CHECK(coco_tap(&e, 100) == 0 && c->tap_cap == 100 && live.size() == 34);
    fail_at = n_alloc;
    CHECK(coco_tap(&e, 1000) == Y355_EHIP && !c->tap && c->tap_cap == 0 && live.size() == 33);
    fail_at = -1;
    CHECK(coco_tap(&e, 1000) == 0 && c->tap_cap == 1000 && coco_tap(&e, 10) == 0 && c->tap_cap == 1000);
    c->tap[999] = 1;
    CHECK(ap_stage(&e, 1024) == 0 && e.stage_bytes == 1024 && live.size() == 35);
    fail_at = n_alloc;
    CHECK(ap_stage(&e, 1 << 20) == Y355_EHIP && !e.stage && e.stage_bytes == 0 && live.size() == 34);
    fail_at = -1;
    CHECK(ap_stage(&e, 1 << 20) == 0 && e.stage_bytes == (1 << 20) && owns_exactly_live(e.own));
    e.stage[(1 << 20) - 1] = 1;
    ap_close(&e);
    CHECK(live.empty() && ap_all_null(e));
    ap_close(&e);
}

// ---- the companions' handles, each fresh from the device-free half of its create (no memory yet), as a create makes them: the
// buffers, n_want of them and bytes_want in all; the close, twice; a failure at every allocation; what a destroy does
template <typename H>
void check_companion(const std::function<H *()> &fresh, int (*buffers)(H *), DevOwner &(*owner)(H *), void (*free_handle)(H *), int n_want,
                     size_t bytes_want) {
    H *h = fresh();
    CHECK(h && live.empty() && owner(h).allocs.empty());
    fail_at = -1, n_alloc = 0, n_bytes = 0;
    CHECK(buffers(h) == 0 && n_alloc == n_want && n_bytes == bytes_want && (int)live.size() == n_want && owns_exactly_live(owner(h)));
    y355_dev_release_all(owner(h));
    CHECK(live.empty() && owner(h).allocs.empty());
    free_handle(h);                                 // (a second release: harmless)
    for (int k = 0; k < n_want; ++k) {              // the k-th allocation fails: what was taken goes back, the message stays
        h = fresh();
        fail_at = k, n_alloc = 0, g_err.clear();
        CHECK(buffers(h) == Y355_EHIP && live.empty() && owner(h).allocs.empty() && g_err == "injected allocation failure");
        fail_at = -1;
        free_handle(h);
    }
    h = fresh();
    CHECK(buffers(h) == 0 && (int)live.size() == n_want && owns_exactly_live(owner(h)));
    free_handle(h);
    CHECK(live.empty());
}
void check_loss(int levels) {
    const int A = 2, mb = 2, ml = 2, hs[3] = {levels == 1 ? 2 : 4, 2, 1};
    y355_loss_config cfg;
    CHECK(y355_loss_default_config(&cfg) == 0);
    cfg.num_levels = levels, cfg.num_anchors = A, cfg.num_classes = 2, cfg.in_h = cfg.in_w = 64, cfg.max_batch = mb, cfg.max_labels_per_image = ml;
    size_t N = 0;
    for (int l = 0; l < levels; ++l) cfg.hs[l] = cfg.ws[l] = hs[l], cfg.stride[l] = 64 / hs[l], N += (size_t)hs[l] * hs[l] * A;
    for (int i = 0; i < 2 * levels * A; ++i) cfg.anchors[i] = 1.5 + i;
    y355_loss *h = nullptr;
    CHECK(loss_open(nullptr, host_mem(), &h) == Y355_EINVAL && g_err == "y355_loss_create: null argument");
    cfg.num_levels = 4;
    CHECK(loss_open(&cfg, host_mem(), &h) == Y355_EINVAL && !h && g_err == "num_levels must be 1..3" && live.empty());
    cfg.num_levels = levels;
    const std::function<y355_loss *()> fresh = [&cfg, N] {
        y355_loss *h = nullptr;
        CHECK(loss_open(&cfg, host_mem(), &h) == 0 && y355_loss_num_anchors_total(h) == (int)N);
        return h;
    };
    // target, labels, offsets, partial (one workgroup per image at these sizes), per_image, out
    check_companion(fresh, loss_buffers, loss_owner, loss_free, 6, mb * N * 11 * 4 + mb * ml * 5 * 8 + (mb + 1) * 4 + mb * 5 * 8 + mb * 5 * 8 + 4 * 8);
}
void check_anchors(int64_t max_boxes) {
    const size_t R = 2, nb = (size_t)max_boxes, chunks = (nb + Y355_ANCHORS_CHUNK - 1) / Y355_ANCHORS_CHUNK;
    const size_t MR = Y355_ANCHORS_MAX_RESTARTS, MK = Y355_ANCHORS_MAX_K;
    y355_anchors *h = nullptr;
    CHECK(anchors_open(0, max_boxes, 65, 3, host_mem(), &h) == Y355_EINVAL && !h && g_err == "max_restarts must be 1..64" && live.empty());
    const std::function<y355_anchors *()> fresh = [max_boxes] {
        y355_anchors *h = nullptr;
        CHECK(anchors_open(0, max_boxes, (int)R, 3, host_mem(), &h) == 0 && y355_anchors_num_boxes(h) == 0);
        return h;
    };
    // boxes, groups, score_idx, partial; cent, init; loss, old_loss; iters, done, nfound, first; u; score_anchors, score_out; counts,
    // init_index; flag
    const size_t bytes = nb * 16 + R * nb + nb + R * (3 * MK + 1) * chunks * 8 + 2 * (MR * MK * 2 * 8) + 2 * MR * 8 + 4 * MR * 4 + MR * (MK - 1) * 8 +
                         MK * 2 * 8 + (1 + MK) * 8 + 2 * (MR * MK * 4) + 4;
    check_companion(fresh, anchors_buffers, anchors_owner, anchors_free, 18, bytes);
}

// ---- a pipeline slot's outputs: all four or none
void check_slot() {
    DevOwner o{host_mem(), {}};
    Slot s;
    for (int k = 0; k < 4; ++k) {
        fail_at = k, n_alloc = 0;
        CHECK(y355_slot_outputs(s, o, 2, 100) == Y355_EHIP && !s.boxes && !s.scores && !s.cls && !s.count && live.empty() && o.allocs.empty());
    }
    fail_at = -1, n_alloc = 0;
    CHECK(y355_slot_outputs(s, o, 2, 100) == 0 && s.boxes && s.scores && s.cls && s.count && n_alloc == 4 && owns_exactly_live(o));
    s.boxes[799] = 1.f, s.scores[199] = 1.f, s.cls[199] = 1, s.count[1] = 1;
    CHECK(y355_slot_outputs(s, o, 2, 100) == 0 && n_alloc == 4);          // there already
    CHECK(y355_dev_get(o, &s.ovf, 2) == 0 && live.size() == 5);
    y355_slot_drop_outputs(s, o);
    CHECK(!s.boxes && !s.scores && !s.cls && !s.count && s.ovf && live.size() == 1);
    CHECK(y355_slot_outputs(s, o, 2, 50) == 0 && live.size() == 5);
    y355_dev_release_all(o);
    CHECK(live.empty());
}

// ---- a convolution operator's device memory (conv_op_state.h): create-time buffers, the weight swap, the workspaces and the
// geometry each was last zeroed for, the close
std::vector<uintptr_t> snapshot(const ConvOpMem &m) {
    const void *ptrs[] = {m.w_dev, m.bias_dev, m.bw_dev, m.flag_dev, m.bt_dev, m.ctr_dev, m.in_dev, m.out_dev, m.res_dev};
    std::vector<uintptr_t> v;
    for (const void *p : ptrs) v.push_back((uintptr_t)p);
    for (size_t x : {(size_t)m.w_kid, (size_t)m.w_cout_pad, m.in_cap, m.out_cap, m.res_cap, m.in_geo, m.out_geo, m.res_geo}) v.push_back(x);
    for (void *p : m.own.allocs) v.push_back((uintptr_t)p);
    return v;
}
// one forward of the 24 -> 40 channel 3x3 operator of tests/ops_parent_cases.py: 64-byte input pixels, the padded width of the
// tile its map selects
struct OpStep {
    int B, H, W, cout_pad;
    bool res, fp32;
    size_t geo() const { return ((size_t)B << 40) ^ ((size_t)H << 20) ^ (size_t)W ^ ((size_t)fp32 << 62) ^ ((size_t)1 << 61); }
    size_t in_bytes() const { return (size_t)B * (H + 2) * (W + 2) * 64; }
    size_t out_bytes() const { return (size_t)B * (H + 2) * (W + 2) * cout_pad * (fp32 ? 4 : 2); }
};
int op_step(ConvOpMem &m, const OpStep &s, ConvOpZero *z) {
    return y355_convop_workspaces(m, s.geo(), s.in_bytes(), s.out_bytes(), true, s.res ? s.out_bytes() : 0, z);
}
void check_conv_op() {
    ConvOpMem m;
    m.own.mem = host_mem();
    // create-time buffers: all or none
    for (int cout_pad : {0, 48}) {
        const int n_create = cout_pad ? 3 : 1;
        for (int k = 0; k < n_create; ++k) {
            fail_at = k, n_alloc = 0;
            CHECK(y355_convop_create_i8(m, cout_pad) == Y355_EHIP && live.empty() && m.own.allocs.empty());
            CHECK(!m.flag_dev && !m.bt_dev && !m.ctr_dev);
        }
        fail_at = -1, n_alloc = 0;
        CHECK(y355_convop_create_i8(m, cout_pad) == 0 && n_alloc == n_create && (int)live.size() == n_create && owns_exactly_live(m.own));
        CHECK(m.flag_dev && (m.bt_dev != nullptr) == (cout_pad != 0) && (m.ctr_dev != nullptr) == (cout_pad != 0));
        m.flag_dev[3] = 1u;
        if (cout_pad) m.bt_dev[cout_pad - 1] = 1, m.ctr_dev->guard = 1;
        y355_convop_close(m);
        CHECK(live.empty() && snapshot(m) == snapshot(ConvOpMem{}));
    }
    // the weight swap, int8 (room for the 64-bit biases) and bf16 (the fp32 biases): a failure at every allocation and at an
    // upload leaves the pointers, the key and the memory as they were -- nothing packed at first, then the first tile's
    const std::vector<char> pk1(100, 1), pk2(300, 2);
    const std::vector<float> b1(48, 1.f), b2(64, 2.f);
    for (bool bf16 : {false, true}) {
        CHECK(y355_convop_create_i8(m, 48) == 0);
        const struct { int kid, cout_pad; const std::vector<char> *pk; const float *bias; } swaps[] = {{3, 48, &pk1, b1.data()}, {5, 64, &pk2, b2.data()}};
        for (const auto &sw : swaps) {
            m.in_geo = m.out_geo = m.res_geo = 7;
            const std::vector<uintptr_t> before = snapshot(m);
            const std::set<void *> live_before = live;
            for (int k = 0; k < 3; ++k) {               // k = 2: the upload
                fail_at = k < 2 ? k : -1, fail_upload = k == 2, n_alloc = 0;
                CHECK(y355_convop_swap_weights(m, sw.kid, sw.cout_pad, *sw.pk, bf16 ? sw.bias : nullptr, nullptr) == Y355_EHIP);
                CHECK(snapshot(m) == before && live == live_before);
            }
            fail_at = -1, fail_upload = false, n_alloc = 0;
            CHECK(y355_convop_swap_weights(m, sw.kid, sw.cout_pad, *sw.pk, bf16 ? sw.bias : nullptr, nullptr) == 0 && n_alloc == 2);
            CHECK(m.w_kid == sw.kid && m.w_cout_pad == sw.cout_pad && memcmp(m.w_dev, sw.pk->data(), sw.pk->size()) == 0);
            CHECK(bf16 ? m.bias_dev && !m.bw_dev && m.bias_dev[sw.cout_pad - 1] == sw.bias[0] : m.bw_dev && !m.bias_dev);
            if (!bf16) m.bw_dev[sw.cout_pad - 1] = 1;
            CHECK(m.in_geo == 7 && m.out_geo == 0 && m.res_geo == 0);     // the padded width changed: out and res are zeroed again
            CHECK(live.size() == 5 && owns_exactly_live(m.own));
        }
        y355_convop_close(m);
        CHECK(live.empty());
    }
    // the workspaces on one operator object: a map, a smaller map (another tile: a swap in between), the first map again at a
    // larger batch, with and without a residual, bf16 and fp32 output.  `zeroed` is this check's own record of the geometry
    // each buffer was last reported for; what a step has to report follows from it and from the sizes alone.
    const OpStep steps[] = {{2, 14, 27, 64, true, false},  {1, 9, 11, 48, false, false}, {1, 9, 11, 48, true, false}, {3, 14, 27, 64, false, false},
                            {3, 14, 27, 64, true, false},  {3, 14, 27, 64, false, true}, {1, 9, 11, 48, false, true}, {1, 9, 11, 48, false, false},
                            {2, 14, 27, 64, false, false}, {2, 14, 27, 64, true, false}, {2, 14, 27, 64, true, false}};
    size_t zeroed[3] = {0, 0, 0}, cap[3] = {0, 0, 0};
    for (const OpStep &s : steps) {
        if (m.w_cout_pad != s.cout_pad) {
            CHECK(y355_convop_swap_weights(m, s.cout_pad, s.cout_pad, pk1, b2.data(), nullptr) == 0);
            zeroed[1] = zeroed[2] = 0;
        }
        const size_t need[3] = {s.in_bytes(), s.out_bytes(), s.res ? s.out_bytes() : 0};
        bool want[3];
        for (int i = 0; i < 3; ++i) {
            if (need[i] > cap[i]) cap[i] = need[i], zeroed[i] = 0;      // new memory
            want[i] = need[i] && zeroed[i] != s.geo();
        }
        // the step with its k-th allocation failing, k = 0, 1, ...: the first k it does not reach is the step itself, and
        // reports what it would have reported without the failures before it
        ConvOpZero z;
        bool done = false;
        for (int k = 0; k <= 3 && !done; ++k) {
            const size_t geos[3] = {m.in_geo, m.out_geo, m.res_geo};
            const char *ptrs[3] = {m.in_dev, m.out_dev, m.res_dev};
            fail_at = k, n_alloc = 0;
            done = op_step(m, s, &z) == 0;
            CHECK(owns_exactly_live(m.own) && (done ? n_alloc <= k : g_err == "injected allocation failure"));
            CHECK(!m.in_dev == (m.in_cap == 0) && !m.out_dev == (m.out_cap == 0) && !m.res_dev == (m.res_cap == 0));
            // a recorded geometry changes in one way before the zeroing is enqueued: to "none", with the memory
            CHECK((m.in_geo == geos[0] && m.in_dev == ptrs[0]) || m.in_geo == 0);
            CHECK((m.out_geo == geos[1] && m.out_dev == ptrs[1]) || m.out_geo == 0);
            CHECK((m.res_geo == geos[2] && m.res_dev == ptrs[2]) || m.res_geo == 0);
        }
        fail_at = -1;
        CHECK(done && z.in == want[0] && z.out == want[1] && z.res == want[2]);
        CHECK(m.in_cap >= need[0] && m.out_cap >= need[1] && m.res_cap >= need[2]);
        m.in_dev[need[0] - 1] = 1, m.out_dev[need[1] - 1] = 1;        // (the sanitizer sees a buffer that is too short)
        if (s.res) m.res_dev[need[2] - 1] = 1;
        y355_convop_zeroed(m, s.geo(), z);
        for (int i = 0; i < 3; ++i)
            if (want[i]) zeroed[i] = s.geo();
        CHECK(m.in_geo == s.geo() && m.out_geo == s.geo() && (!s.res || m.res_geo == s.geo()));
        CHECK(op_step(m, s, &z) == 0 && !z.in && !z.out && !z.res);     // the same call again: nothing to zero
    }
    y355_convop_close(m);
    CHECK(live.empty());
    // in fits, out must grow and fails; then the same call again: in was not zeroed for the new geometry, and is reported
    {
        const OpStep a{1, 9, 11, 48, false, false}, b{1, 7, 9, 192, false, false};
        ConvOpZero z;
        CHECK(b.in_bytes() < a.in_bytes() && b.out_bytes() > a.out_bytes());
        CHECK(op_step(m, a, &z) == 0 && z.in && z.out && !z.res);
        y355_convop_zeroed(m, a.geo(), z);
        const char *in_a = m.in_dev;
        fail_at = 0, n_alloc = 0;
        CHECK(op_step(m, b, &z) == Y355_EHIP && n_alloc == 1 && m.in_dev == in_a && m.in_geo == a.geo() && !m.out_dev && m.out_geo == 0);
        fail_at = -1;
        CHECK(op_step(m, b, &z) == 0 && z.in && z.out && !z.res && m.in_dev == in_a && m.in_geo == a.geo());
        y355_convop_zeroed(m, b.geo(), z);
        CHECK(m.in_geo == b.geo() && m.out_geo == b.geo() && m.res_geo == 0);
        y355_convop_close(m);
    }
    // g1 with a residual, g2 without, g2 with: res is still in g1's layout, and is the one buffer reported
    {
        const OpStep g1r{2, 14, 27, 64, true, false}, g2{1, 9, 11, 64, false, false}, g2r{1, 9, 11, 64, true, false};
        ConvOpZero z;
        CHECK(op_step(m, g1r, &z) == 0 && z.in && z.out && z.res);
        y355_convop_zeroed(m, g1r.geo(), z);
        CHECK(op_step(m, g2, &z) == 0 && z.in && z.out && !z.res);
        y355_convop_zeroed(m, g2.geo(), z);
        CHECK(m.res_geo == g1r.geo());
        n_alloc = 0;
        CHECK(op_step(m, g2r, &z) == 0 && !z.in && !z.out && z.res && n_alloc == 0);
        y355_convop_zeroed(m, g2r.geo(), z);
        CHECK(m.res_geo == g2.geo() && live.size() == 3 && owns_exactly_live(m.own));
    }
    // an operator whose output has no halo to keep (int8 results, the general geometry): out is never reported
    {
        ConvOpZero z;
        CHECK(y355_convop_workspaces(m, 5, 10, 10, false, 0, &z) == 0 && z.in && !z.out && !z.res);
    }
    y355_convop_close(m);
    CHECK(live.empty() && m.own.allocs.empty() && snapshot(m) == snapshot(ConvOpMem{}));
    y355_convop_close(m);                           // a second close does nothing
    CHECK(live.empty());
}
}  // namespace

int main() {
    check_owner();
    check_conv_op();
    check_apeval_buffers(8);
    check_apeval_buffers(5000);                     // five tiles of the sort's histogram
    check_apeval_gt();
    check_coco();
    check_slot();
    check_loss(1);                                  // gt_creator's form
    check_loss(3);                                  // multi_gt_creator's
    check_anchors(1);                               // one chunk
    check_anchors(Y355_ANCHORS_CHUNK + 1);          // two
    check_head(2000, 2, 0, true, true);            // a small head: engine-like (tap and host outputs)
    check_head(2000, 1, 100, false, true);          // y355_head_f32_ex without the tap
    check_head(10647, 2, 0, true, false);           // more than 4096 anchors: y355_net-like (no host outputs)
    check_head(10647, 3, 5000, true, true);         // max_det between the two capacities
    check_stage();
    check_core(180, true);                          // engine-like: host outputs
    check_core(10647, false);                       // y355_net-like, more than 4096 anchors
    CHECK(y355_head_check_option(10647, true, 4096, "m") == 0 && y355_head_check_option(10647, true, 10647, "m") == 0);
    CHECK(y355_head_check_option(10647, true, 10648, "cap message") == Y355_EINVAL && g_err == "cap message");
    CHECK(y355_head_check_option(2000, true, 4096, "m") == 0 && y355_head_check_option(2000, true, 4097, "m") == Y355_EINVAL);
    CHECK(y355_head_check_option(2000, true, 2000, "m") == Y355_EINVAL);
    int e = 0;
    CHECK(y355_tracker_exponent(0.f, &e) == 1 && y355_tracker_exponent(-1.f, &e) == 1 && y355_tracker_exponent(INFINITY, &e) == 1);
    CHECK(y355_tracker_exponent(1.f, &e) == 0 && e == 0 && y355_tracker_exponent(0.75f, &e) == 0 && e == -1);
    CHECK(y355_tracker_exponent(1e-30f, &e) == 2 && y355_tracker_exponent(1e30f, &e) == 2 && y355_tracker_exponent(63.5f, &e) == 0 && e == 5);
    CHECK(y355_core_check_config(80, 96, 16, 5, 16, 2, 1, 150) == 0 && y355_core_check_config(80, 96, 32, 5, 16, 2, 1, 150) == Y355_EINVAL &&
          g_err == "input size must be a positive multiple of 32");
    CHECK(y355_head_check_option(2000, false, 1, "m") == 0 && y355_head_check_option(2000, false, 2, "route message") == Y355_EINVAL &&
          g_err == "route message");
    puts("host_state_check: ok");
    return 0;
}
