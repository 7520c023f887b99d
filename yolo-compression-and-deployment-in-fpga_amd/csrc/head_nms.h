// yolo355 -- what the two NMS routes of the detection head share: the head workspace (HeadWork, the kernels' argument), the
// host state that owns it (HeadState, head_state.hip: one per y355_engine, y355_net and y355_head_f32_ex call) and the
// reference's suppression predicate.  head_nms.hip: decode, and the route for images with at most Y355_NMS_CAP candidates
// (bin sort, pruned pair walk, rounds); nms_large.hip: the route for more (radix sort, block-greedy resolve).
#pragma once
#include "y355_common.h"

struct HeadWork {
    float *cbox;          // [B][CAP][4]  compacted candidates, (anchor, bin) order
    float *cscore;        // [B][CAP]
    int *ccls;            // [B][CAP]
    int *corig;           // [B][CAP]     anchor index n = cell*A + a of compact position p
    int *count;           // [B]          candidates per image
    unsigned int *edges;  // [B][EDGE_CAP] suppressing pairs (p << 12) | q with p < q (compact positions)
    int *nedges;          // [B][2]        number of edges; overflow flag (a list did not fit)
    int *binstart;        // [B][CAP+8]   first compact position of bin (a*HW + by*Ws + bx)
    float *astat;         // [B][MAXG][4] per candidate group: wmax, hmax, amin, amax (clamped boxes)
    int *tiny;            // [B][CAP]     positions of candidates with area < AREA_MIN
    int *ntiny;           // [B]
    int *ctype;           // [B][CAP]     candidate group of compact position p
    float *dbox;          // [B][CAP][4]  decode of every anchor, (level, anchor, cell) order
    float *dscore;        // [B][CAP]
    int *dcls;            // [B][CAP]
    // heads with more than CAP anchors per image (three-level models at 416 x 416): decode_kernel writes the raw arrays
    // (pitch rstride), compact_kernel keeps the anchors at or above conf_thresh in anchor-index order in dbox / dscore /
    // dcls (at most CAP of them; more sets ovf[b]); the sort then sees an ordinary <= CAP-anchor image
    float *rbox;          // [B][rstride][4] or null (= small head: decode writes dbox directly)
    float *rscore;        // [B][rstride]
    int *rcls;            // [B][rstride]
    int *rcount;          // [B] anchors kept by the compaction that the small route takes (0: the image went to the large route)
    int *ovf;             // [B] 1: more anchors than the candidate capacity passed the threshold (the rest were dropped)
    int rstride;
    unsigned long long *stamps;   // diagnostics or null
    // large route (nms_large.hip): set only when the candidate capacity lcap is above CAP or the route is forced.
    // compact_large_kernel keeps up to lcap anchors in anchor-index order; an image's position in that list is its rank
    float *lbox;          // [B][lcap][4]
    float *lscore;        // [B][lcap]
    int *lcls;            // [B][lcap]
    int *lcount;          // [B] candidates of an image the large route takes (0: the image went to the small route)
    uint2 *lsort;         // [2][B][lcap] ping-pong of the radix sort: (~score bits, class << 16 | rank)
    float *lkbox;         // [B][lcap][4] boxes kept so far, per class segment of the sorted list
    unsigned char *lkeep; // [B][lcap] 1: rank survives
    int lcap;
    int lforce;           // 1: every image takes the large route
};

// ---- host state of one detection head: the workspace, its sizes, the candidate tap and the host calls' outputs
struct HeadState {
    HeadWork wk{};            // every array of the head; lcap, lforce, stamps (and rbox: null for a small head on the automatic
                              // route) are the launcher's to set per launch
    int N = 0, max_batch = 0; // anchors per image, images per forward
    int cfg_max_det = 0;      // what the configuration asked for (<= 0: no limit)
    int max_det = 0;          // per-image cap of the returned detections: cfg_max_det within the candidates an image can have
    int cap = 0, route = 0;   // candidate capacity (read it through y355_head_capacity) and Y355_HEAD_ROUTE_*
    float *cand_box = nullptr, *cand_score = nullptr;   // [B][N][4], [B][N] tap of every anchor's decode, or null: no tap
    int *cand_cls = nullptr;
    float *o_box = nullptr, *o_score = nullptr;         // [B][max_det][4], [B][max_det] outputs of the host calls, or null
    int *o_cls = nullptr, *o_count = nullptr;
    DevOwner own;             // every array above
};
inline int y355_head_capacity(const HeadState &st) { return st.cap ? st.cap : Y355_NMS_CAP; }
// Allocates everything a head of N anchors per image and B images needs at capacity `cap` and `route`; a failure (non-zero,
// the allocator's message) frees what it took.
int y355_head_create(HeadState &st, int N, int B, int cfg_max_det, int cap, int route, bool want_tap, bool want_host_outputs,
                     const DevMem &mem);
void y355_head_destroy(HeadState &st);
// Another capacity / route: the raw decode arrays (N > Y355_NMS_CAP, or the large route forced), the large route's lists
// (cap > Y355_NMS_CAP, or forced) and the host calls' outputs at the new max_det.  Everything new is allocated first, then
// swapped in: a failure (non-zero) leaves st as it was.  The caller has synchronised the stream the head runs on.
int y355_head_resize(HeadState &st, int cap, int route);
// the range of a capacity (is_cap) or route value for a head of N anchors; 0, or Y355_EINVAL with the caller's message
int y355_head_check_option(int N, bool is_cap, int value, const char *msg);
// a checked option value -> y355_head_resize (the other of the two stays)
inline int y355_head_set_option(HeadState &st, bool is_cap, int value) {
    return y355_head_resize(st, is_cap ? value : y355_head_capacity(st), is_cap ? st.route : value);
}
// Heads that have the flags (st.wk.ovf: more than Y355_NMS_CAP anchors, or the large route forced).  read: *overflow = 1 if,
// in a forward since the last call, more anchors of an image passed conf_thresh than the capacity holds; waits for s; clears.
// take: the flags move to dst_dev [max_batch] on s and are cleared behind the copy (pipeline.hip: a ticket's own overflow)
hipError_t y355_head_overflow_read(const HeadState &st, hipStream_t s, int *overflow);
hipError_t y355_head_overflow_take(const HeadState &st, int *dst_dev, hipStream_t s);
// the candidate tap of the last Y355_F_TAP forward / candidates and suppressing pairs per image (count[batch],
// nedges[2 * batch]: list length, overflow / abort flag) of the last forward's NMS, to the host; both wait for s
hipError_t y355_head_get_candidates(const HeadState &st, hipStream_t s, int batch, float *boxes, float *scores, int32_t *cls);
hipError_t y355_head_debug_counts(const HeadState &st, hipStream_t s, int batch, int32_t *count, int32_t *nedges);
// What every caller's HeadParams has in common: sizes, thresholds, the tap (only with `tap`: Y355_F_TAP), max_det, outputs.
// The levels, A, C, wh_mul, the grouping and pairs_wgs are the caller's.
void y355_head_fill(HeadParams &p, const HeadState &st, float conf_thresh, float nms_thresh, int in_h, int in_w, float *out_box,
                    float *out_score, int *out_cls, int *out_count, bool tap);
// candidates grouped by area octave: bins on a grid of at most 16 x 16 over level 0's Hs x Ws cells
inline void y355_head_area_bins(HeadParams &p, int Hs, int Ws) {
    p.group_by_area = 1;
    p.Hb = Hs < 16 ? Hs : 16;
    p.Wb = Ws < 16 ? Ws : 16;
}
// channels of a prediction map's buffer for A * (5 + C) real ones
inline int y355_pred_channels(int predc) { return predc <= 64 ? 64 : predc <= 128 ? 128 : 256; }
int y355_prepare_head(void);
// decode, candidate sort, pruned pair walk (edge list), rounds + output.  `mid` (optional) is recorded
// between the candidate sort and the pair walk.
// `kev` (optional): start / end events of the four launches decode, candidate sort, pair walk, rounds + output
void y355_launch_head_nms(const HeadParams &p, int batch, const HeadState &st, hipStream_t s, hipEvent_t mid,
                          hipEvent_t (*kev)[2] = nullptr);

// ---- the reference's suppression test (slim_yolo_v2.py:159-171), same class assumed
__device__ __forceinline__ bool suppresses_exact(const float4 a, float area_a, const float4 c, float area_c, float thr) {
    const float xx1 = fmaxf(a.x, c.x), yy1 = fmaxf(a.y, c.y);
    const float xx2 = fminf(a.z, c.z), yy2 = fminf(a.w, c.w);
    const float w = fmaxf(1e-28f, xx2 - xx1), h = fmaxf(1e-28f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = inter / (area_a + area_c - inter);
    return !(ovr <= thr);
}

// nms_large.hip.  compact: after decode_kernel wrote the raw arrays, instead of compact_kernel; nms: after resolve_emit_kernel
void y355_launch_compact_large(const HeadParams &p, const HeadWork &wk, int batch, hipStream_t s);
void y355_launch_nms_large(const HeadParams &p, const HeadWork &wk, int batch, hipStream_t s);
