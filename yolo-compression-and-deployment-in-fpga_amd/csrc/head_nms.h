// yolo355 -- what the two NMS routes of the detection head share: the device view of the head workspace and the
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
