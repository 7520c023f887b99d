/* A plain C99 client of the COCO part of the y355_apeval_* block of include/yolo355.h.  Built and run by
 * tests/test_coco_ap_ref.py (and tests/test_coco_ap.py on a GPU): the entry points are linked, and every argument check answers
 * before any device work -- so this passes without a GPU.  Where a GPU is present it also runs the limits that need a live
 * handle and the known answers K1 .. K3 of the COCO contract. */
#include <stdio.h>
#include <string.h>
#include "yolo355.h"

#define EXPECT(expr, code, where)                                                       \
    do {                                                                                \
        int rc_ = (expr);                                                               \
        if (rc_ != (code)) { printf("%s: %d (%s)\n", where, rc_, y355_last_error()); return __LINE__; } \
    } while (0)

#define T 10
#define R 101
#define A 4
#define M 3
static double iou_thrs[T], rec_thrs[R], precision[T * R * A * M], recall[T * A * M], stats[12];
static const double area_rng[A * 2] = {0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10};
static const int32_t max_dets[M] = {1, 10, 100};

static double prec_at(int t, int r, int a, int m) { return precision[((t * R + r) * A + a) * M + m]; }   /* K = 1 */
static double rec_at(int t, int a, int m) { return recall[(t * A + a) * M + m]; }

/* one image, one category: ng boxes (x y w h, area, crowd), nd detections (x1 y1 x2 y2, score) */
static int run(y355_apeval *e, int ng, const double *box, const double *area, const uint8_t *crowd, int nd, const float *det,
               const float *score) {
    int32_t off[2], cls[4] = {0, 0, 0, 0}, count[1];
    off[0] = 0; off[1] = ng; count[0] = nd;
    EXPECT(y355_apeval_set_gt_coco(e, off, box, area, cls, crowd, NULL), 0, "set_gt_coco");
    EXPECT(y355_apeval_reset(e), 0, "reset");
    EXPECT(y355_apeval_add_host(e, 0, 1, nd, det, score, cls, count), 0, "add_host");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), 0, "compute_coco");
    return 0;
}

int main(void) {
    y355_apeval *e = NULL;
    const double p = 1.0 / (1.0 + 2.220446049250313e-16);
    int32_t i32[8] = {0};
    int64_t i64[2];
    int rc, t, r, line;
    for (t = 0; t < T; ++t) iou_thrs[t] = 0.5 + 0.05 * t;
    for (r = 0; r < R; ++r) rec_thrs[r] = r / 100.0;
    /* a null handle is rejected everywhere, before anything else is looked at */
    EXPECT(y355_apeval_set_gt_coco(NULL, i32, precision, precision, i32, (const uint8_t *)i32, NULL), Y355_EINVAL, "set_gt_coco null");
    EXPECT(y355_apeval_compute_coco(NULL, iou_thrs, T, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), Y355_EINVAL,
           "compute_coco null");
    EXPECT(y355_apeval_coco_matches(NULL, 0, 0, 0, 0, 0, i64, i64 + 1, NULL, NULL, NULL, NULL), Y355_EINVAL, "coco_matches null");
    rc = y355_apeval_create(0, 1, 1, 16, &e);
    if (rc != 0) {
        if (rc != Y355_EHIP || e != NULL) { printf("create: %d\n", rc); return __LINE__; }
        printf("ok cocoeval (no GPU)\n");
        return 0;
    }
    /* the limits and the order of the calls */
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), Y355_ENOTREADY,
           "compute_coco without gt");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, 17, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), Y355_EINVAL, "T 17");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, 1025, area_rng, A, max_dets, M, precision, recall, stats), Y355_EINVAL, "R 1025");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, 9, max_dets, M, precision, recall, stats), Y355_EINVAL, "A 9");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, max_dets, 9, precision, recall, stats), Y355_EINVAL, "M 9");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, 0, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), Y355_EINVAL, "T 0");
    i32[0] = 10; i32[1] = 1; i32[2] = 100;
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, i32, M, precision, recall, stats), Y355_EINVAL, "max_dets order");
    i32[0] = 1; i32[1] = 10; i32[2] = (1 << 20) + 1;
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, i32, M, precision, recall, stats), Y355_EINVAL, "max_dets 2^20 + 1");
    EXPECT(y355_apeval_compute_coco(e, NULL, T, rec_thrs, R, area_rng, A, max_dets, M, precision, recall, stats), Y355_EINVAL, "null iou_thrs");
    EXPECT(y355_apeval_compute_coco(e, iou_thrs, T, rec_thrs, R, area_rng, A, max_dets, M, NULL, recall, stats), Y355_EINVAL, "null precision");
    EXPECT(y355_apeval_coco_matches(e, 0, 0, 0, 0, 0, i64, i64 + 1, NULL, NULL, NULL, NULL), Y355_ENOTREADY, "coco_matches before compute");
    EXPECT(y355_apeval_coco_matches(e, 1, 0, 0, 0, 0, i64, i64 + 1, NULL, NULL, NULL, NULL), Y355_EINVAL, "coco_matches image");
    EXPECT(y355_apeval_coco_matches(e, 0, 0, 0, 0, 0, NULL, i64 + 1, NULL, NULL, NULL, NULL), Y355_EINVAL, "coco_matches null count");
    i32[0] = 0; i32[1] = 1;
    EXPECT(y355_apeval_set_gt_coco(e, NULL, precision, precision, i32, (const uint8_t *)i32, NULL), Y355_EINVAL, "set_gt_coco null offsets");
    EXPECT(y355_apeval_set_gt_coco(e, i32, NULL, precision, i32, (const uint8_t *)i32, NULL), Y355_EINVAL, "set_gt_coco null boxes");
    EXPECT(y355_apeval_set_gt_coco(e, i32, precision, precision, i32 + 1, (const uint8_t *)i32, NULL), Y355_EINVAL, "set_gt_coco class");
    EXPECT(y355_apeval_set_gt_coco(e, i32, precision, precision, i32, (const uint8_t *)i32, i32 + 1), Y355_EINVAL, "set_gt_coco rank");
    {   /* K1: one box, one detection of IoU 2500 / 2500: precision p everywhere in the all and medium ranges, recall 1 */
        const double box[4] = {10, 10, 50, 50}, area[1] = {2500};
        const uint8_t crowd[1] = {0};
        const float det[4] = {10, 10, 60, 60}, score[1] = {0.9f};
        int a, m;
        if ((line = run(e, 1, box, area, crowd, 1, det, score)) != 0) return line;
        for (t = 0; t < T; ++t)
            for (a = 0; a < A; ++a)
                for (m = 0; m < M; ++m) {
                    const int in = a == 0 || a == 2;
                    if (rec_at(t, a, m) != (in ? 1.0 : -1.0)) return __LINE__;
                    for (r = 0; r < R; ++r)
                        if (prec_at(t, r, a, m) != (in ? p : -1.0)) return __LINE__;
                }
        if (stats[3] != -1 || stats[5] != -1 || stats[9] != -1 || stats[11] != -1 || stats[6] != 1 || stats[7] != 1 || stats[8] != 1 ||
            stats[10] != 1)
            return __LINE__;
        if (stats[0] < p - 1010 * 2.3e-16 || stats[0] > p + 1010 * 2.3e-16 || stats[1] < p - 101 * 2.3e-16 || stats[1] > p + 101 * 2.3e-16 ||
            stats[2] != stats[1] || stats[4] != stats[0])
            return __LINE__;
    }
    {   /* K2: a second box nobody finds and a false positive: p at the 51 recall points <= 0.5, 0 above; AR 0.5 */
        const double box[8] = {10, 10, 50, 50, 200, 200, 50, 50}, area[2] = {2500, 2500};
        const uint8_t crowd[2] = {0, 0};
        const float det[8] = {10, 10, 60, 60, 300, 10, 340, 50}, score[2] = {0.9f, 0.8f};
        if ((line = run(e, 2, box, area, crowd, 2, det, score)) != 0) return line;
        for (t = 0; t < T; ++t) {
            if (rec_at(t, 0, 0) != 0.5 || rec_at(t, 0, 2) != 0.5) return __LINE__;
            for (r = 0; r < R; ++r)
                if (prec_at(t, r, 0, 2) != (r <= 50 ? p : 0.0)) return __LINE__;
        }
        if (stats[6] != 0.5 || stats[7] != 0.5 || stats[8] != 0.5) return __LINE__;
        if (stats[0] < 51 * p / 101 - 1010 * 2.3e-16 || stats[0] > 51 * p / 101 + 1010 * 2.3e-16 || stats[1] != stats[2]) return __LINE__;
    }
    {   /* K3: a crowd box absorbs two detections, the better-scored of which comes first: AR@1 = 0, AR@10 = AR@100 = 1 */
        const double box[8] = {10, 10, 50, 50, 100, 100, 200, 200}, area[2] = {2500, 40000};
        const uint8_t crowd[2] = {0, 1};
        const float det[12] = {10, 10, 60, 60, 120, 120, 160, 160, 150, 150, 190, 190}, score[3] = {0.9f, 0.95f, 0.5f};
        int32_t pos[3], dtm[T * 3];
        uint8_t ig[T * 3], marked[T * 2];
        if ((line = run(e, 2, box, area, crowd, 3, det, score)) != 0) return line;
        if (stats[6] != 0 || stats[7] != 1 || stats[8] != 1) return __LINE__;
        for (t = 0; t < T; ++t)
            for (r = 0; r < R; ++r)
                if (prec_at(t, r, 0, 2) != p) return __LINE__;
        EXPECT(y355_apeval_coco_matches(e, 0, 0, 0, 3, 2, i64, i64 + 1, pos, dtm, ig, marked), 0, "coco_matches");
        if (i64[0] != 3 || i64[1] != 2 || pos[0] != 1 || pos[1] != 0 || pos[2] != 2) return __LINE__;
        for (t = 0; t < T; ++t)
            if (dtm[3 * t] != 1 || dtm[3 * t + 1] != 0 || dtm[3 * t + 2] != 1 || ig[3 * t] != 1 || ig[3 * t + 1] != 0 || ig[3 * t + 2] != 1 ||
                marked[2 * t] != 1 || marked[2 * t + 1] != 1)
                return __LINE__;
        EXPECT(y355_apeval_coco_matches(e, 0, 0, 4, 3, 2, i64, i64 + 1, pos, dtm, ig, marked), Y355_EINVAL, "coco_matches area index");
        EXPECT(y355_apeval_reset(e), 0, "reset");
        EXPECT(y355_apeval_coco_matches(e, 0, 0, 0, 3, 2, i64, i64 + 1, pos, dtm, ig, marked), Y355_ENOTREADY, "coco_matches after reset");
    }
    y355_apeval_destroy(e);
    printf("ok cocoeval\n");
    return 0;
}
