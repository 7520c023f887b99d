/* A plain C99 client of the y355_apeval_* part of include/yolo355.h.  Built and run by tests/test_voc_ap_ref.py: every entry
 * point is linked, and every argument check answers before any device work -- so this passes without a GPU.  Where a GPU is
 * present the last part also runs the checks that need a live handle. */
#include <stdio.h>
#include <string.h>
#include "yolo355.h"

#define EXPECT(expr, code, where)                                                       \
    do {                                                                                \
        int rc_ = (expr);                                                               \
        if (rc_ != (code)) { printf("%s: %d (%s)\n", where, rc_, y355_last_error()); return __LINE__; } \
    } while (0)

int main(void) {
    y355_apeval *e = (y355_apeval *)&e;      /* must be reset to NULL by a failing create */
    float f[8] = {0};
    int32_t i32[8] = {0};
    uint8_t u8[8] = {0};
    double d[8];
    int64_t i64[8];
    int rc;
    /* create: the ranges of the header */
    EXPECT(y355_apeval_create(0, 20, 10, 100, NULL), Y355_EINVAL, "create null out");
    EXPECT(y355_apeval_create(-1, 20, 10, 100, &e), Y355_EINVAL, "create device");
    if (e != NULL) return __LINE__;
    EXPECT(y355_apeval_create(0, 0, 10, 100, &e), Y355_EINVAL, "create classes 0");
    EXPECT(y355_apeval_create(0, 257, 10, 100, &e), Y355_EINVAL, "create classes 257");
    if (strstr(y355_last_error(), "num_classes") == NULL) return __LINE__;
    EXPECT(y355_apeval_create(0, 20, 0, 100, &e), Y355_EINVAL, "create images 0");
    EXPECT(y355_apeval_create(0, 20, (1 << 24) + 1, 100, &e), Y355_EINVAL, "create images 2^24 + 1");
    EXPECT(y355_apeval_create(0, 20, 10, 0, &e), Y355_EINVAL, "create max_dets 0");
    EXPECT(y355_apeval_create(0, 20, 10, ((int64_t)1 << 27) + 1, &e), Y355_EINVAL, "create max_dets 2^27 + 1");
    if (strstr(y355_last_error(), "max_dets") == NULL) return __LINE__;
    /* a null handle is rejected everywhere */
    y355_apeval_destroy(NULL);
    EXPECT(y355_apeval_set_gt(NULL, i32, f, i32, u8), Y355_EINVAL, "set_gt null");
    EXPECT(y355_apeval_add(NULL, 0, 1, 1, f, f, i32, i32, NULL), Y355_EINVAL, "add null");
    EXPECT(y355_apeval_add_host(NULL, 0, 1, 1, f, f, i32, i32), Y355_EINVAL, "add_host null");
    EXPECT(y355_apeval_reset(NULL), Y355_EINVAL, "reset null");
    EXPECT(y355_apeval_compute(NULL, 0.5, Y355_AP_VOC07, Y355_AP_Q_VOCFILE, d, i32, i64, d), Y355_EINVAL, "compute null");
    EXPECT(y355_apeval_curve(NULL, 0, 0, NULL, NULL, NULL, i64), Y355_EINVAL, "curve null");
    if (Y355_AP_VOC07 == Y355_AP_AREA || Y355_AP_Q_VOCFILE == Y355_AP_Q_NONE) return __LINE__;
    /* a valid create needs a GPU: without one it fails loudly as a HIP error and leaves no handle */
    rc = y355_apeval_create(0, 3, 4, 16, &e);
    if (rc != 0) {
        if (rc != Y355_EHIP || e != NULL || strlen(y355_last_error()) == 0) { printf("create: %d\n", rc); return __LINE__; }
        printf("ok apeval (no GPU)\n");
        return 0;
    }
    /* with a handle: the remaining checks, none of which launches anything */
    EXPECT(y355_apeval_compute(e, 0.5, Y355_AP_VOC07, Y355_AP_Q_VOCFILE, d, i32, i64, d), Y355_ENOTREADY, "compute without gt");
    EXPECT(y355_apeval_set_gt(e, NULL, f, i32, u8), Y355_EINVAL, "set_gt null offsets");
    i32[0] = 1;
    EXPECT(y355_apeval_set_gt(e, i32, f, i32, u8), Y355_EINVAL, "set_gt offsets[0]");
    i32[0] = 0; i32[1] = 1; i32[2] = 0;
    EXPECT(y355_apeval_set_gt(e, i32, f, i32, u8), Y355_EINVAL, "set_gt decreasing");
    {
        int32_t off[5] = {0, 1, 1, 2, 2}, cls[2] = {0, 3};
        EXPECT(y355_apeval_set_gt(e, off, f, cls, u8), Y355_EINVAL, "set_gt class");
        EXPECT(y355_apeval_set_gt(e, off, NULL, cls, u8), Y355_EINVAL, "set_gt null boxes");
        cls[1] = 2;
        EXPECT(y355_apeval_set_gt(e, off, f, cls, u8), 0, "set_gt");
    }
    EXPECT(y355_apeval_add(e, 0, 1, 1, NULL, f, i32, i32, NULL), Y355_EINVAL, "add null boxes");
    EXPECT(y355_apeval_add(e, -1, 1, 1, f, f, i32, i32, NULL), Y355_EINVAL, "add first_image");
    EXPECT(y355_apeval_add(e, 3, 2, 1, f, f, i32, i32, NULL), Y355_EINVAL, "add past the list");
    EXPECT(y355_apeval_add(e, 0, 0, 1, f, f, i32, i32, NULL), Y355_EINVAL, "add batch 0");
    EXPECT(y355_apeval_add(e, 0, 1, 0, f, f, i32, i32, NULL), Y355_EINVAL, "add max_det 0");
    EXPECT(y355_apeval_add_host(e, 0, 1, (1 << 20) + 1, f, f, i32, i32), Y355_EINVAL, "add_host max_det");
    EXPECT(y355_apeval_compute(e, 0.5, 2, Y355_AP_Q_VOCFILE, d, i32, i64, d), Y355_EINVAL, "compute metric");
    EXPECT(y355_apeval_compute(e, 0.5, Y355_AP_AREA, 2, d, i32, i64, d), Y355_EINVAL, "compute quantize");
    EXPECT(y355_apeval_compute(e, 0.5, Y355_AP_AREA, Y355_AP_Q_NONE, NULL, i32, i64, d), Y355_EINVAL, "compute null ap");
    EXPECT(y355_apeval_curve(e, 0, 0, NULL, NULL, NULL, i64), Y355_ENOTREADY, "curve before compute");
    EXPECT(y355_apeval_curve(e, 3, 0, NULL, NULL, NULL, i64), Y355_EINVAL, "curve class");
    EXPECT(y355_apeval_curve(e, 0, -1, NULL, NULL, NULL, i64), Y355_EINVAL, "curve capacity");
    EXPECT(y355_apeval_curve(e, 0, 0, NULL, NULL, NULL, NULL), Y355_EINVAL, "curve null n");
    EXPECT(y355_apeval_reset(e), 0, "reset");
    y355_apeval_destroy(e);
    printf("ok apeval\n");
    return 0;
}
