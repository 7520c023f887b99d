/*
 * yolo355_loss -- C ABI of the companion library libyolo355_loss.so: the reference's training targets and the forward
 * value of its losses on the GPU.
 *
 *   targets   tools.gt_creator (tools.py:132-253: one level, anchors in grid units) and tools.multi_gt_creator
 *             (tools.py:256-374: several levels, anchors in pixels)
 *   loss      decode_boxes + tools.iou_score + tools.loss with obj_loss_f='mse' (tools.py:377-435), i.e. the branch
 *             `trainable=True` of every model's forward (models/slim_yolo_v2.py:360-382, models/yolo_v2.py:212-232,
 *             models/tiny_yolo_v3.py:249-273, models/yolo_v3.py, models/yolo_v3_spp.py)
 *
 * No backward pass.  The library is independent of libyolo355.so (include/yolo355.h): it reads prediction maps as plain
 * fp32 NCHW device tensors.  All functions return 0 or a negative Y355_LOSS_E* code; y355_loss_last_error() gives the
 * message of the last failure on the calling thread.  Arguments are checked before any HIP call.  A handle is
 * single-threaded.
 */
#ifndef YOLO355_LOSS_H
#define YOLO355_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_LOSS_MAX_LEVELS 3
#define Y355_LOSS_MAX_ANCHORS 16       /* per level */
#define Y355_LOSS_TARGET_FIELDS 11     /* obj, cls, tx, ty, tw, th, weight, x1, y1, x2, y2 */

#define Y355_LOSS_OK 0
#define Y355_LOSS_EINVAL (-1)          /* bad argument */
#define Y355_LOSS_EHIP (-2)            /* HIP runtime error */
#define Y355_LOSS_ENOTREADY (-3)       /* no labels set for this batch */

typedef struct y355_loss y355_loss;

typedef struct y355_loss_config {
    int32_t device_id;
    int32_t num_levels;                              /* 1..3 */
    int32_t hs[Y355_LOSS_MAX_LEVELS];                /* grid rows / columns / stride of each level, in the head's order */
    int32_t ws[Y355_LOSS_MAX_LEVELS];
    int32_t stride[Y355_LOSS_MAX_LEVELS];
    int32_t num_anchors;                             /* A, per level */
    double anchors[2 * Y355_LOSS_MAX_LEVELS * Y355_LOSS_MAX_ANCHORS]; /* (w,h), level 0 first; the targets use them as they
                                                        are (float64, as the reference's lists), the decode as float32 */
    int32_t num_classes;                             /* C */
    int32_t in_h, in_w;                              /* network input size */
    float wh_mul;                                    /* decode: w = exp(tw) * anchor_w * wh_mul (stride: anchors in grid
                                                        units; 1: pixels) */
    int32_t anchors_in_grid_units;                   /* 1: gt_creator's form (one level only); 0: multi_gt_creator's */
    double ignore_thresh;                            /* data/config.py:33: 0.5 */
    double obj_weight, noobj_weight;                 /* tools.loss 'mse': 5, 1 */
    int32_t max_batch;
    int32_t max_labels_per_image;
} y355_loss_config;

const char *y355_loss_last_error(void);

/* zeroes *cfg and fills the defaults: ignore_thresh 0.5, obj / noobj weights 5 / 1, wh_mul 1, one level */
int y355_loss_default_config(y355_loss_config *cfg);

int y355_loss_create(const y355_loss_config *cfg, y355_loss **out);
void y355_loss_destroy(y355_loss *h);

/* N: anchors of an image, level 0 first, cell * A + a inside a level */
int y355_loss_num_anchors_total(const y355_loss *h);

/* Target assignment of a batch.  offsets[batch + 1]: image b owns labels offsets[b] .. offsets[b + 1] - 1 of
 * labels[n][5] = xmin, ymin, xmax, ymax, cls (float64; coordinates in [0, 1], cls in 0 .. C - 1, all finite: anything
 * else is Y355_LOSS_EINVAL before any device work).  Builds the handle's dense target tensor [batch][N][11] float32 on
 * the device: labels in list order, a later write to a slot wins, an "ignore" write sets fields 0 and 6 only, a cell
 * outside the grid is dropped.  Synchronous. */
int y355_loss_set_labels(y355_loss *h, const int32_t *offsets, const double *labels, int32_t batch);

/* the handle's target tensor of the last y355_loss_set_labels, [batch][N][11] float32, to the host */
int y355_loss_get_targets(y355_loss *h, int32_t batch, float *dst_host);

/* The four losses of a batch.  pred_dev[num_levels]: fp32 NCHW maps [batch][A * (5 + C)][hs][ws] on the device, channels
 * [obj x A | cls x A*C | txtytwth x A*4].  target_dev: a dense [batch][N][11] float32 tensor on the device, or NULL: the
 * handle's own (the batch of the last y355_loss_set_labels must equal `batch`).  out[4] = conf_loss, cls_loss,
 * txtytwth_loss, total_loss; per_image (or NULL) [batch][5] = pos, neg, cls, txty, twth.  Terms are the reference's fp32
 * operations, sums are float64 in a fixed order: the result is the same bit for bit from run to run, and an image's
 * five parts do not depend on the rest of the batch.  Runs on `stream` (a hipStream_t; NULL: the null stream) and
 * returns after it has finished. */
int y355_loss_compute(y355_loss *h, const void *const *pred_dev, const void *target_dev, int32_t batch, void *stream,
                      double *out, double *per_image);

/* tools.iou_score (tools.py:377-389): out_dev[i] = IoU of boxes_a_dev[i][4] and boxes_b_dev[i][4] (x1, y1, x2, y2, fp32, on the
 * device), the (tl < br) product included.  Asynchronous on `stream`. */
int y355_loss_iou_score(int32_t device_id, const void *boxes_a_dev, const void *boxes_b_dev, int64_t n, void *out_dev, void *stream);

/* tools.loss (tools.py:392-435, obj_loss_f='mse') on the tensors it takes itself, fp32 on the device: conf [batch][N], cls
 * [batch][N][C], txtytwth [batch][N][4], label [batch][N][8] = iou, obj, cls, tx, ty, tw, th, weight.  out / per_image and
 * the order of the sums as y355_loss_compute.  Returns after `stream` has finished. */
int y355_loss_flat(int32_t device_id, const void *conf_dev, const void *cls_dev, const void *txtytwth_dev, const void *label_dev,
                   int32_t batch, int32_t num_anchors_total, int32_t num_classes, double obj_weight, double noobj_weight, void *stream,
                   double *out, double *per_image);

#ifdef __cplusplus
}
#endif
#endif
