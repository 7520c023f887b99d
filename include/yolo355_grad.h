/*
 * yolo355_grad -- C ABI of the companion library libyolo355_grad.so: the reference's four training losses TOGETHER WITH
 * their gradient with respect to the prediction maps, on the GPU.  The first link of a backward pass: everything behind it
 * is a convolution network that the caller's own framework differentiates.
 *
 *   value      what y355_loss_compute (include/yolo355_loss.h) returns for the same input, bit for bit
 *   gradient   of tools.loss with obj_loss_f='mse' (tools.py:392-435, MSELoss :27-42).  The IoU that serves as the
 *              objectness label is a constant, as the models take it under torch.no_grad() (models/slim_yolo_v2.py:362-364).
 *
 * Per anchor, with s = sigmoid(conf), mask = [weight > 0], pos = [obj == 1], neg = [obj == 0], upstream gradients
 * u_conf, u_cls, u_box, u_tot and k_x = (u_x + u_tot) / batch (fp32, computed once, the LAST factor of an element):
 *
 *   d conf   = ((obj_w * pos) * (2 (s - iou)) + (noobj_w * neg) * (2 s)) * (s (1 - s))   * k_conf
 *   d cls[c] = ((softmax(cls)[c] - [c == t_cls]) * mask)                                 * k_cls
 *   d tx     = (((sigmoid(tx) - t_tx) * weight) * mask)                                  * k_box     (ty alike)
 *   d tw     = (((2 (tw - t_tw)) * weight) * mask)                                       * k_box     (th alike)
 *
 * Masks are multiplications: a non-finite factor at a masked anchor gives NaN where torch's autograd gives it.  One thread
 * owns an anchor and writes its 5 + C gradient channels; there are no atomics.  So every element of the gradient maps is
 * written exactly once, the maps are the same bit for bit from run to run, and an image's gradient does not depend on the
 * rest of the batch (but for the factor k).
 *
 * The header takes y355_loss_config and the Y355_LOSS_* limits from yolo355_loss.h: the type only, the library links nothing
 * of libyolo355_loss.so or libyolo355.so.  All functions return 0 or a negative Y355_GRAD_E* code; y355_grad_last_error()
 * gives the message of the last failure on the calling thread.  Arguments are checked before any HIP call.  The caller's
 * current device is left as it was.  A handle is single-threaded.
 */
#ifndef YOLO355_GRAD_H
#define YOLO355_GRAD_H

#include <stddef.h>
#include <stdint.h>

#include "yolo355_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_GRAD_OK 0
#define Y355_GRAD_EINVAL (-1)          /* bad argument */
#define Y355_GRAD_EHIP (-2)            /* HIP runtime error */
#define Y355_GRAD_ENOTREADY (-3)       /* no labels set for this batch */

typedef struct y355_grad y355_grad;

const char *y355_grad_last_error(void);

/* the rules of y355_loss_create, on a configuration filled as for it (y355_loss_default_config's values: ignore_thresh 0.5,
 * obj / noobj weights 5 / 1, wh_mul 1, one level) */
int y355_grad_create(const y355_loss_config *cfg, y355_grad **out);
void y355_grad_destroy(y355_grad *h);

/* N: anchors of an image, level 0 first, cell * A + a inside a level */
int y355_grad_num_anchors_total(const y355_grad *h);

/* y355_loss_set_labels: same contract, same checks, same dense [batch][N][11] float32 target tensor, built on the device.
 * Synchronous. */
int y355_grad_set_labels(y355_grad *h, const int32_t *offsets, const double *labels, int32_t batch);

/* *out: the device pointer of the target tensor of the last y355_grad_set_labels (batch: 1 .. its batch), valid until
 * the next y355_grad_set_labels or y355_grad_destroy */
int y355_grad_targets_dev(y355_grad *h, int32_t batch, const void **out);

/* The four losses of a batch and their gradient in one pass over the maps (one terms-and-gradient launch, one finish
 * launch).  pred_dev[num_levels]: fp32 NCHW maps [batch][A * (5 + C)][hs][ws] on the device, channels
 * [obj x A | cls x A*C | txtytwth x A*4].  target_dev: a dense [batch][N][11] float32 tensor on the device, or NULL: the
 * handle's own.  upstream_dev: four fp32 on the device, the gradients arriving at conf_loss, cls_loss, txtytwth_loss and
 * total_loss, read by the kernel; NULL: {0, 0, 0, 1}.  grad_dev[num_levels]: maps of the shape of pred_dev, every element
 * written exactly once (no need to clear them); NULL: the value only.  out[4] and per_image (or NULL) [batch][5]: as
 * y355_loss_compute, bit for bit.  Runs on `stream` and returns after it has finished. */
int y355_grad_forward_backward(y355_grad *h, const void *const *pred_dev, const void *target_dev, int32_t batch,
                               const void *upstream_dev, void *const *grad_dev, void *stream, double *out, double *per_image);

/* The gradient alone, the bits y355_grad_forward_backward writes.  Asynchronous on `stream`: for a backward whose
 * upstream gradients exist only after the forward has returned. */
int y355_grad_backward(y355_grad *h, const void *const *pred_dev, const void *target_dev, int32_t batch, const void *upstream_dev,
                       void *const *grad_dev, void *stream);

/* The same on the tensors tools.loss itself takes, fp32 on the device: conf [batch][N], cls [batch][N][C], txtytwth
 * [batch][N][4], label [batch][N][8] = iou, obj, cls, tx, ty, tw, th, weight; g_conf, g_cls, g_txtytwth of the shapes of
 * the first three, all of them or none (NULL: the value only).  out (with per_image or NULL) as y355_loss_flat, and the call
 * returns after `stream` has finished; out == NULL (then the gradients are required): the gradient alone, asynchronous. */
int y355_grad_flat(int32_t device_id, const void *conf_dev, const void *cls_dev, const void *txtytwth_dev, const void *label_dev,
                   int32_t batch, int32_t num_anchors_total, int32_t num_classes, double obj_weight, double noobj_weight,
                   const void *upstream_dev, void *g_conf_dev, void *g_cls_dev, void *g_txtytwth_dev, void *stream, double *out,
                   double *per_image);

#ifdef __cplusplus
}
#endif
#endif
