/*
 * yolo355_bntrain -- C ABI of the companion library libyolo355_bntrain.so: one training step of the BatchNorm SlimYOLOv2
 * (models/slim_yolo_v2.py::SlimYOLOv2: nine 3x3 convolutions with bias, BatchNorm2d in training mode and LeakyReLU 0.125,
 * 2x2 max-pools after layers 1, 2, 4 and 6, a plain 3x3 prediction convolution) on the GPU: a forward that takes the batch
 * statistics, moves the running ones and keeps what the backward needs, the backward pass down to the first layer's
 * weights, and torch.optim.SGD (momentum, weight decay, dampening 0, no Nesterov) on every parameter.  The loss stays in
 * libyolo355_grad.so, as for libyolo355_train.so, whose ABI this one mirrors.
 *
 * Arithmetic (an extension of 6m).  rb = round-to-nearest-even to bf16, N = B h w of layer k's
 * pre-pool grid.
 *   forward   A_0 = rb(x);  Z_k = rb(conv(A_{k-1}, rb(W_k)) + b_k), bf16 NHWC on the pre-pool grid, kept;
 *             per channel s = sum Z, q = sum Z^2 in float64 (runs of pixels, one partial each, added in their order: no
 *             atomics), mean64 = s / N, var64 = max(q / N - mean64^2, 0), mean = (float)mean64, var = (float)var64,
 *             invstd = (float)(1 / sqrt(var64 + eps));  running_mean = (float)(0.9 running_mean + 0.1 mean64),
 *             running_var = (float)(0.9 running_var + 0.1 var64 N / (N - 1)), num_batches_tracked += 1;
 *             xhat = (Z - mean) * invstd;  y = xhat * gamma + beta;  v = y > 0 ? y : y * 0.125f  (separately rounded fp32);
 *             A_k = rb(pool_k(v)), I_k the window position of the first maximum;  P = conv(A_9, rb(W_10)) + b_10, fp32 NCHW.
 *   backward  G_10 = rb(dP);  dY_k: section 6m's data gradient from G_{k+1};  dbeta_k = (float) sum dY,
 *             dgamma_k = (float) sum dY xhat  (float64 sums, the same runs);  m1 = dbeta / (float)N, m2 = dgamma / (float)N,
 *             t = dY - m1, t = t - xhat * m2, G_k = rb(t * (gamma * invstd))  (separately rounded fp32);
 *             dW_k, db_k from G_k and A_{k-1} as in section 6m.
 *   update    section 6m's SGD on W, b, gamma, beta of layers 1..9 and W, b of pred, weight decay on all of them; the
 *             running statistics are not parameters.
 *
 * Layers are numbered 1..10 (10 = pred); BatchNorm exists on 1..9.  All functions return 0 or a negative Y355_BNTRAIN_E*
 * code; y355_bntrain_last_error() gives the message of the last failure on the calling thread.  Arguments are checked before
 * any HIP call.  Launches go to the stream the caller passes and nothing waits for the host, but for the entry points that
 * return host values (load / get).  The caller's current device is left as it was.  A handle is single-threaded.
 */
#ifndef YOLO355_BNTRAIN_H
#define YOLO355_BNTRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_BNTRAIN_OK 0
#define Y355_BNTRAIN_EINVAL (-1)       /* bad argument */
#define Y355_BNTRAIN_EHIP (-2)         /* HIP runtime error */
#define Y355_BNTRAIN_ENOTREADY (-3)    /* backward before forward, gradients before backward */

#define Y355_BNTRAIN_LAYERS 10
#define Y355_BNTRAIN_BN_LAYERS 9
#define Y355_BNTRAIN_EPS 1e-5          /* BatchNorm2d's defaults */
#define Y355_BNTRAIN_MOMENTUM 0.1

/* y355_bntrain_get_tensor: kind of tensor t */
#define Y355_BNTRAIN_ACT 0             /* A_t, t = 0..9: bf16 bits (uint16) NHWC [B][h][w][c]; A_0 has 8 channels (3 real) */
#define Y355_BNTRAIN_IDX 1             /* I_t, t in {1, 2, 4, 6}: uint8 NHWC [B][h][w][c] on the pooled grid */
#define Y355_BNTRAIN_GRAD 2            /* G_t, t = 1..10: bf16 bits NHWC on layer t's pre-pool grid (t <= 9: the gradient with
                                          respect to Z_t); G_10 has its channels padded with zeros to a power of two >= 32 */
#define Y355_BNTRAIN_Z 3               /* Z_t, t = 1..9: bf16 bits NHWC on layer t's pre-pool grid */
#define Y355_BNTRAIN_DY 4              /* dY_t, t = 1..9: bf16 bits NHWC on layer t's pre-pool grid */

typedef struct y355_bntrain y355_bntrain;

const char *y355_bntrain_last_error(void);

/* A trainer for inputs up to max_h x max_w (multiples of 16) and batches up to max_batch on the current device, at size
 * max_h x max_w; weights and biases zero until loaded, gamma = 1, beta = 0, running_mean = 0, running_var = 1,
 * num_batches_tracked = 0.  All of its device memory is allocated here, or none. */
int y355_bntrain_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_bntrain **out);
void y355_bntrain_destroy(y355_bntrain *h);

/* the input size of the following forwards (multiples of 16, within the maximum): the reference's set_grid */
int y355_bntrain_set_size(y355_bntrain *h, int32_t height, int32_t width);

/* layer k = 1..10: host fp32 w [cout][cin][3][3] and b [cout].  Synchronous.  load keeps the momentum buffers. */
int y355_bntrain_load_layer(y355_bntrain *h, int32_t k, const float *w, const float *b);
int y355_bntrain_get_layer(y355_bntrain *h, int32_t k, float *w, float *b);
/* [cout, cin] of layer k into shape[2] */
int y355_bntrain_layer_shape(const y355_bntrain *h, int32_t k, int32_t *shape);
/* BatchNorm of layer k = 1..9: host fp32 [cout] each and the count.  Synchronous.  get: any pointer may be NULL. */
int y355_bntrain_load_bn(y355_bntrain *h, int32_t k, const float *gamma, const float *beta, const float *running_mean, const float *running_var,
                         int64_t num_batches_tracked);
int y355_bntrain_get_bn(y355_bntrain *h, int32_t k, float *gamma, float *beta, float *running_mean, float *running_var, int64_t *num_batches_tracked);

/* x_dev: fp32 NCHW [batch][3][H][W] on the device.  Always in training mode: batch statistics, and the running ones move.
 * Refused where batch * H/16 * W/16 < 2 (one value per channel has no variance). */
int y355_bntrain_forward(y355_bntrain *h, const void *x_dev, int32_t batch, void *stream);
/* *out: the device pointer of P (fp32 NCHW) of the last forward, valid until y355_bntrain_destroy */
int y355_bntrain_pred(y355_bntrain *h, void **out);
/* mean, var (biased) and invstd of layer k = 1..9 in the last forward, host fp32 [cout]; any may be NULL */
int y355_bntrain_get_batch_stats(y355_bntrain *h, int32_t k, float *mean, float *var, float *invstd);
/* dpred_dev: fp32 NCHW, the shape of P; needs the tensors of a forward */
int y355_bntrain_backward(y355_bntrain *h, const void *dpred_dev, void *stream);
/* the gradients of the last backward (an update leaves them as they were), host fp32; either may be NULL */
int y355_bntrain_get_grad(y355_bntrain *h, int32_t k, float *dw, float *db);
int y355_bntrain_get_bn_grad(y355_bntrain *h, int32_t k, float *dgamma, float *dbeta);
/* the momentum buffers, host fp32; and rb(W_k) as the forward reads it, bf16 bits [cout][cin][3][3] */
int y355_bntrain_get_momentum(y355_bntrain *h, int32_t k, float *mw, float *mb);
int y355_bntrain_get_bn_momentum(y355_bntrain *h, int32_t k, float *mgamma, float *mbeta);
int y355_bntrain_get_packed(y355_bntrain *h, int32_t k, uint16_t *w_bf16);

/* y355_train_wgrad_plan's answer for layer k = 1..10: out[4] = {npix, max_runs, runs, chunk}; no device call */
int y355_bntrain_wgrad_plan(const y355_bntrain *h, int32_t k, int32_t batch, int32_t *out);
/* How a forward (and a backward) of `batch` images at the current size cuts the reductions of layer k = 1..9 over its
 * N = batch * h * w pixels: out[3] = {N, runs, chunk} -- `runs` workgroup runs of `chunk` pixels each (a multiple of 128; the
 * last run takes the rest), added afterwards in the order of the runs.  A function of the layer, the batch and the size alone,
 * the very one the passes launch from; no device call.  Refused where N does not fit int32_t. */
int y355_bntrain_stats_plan(const y355_bntrain *h, int32_t k, int32_t batch, int32_t *out);

/* the update of every parameter on `stream`; needs the gradients of a backward */
int y355_bntrain_sgd_step(y355_bntrain *h, float lr, float momentum, float weight_decay, void *stream);

/* [B, h, w, c] of tensor t of `kind` at the current size and the last forward's batch into shape[4] */
int y355_bntrain_tensor_shape(const y355_bntrain *h, int32_t kind, int32_t t, int32_t *shape);
/* the tensor to the host (its elements: see the kinds); synchronous */
int y355_bntrain_get_tensor(y355_bntrain *h, int32_t kind, int32_t t, void *out);

#ifdef __cplusplus
}
#endif
#endif
