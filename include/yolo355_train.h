/*
 * yolo355_train -- C ABI of the companion library libyolo355_train.so: one fine-tuning step of the BN-folded SlimYOLOv2
 * (SlimYOLOv2_quantize_bnfuse: nine 3x3 convolutions with bias and LeakyReLU 0.125, 2x2 max-pools after layers 1, 2, 4 and 6,
 * a 3x3 prediction convolution) on the GPU: a forward that keeps what the backward needs, the backward pass down to the
 * first layer's weights, and torch.optim.SGD (momentum, weight decay, dampening 0, no Nesterov).  The loss stays in
 * libyolo355_grad.so: y355_train_pred's map goes to y355_grad_forward_backward, its gradient map to y355_train_backward.
 *
 * Arithmetic.  rb = round-to-nearest-even to bf16.
 *   forward   A_0 = rb(x);  A_k = rb(pool_k(leaky(conv(A_{k-1}, rb(W_k)) + b_k))), k = 1..9, sums in fp32 on
 *             v_mfma_f32_16x16x32_bf16, bias and slope in fp32, the pool on the fp32 values; a pooled layer also stores
 *             I_k in {0,1,2,3}, the row-major window position of the maximum (the first one on ties);
 *             P = conv(A_9, rb(W_10)) + b_10 in fp32, NCHW [B][A(5+C)][H/16][W/16].
 *   backward  G_10 = rb(dP);  db_k = sum G_k,  dW_k = sum G_k * shifted A_{k-1}  (fp32 sums of exact products, split over
 *             workgroups into a workspace and added in a fixed order: no atomics, the same bits from run to run);
 *             G_{k-1} = rb(unpool_{I_{k-1}}(conv_transpose(G_k, rb(W_k)) * (A_{k-1} > 0 ? 1 : 0.125))), every element
 *             written exactly once.  The gradient with respect to the image is not computed.
 *   update    g += weight_decay * p;  buf = first step ? g : momentum * buf + g;  p -= lr * buf;  every operation a
 *             separately rounded fp32 operation; then rb(W) is packed again for the forward and the data gradient.
 * Master weights, biases, gradients and momentum are fp32.
 *
 * Layers are numbered 1..10 (10 = pred).  All functions return 0 or a negative Y355_TRAIN_E* code;
 * y355_train_last_error() gives the message of the last failure on the calling thread.  Arguments are checked before any HIP
 * call.  Launches go to the stream the caller passes and nothing waits for the host, but for the entry points that return
 * host values (load / get).  The caller's current device is left as it was.  A handle is single-threaded.
 */
#ifndef YOLO355_TRAIN_H
#define YOLO355_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_TRAIN_OK 0
#define Y355_TRAIN_EINVAL (-1)         /* bad argument */
#define Y355_TRAIN_EHIP (-2)           /* HIP runtime error */
#define Y355_TRAIN_ENOTREADY (-3)      /* backward before forward, gradients before backward */

#define Y355_TRAIN_LAYERS 10

/* y355_train_get_tensor: kind of tensor t */
#define Y355_TRAIN_ACT 0               /* A_t, t = 0..9: bf16 bits (uint16) NHWC [B][h][w][c]; A_0 has 8 channels (3 real) */
#define Y355_TRAIN_IDX 1               /* I_t, t in {1, 2, 4, 6}: uint8 NHWC [B][h][w][c] on the pooled grid */
#define Y355_TRAIN_GRAD 2              /* G_t, t = 1..10: bf16 bits NHWC [B][h][w][c] on layer t's pre-pool grid; G_10 has
                                          its channels padded with zeros to a power of two >= 32 */

typedef struct y355_train y355_train;

const char *y355_train_last_error(void);

/* A trainer for inputs up to max_h x max_w (multiples of 16) and batches up to max_batch on the current device, at size
 * max_h x max_w; weights zero until loaded.  All of its device memory is allocated here, or none. */
int y355_train_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_train **out);
void y355_train_destroy(y355_train *h);

/* the input size of the following forwards (multiples of 16, within the maximum): the reference's set_grid */
int y355_train_set_size(y355_train *h, int32_t height, int32_t width);

/* layer k = 1..10: host fp32 w [cout][cin][3][3] and b [cout].  Synchronous.  load keeps the momentum buffers. */
int y355_train_load_layer(y355_train *h, int32_t k, const float *w, const float *b);
int y355_train_get_layer(y355_train *h, int32_t k, float *w, float *b);
/* [cout, cin] of layer k into shape[2] */
int y355_train_layer_shape(const y355_train *h, int32_t k, int32_t *shape);

/* x_dev: fp32 NCHW [batch][3][H][W] on the device */
int y355_train_forward(y355_train *h, const void *x_dev, int32_t batch, void *stream);
/* *out: the device pointer of P (fp32 NCHW) of the last forward, valid until y355_train_destroy */
int y355_train_pred(y355_train *h, void **out);
/* dpred_dev: fp32 NCHW, the shape of P; needs the tensors of a forward */
int y355_train_backward(y355_train *h, const void *dpred_dev, void *stream);
/* the gradients of the last backward (an update leaves them as they were), host fp32; either may be NULL */
int y355_train_get_grad(y355_train *h, int32_t k, float *dw, float *db);
/* the momentum buffers, host fp32; and rb(W_k) as the forward reads it, bf16 bits [cout][cin][3][3] */
int y355_train_get_momentum(y355_train *h, int32_t k, float *mw, float *mb);
int y355_train_get_packed(y355_train *h, int32_t k, uint16_t *w_bf16);

/* How a backward after a forward of `batch` images (1..max_batch) at the current size splits layer k's weight gradient:
 * out[4] = {npix, max_runs, runs, chunk}.  The npix = batch * h * w pixels of G_k go to `runs` <= max_runs workgroup runs of
 * `chunk` pixels each (a multiple of 32; the last run takes the rest), added afterwards in the order of the runs.  The very
 * function the backward launches from; no device call.  Refused where npix does not fit int32_t. */
int y355_train_wgrad_plan(const y355_train *h, int32_t k, int32_t batch, int32_t *out);

/* one launch over all parameters on `stream`; needs the gradients of a backward */
int y355_train_sgd_step(y355_train *h, float lr, float momentum, float weight_decay, void *stream);

/* [B, h, w, c] of tensor t of `kind` at the current size and the last forward's batch into shape[4] */
int y355_train_tensor_shape(const y355_train *h, int32_t kind, int32_t t, int32_t *shape);
/* the tensor to the host (its elements: see the kinds); synchronous */
int y355_train_get_tensor(y355_train *h, int32_t kind, int32_t t, void *out);

#ifdef __cplusplus
}
#endif
#endif
