/*
 * yolo355_qtrain -- C ABI of the companion library libyolo355_qtrain.so: one quantisation-aware fine-tuning step of the
 * BN-folded SlimYOLOv2 on the GPU.  The forward is the deployed int8 network (y355_engine: power-of-two 8-bit weights, biases
 * and activations) computed as a fake quantisation in fp32, bit for bit; the backward is the straight-through estimator; the
 * update is yolo355_train.h's SGD on the fp32 masters, after which weights and biases are quantised again on the device.  The
 * surface is yolo355_train.h's with the entry points of the quantiser on top.  The loss stays in libyolo355_grad.so.
 *
 * Arithmetic.  rne = round half to even; rb = rne to bf16;
 *     fq_e(v) = clip(rne(v * 2^e), -127, 127) * 2^-e.
 * Layers are numbered 1..10 (10 = pred), trackers 0..10 (the input, the nine layers of conv1..conv7, pred).
 *   weights   after every load and every SGD step, per tensor T (W_k or b_k):  m = max|T|,  s = fl32(127 / m),
 *             e = floor(log2 s) taken exactly as the exponent field of s (not through log2f),  Tq = fq_e(T).  An all-zero
 *             tensor takes e = 0, q = 0; where 127 / m overflows fp32 (m below 2^-121) e = 127.
 *             torch.floor(torch.log2(s)) (prep.quantize_tensor) can differ in one place only: s within rounding of a power
 *             of two from below, where log2f may round up to the integer and give e + 1.  There m lies just above
 *             127 * 2^-(e+1), so at e + 1 the largest element still rounds to +-127 and nothing leaves the 8 bits: torch's
 *             tensor is a valid one at twice the scale, this library keeps e.  The tests assert that the two rules agree on
 *             the weights they use.
 *   exponents e_a[0..10] of the activations are frozen values the caller sets (y355_qtrain_set_act_exponents); the tracker's
 *             moving average does not run inside a forward.  Every forward leaves per tracker the batch's max|v| before
 *             quantisation and the number of elements with |rne(v 2^e)| > 127 (counted before the pool); both through
 *             integer atomics, exact and the same from run to run.
 *   forward   A_0 = fq_{e_a[0]}(x), NHWC bf16;  z = conv(A_{k-1}, Wq_k) + bq_k in fp32 (v_mfma_f32_16x16x32_bf16: the
 *             operands q 2^-e are exact in bf16, the products exact, the sums exact while the integer accumulator stays below
 *             2^24);  v = z > 0 ? z : 0.125 z;  a pooled layer takes the 2x2 maximum of the fp32 v, the first position on
 *             ties;  A_k = fq_{e_a[k]}(.) stored as bf16, exact;  P = fq_{e_a[10]}(conv(A_9, Wq_10) + bq_10), fp32 NCHW.
 *             Beside A_k (and P) one state byte per output element, S_k: bits 0-1 the window position (pooled layers),
 *             bit 2 the selected z <= 0 (layers 1..9), bit 3 the element was clipped.
 *   backward  G_10 = rb(dP * [not clipped]);  G_{k-1} = rb(unpool(conv_transpose(G_k, Wq_k)) * (bit 2 ? 0.125 : 1) *
 *             (bit 3 ? 0 : 1)), every element written once;  dW_k, db_k from G_k and the quantised A_{k-1} as in
 *             yolo355_train.h; the quantiser of weights and biases passes the gradient through.  No float atomics.
 *   update    yolo355_train.h's on the fp32 masters, then the quantisation above.
 *
 * All functions return 0 or a negative Y355_QTRAIN_E* code; y355_qtrain_last_error() gives the message of the last failure on
 * the calling thread.  Arguments are checked before any HIP call.  The caller's current device is left as it was.  A handle is
 * single-threaded.
 */
#ifndef YOLO355_QTRAIN_H
#define YOLO355_QTRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_QTRAIN_OK 0
#define Y355_QTRAIN_EINVAL (-1)        /* bad argument */
#define Y355_QTRAIN_EHIP (-2)          /* HIP runtime error */
#define Y355_QTRAIN_ENOTREADY (-3)     /* forward before the exponents, backward before forward, gradients before backward */

#define Y355_QTRAIN_LAYERS 10
#define Y355_QTRAIN_TRACKERS 11
#define Y355_QTRAIN_MAX_ACT_EXPONENT 96     /* |e_a| of y355_qtrain_set_act_exponents */

/* y355_qtrain_get_tensor: kind of tensor t (0..2: as in yolo355_train.h) */
#define Y355_QTRAIN_ACT 0              /* A_t, t = 0..9: bf16 bits NHWC; its values are q * 2^-e_a[t], |q| <= 127 */
#define Y355_QTRAIN_IDX 1              /* t in {1, 2, 4, 6}: the bytes of S_t (the window position is S_t & 3) */
#define Y355_QTRAIN_GRAD 2             /* G_t, t = 1..10: bf16 bits NHWC on layer t's pre-pool grid; G_10 padded as S_10 */
#define Y355_QTRAIN_STATE 3            /* S_t, t = 1..10: uint8 NHWC on A_t's grid; S_10 on P's grid with the channels padded
                                          with zeros to a power of two >= 32 */
#define Y355_QTRAIN_S_POS 3            /* bits 0-1 */
#define Y355_QTRAIN_S_NEG 4            /* bit 2 */
#define Y355_QTRAIN_S_CLIP 8           /* bit 3 */

typedef struct y355_qtrain y355_qtrain;

const char *y355_qtrain_last_error(void);

/* as in yolo355_train.h; the weights are zero (e = 0, q = 0) until loaded */
int y355_qtrain_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_qtrain **out);
void y355_qtrain_destroy(y355_qtrain *h);
int y355_qtrain_set_size(y355_qtrain *h, int32_t height, int32_t width);

/* layer k = 1..10: the fp32 masters, host w [cout][cin][3][3] and b [cout].  load quantises every tensor again.  Synchronous. */
int y355_qtrain_load_layer(y355_qtrain *h, int32_t k, const float *w, const float *b);
int y355_qtrain_get_layer(y355_qtrain *h, int32_t k, float *w, float *b);
int y355_qtrain_layer_shape(const y355_qtrain *h, int32_t k, int32_t *shape);

/* the frozen activation exponents e_a[11], each within +-Y355_QTRAIN_MAX_ACT_EXPONENT; a forward is refused until they are set.
 * The tensors of an earlier forward stay those of the exponents it ran with. */
int y355_qtrain_set_act_exponents(y355_qtrain *h, const int32_t *e_a);
int y355_qtrain_get_act_exponents(const y355_qtrain *h, int32_t *e_a);
/* of the last forward, per tracker: max|v| before quantisation and the elements with |rne(v 2^e)| > 127; either may be NULL */
int y355_qtrain_get_act_stats(y355_qtrain *h, float *max_abs, int64_t *clipped);
/* out[20] = (e_w, e_b) of layers 1..10 as the device computed them; and bq_k, host fp32 [cout] */
int y355_qtrain_get_weight_exponents(y355_qtrain *h, int32_t *out);
int y355_qtrain_get_qbias(y355_qtrain *h, int32_t k, float *bq);

/* x_dev: fp32 NCHW [batch][3][H][W] on the device */
int y355_qtrain_forward(y355_qtrain *h, const void *x_dev, int32_t batch, void *stream);
int y355_qtrain_pred(y355_qtrain *h, void **out);
int y355_qtrain_backward(y355_qtrain *h, const void *dpred_dev, void *stream);
int y355_qtrain_get_grad(y355_qtrain *h, int32_t k, float *dw, float *db);
int y355_qtrain_get_momentum(y355_qtrain *h, int32_t k, float *mw, float *mb);
/* Wq_k as the forward reads it, bf16 bits [cout][cin][3][3] */
int y355_qtrain_get_packed(y355_qtrain *h, int32_t k, uint16_t *w_bf16);
int y355_qtrain_wgrad_plan(const y355_qtrain *h, int32_t k, int32_t batch, int32_t *out);

/* the update of every master on `stream`, then the quantisation of every tensor; needs the gradients of a backward */
int y355_qtrain_sgd_step(y355_qtrain *h, float lr, float momentum, float weight_decay, void *stream);

int y355_qtrain_tensor_shape(const y355_qtrain *h, int32_t kind, int32_t t, int32_t *shape);
int y355_qtrain_get_tensor(y355_qtrain *h, int32_t kind, int32_t t, void *out);

#ifdef __cplusplus
}
#endif
#endif
