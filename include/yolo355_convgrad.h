/*
 * yolo355_convgrad -- C ABI of the companion library libyolo355_convgrad.so: a differentiable convolution of any geometry the
 * operator API accepts (y355_conv_geom of yolo355.h: groups 1, zero padding), on the bf16 MFMA of gfx950, with fp32 parameters
 * that stay on the device.  It is the operator that holds the arithmetic of a network's backward pass; BatchNorm, pooling,
 * upsample, concat, reorg and the optimiser stay the caller's framework's, the loss and its gradient are libyolo355_grad.so's.
 *
 * Arithmetic.  rb = round to nearest even to bf16; every sum in fp32 on v_mfma_f32_16x16x32_bf16 from
 * a zero accumulator, stored as fp32.
 *   forward   z = sum rb(x) rb(W), then + bias (fp32);  y = z > 0 ? z : z * neg_slope, unrounded.
 *   backward  G = rb(dy * (y > 0 ? 1 : neg_slope))  (neg_slope == 1: G = rb(dy), y is not read);
 *             db[co] = sum_{b,oy,ox} G;
 *             dW[co,ci,ky,kx] = sum_{b,oy,ox} G[b,co,oy,ox] rb(x)[b, ci, oy s_h + ky d_h - pad_top, ox s_w + kx d_w - pad_left];
 *             dX = conv_transpose(G, rb(W)); every element of dx is written exactly once, the zeros of pixels no window
 *             reaches included.
 *   No float atomics: the pixel sum of dW / db is cut into runs (y355_convgrad_wgrad_plan), one wave per (tile, tap, run)
 *   writes a partial sum and a second launch adds the runs in their order, so the bits are the same from run to run.
 *
 * x [B][cin][H][W], w [cout][cin][kh][kw], bias [cout], y and dy [B][cout][Ho][Wo], dx as x, dw as w, db as bias: fp32,
 * contiguous, on the handle's device.  The weights are packed on the device inside each call; nothing of a forward is kept in
 * the handle, so a backward may follow any forward and one handle may serve several layers of one geometry.  Launches go on
 * the stream the caller passes and nothing waits for the host, except that a workspace that has to grow is freed and
 * allocated again (the workspaces of a handle are reused in stream order: one handle, one stream at a time, one thread).
 *
 * All functions return 0 or a negative Y355_CONVGRAD_E* code; y355_convgrad_last_error() gives the message of the last failure
 * on the calling thread.  Arguments are checked before any HIP call.  The caller's current device is left as it was.
 */
#ifndef YOLO355_CONVGRAD_H
#define YOLO355_CONVGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y355_CONVGRAD_OK 0
#define Y355_CONVGRAD_EINVAL (-1)      /* bad argument */
#define Y355_CONVGRAD_EHIP (-2)        /* HIP runtime error */

#define Y355_CONVGRAD_MAX_CHANNELS 4096

/* y355_conv_geom's fields and limits: kh, kw 1..32; stride 1..16; dilation 1..32; each pad 0..64 */
typedef struct y355_convgrad_geom {
    int32_t kh, kw, stride_h, stride_w, dil_h, dil_w, pad_top, pad_bottom, pad_left, pad_right;
} y355_convgrad_geom;

typedef struct y355_convgrad y355_convgrad;

const char *y355_convgrad_last_error(void);

/* (Ho, Wo) of a geometry on a height x width map, as y355_conv_geom_out_size gives them; no GPU needed */
int y355_convgrad_out_size(const y355_convgrad_geom *g, int32_t height, int32_t width, int32_t *ho, int32_t *wo);

/* cin, cout 1..Y355_CONVGRAD_MAX_CHANNELS; neg_slope: 1 no activation, 0 ReLU, otherwise LeakyReLU (finite, >= 0) */
int y355_convgrad_create(int32_t device_id, int32_t cin, int32_t cout, const y355_convgrad_geom *g, float neg_slope, y355_convgrad **out);
void y355_convgrad_destroy(y355_convgrad *h);

/* bias_dev may be NULL (no bias) */
int y355_convgrad_forward(y355_convgrad *h, const void *x_dev, const void *w_dev, const void *bias_dev, int32_t batch, int32_t height,
                          int32_t width, void *y_dev, void *stream);
/* y_dev may be NULL only when neg_slope == 1; an output that is NULL is not computed */
int y355_convgrad_backward(y355_convgrad *h, const void *x_dev, const void *w_dev, const void *y_dev, const void *dy_dev, int32_t batch,
                           int32_t height, int32_t width, void *dx_dev, void *dw_dev, void *db_dev, void *stream);
/* out[4] = {npix = B Ho Wo, runs, chunk (pixels of a run, a multiple of 32), last (pixels of the last run)} of the weight
 * gradient at that shape: what y355_convgrad_backward launches from; no device call */
int y355_convgrad_wgrad_plan(const y355_convgrad *h, int32_t batch, int32_t height, int32_t width, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
