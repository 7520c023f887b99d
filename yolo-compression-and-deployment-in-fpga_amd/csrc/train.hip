// yolo355_train -- one fine-tuning step of the BN-folded SlimYOLOv2 on the GPU (gfx950): forward with what the backward
// needs, data and weight gradients of the ten 3x3 convolutions, SGD; C ABI in include/yolo355_train.h, linked into
// libyolo355_train.so on its own (nothing of libyolo355.so is used).  The arithmetic contract is DESIGN.md section 6m.
//
// Layouts.  Activations A_t, pool positions I_t and gradients G_t are NHWC (a pixel's channels are contiguous), so a lane's
// MFMA fragment of eight consecutive input channels of one tap is one 16-byte load.  The GEMM index of a convolution is
// k = tap * cinp + ci (cinp a power of two >= 8), cut into k-steps of 32; weights are packed per (16-row tile, k-step) as
// the 64 x 16 bytes of the A operand (lane (g, i): row i, k = 8 g .. 8 g + 7).
//
// The kernels (train_core.h, which bntrain.hip compiles too):
//   train_input_kernel  A_0 = rb(x): NCHW fp32 -> NHWC bf16, 3 channels padded to 8
//   train_conv_kernel    implicit GEMM, rows = output channels (packed weights), columns = pixels (gathered from NHWC with
//                        zero padding), four column sets per wave: four runs of 16 pixels, or the four positions of 16
//                        pooling windows.  Epilogues: bias + LeakyReLU (+ 2x2 pool with I_k) -> bf16; bias -> fp32 NCHW (P);
//                        data gradient: times the slope mask of A_{k-1}, rb, written through I_{k-1} (all four positions).
//   train_dpred_kernel   G_10 = rb(dP): NCHW fp32 -> NHWC bf16, channels padded with zeros
//   train_wgrad_kernel   dW_k and db_k: rows = output channels of G_k, columns = 16 input channels of A_{k-1} for each of
//                        the nine taps, summed over a run of pixels; one wave per (tile, run), partial sums to a workspace
//   train_reduce_kernel  adds the runs in a fixed order (four interleaved chains, then their sum): no atomics
//   train_sgd_kernel     the update of every parameter and the bf16 packs of the forward and of the data gradient
//
// The handle, the create rules, the device memory, the entry points' bodies and the launches of a layer are train_host.h's
// (bntrain.hip compiles it too); this file owns the two passes' loops and the C ABI.
#include "../../include/yolo355_train.h"
#pragma GCC visibility push(hidden)
#include "y355_host.h"
static_assert(Y355_TRAIN_OK == Y355_OK && Y355_TRAIN_EINVAL == Y355_EINVAL && Y355_TRAIN_EHIP == Y355_EHIP && Y355_TRAIN_ENOTREADY == Y355_ENOTREADY,
              "y355_fail and HIPCHK return yolo355.h's codes");

static thread_local std::string g_err;                  // y355_train_last_error's text
#ifndef Y355_HOSTCHECK                                   // (train_host_check.cpp links its own)
int y355_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#endif

#define TRAIN_FAMILY "y355_train"
#include "train_core.h"
#include "train_host.h"
static_assert(NL == Y355_TRAIN_LAYERS, "train_core.h's layer table");
static_assert(Y355_TRAIN_ACT == T_ACT && Y355_TRAIN_IDX == T_IDX && Y355_TRAIN_GRAD == T_GRAD, "train_host.h's tensor kinds");

struct y355_train : TrainCore {};

// The seams of train_host_check.cpp, which does not see the struct: y355_train_create's two parts (the rules and the host
// state; all of the device memory or none of it), the owner, the release and the state the refusals must leave alone.
int train_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_train **out) {
    return core_open(max_h, max_w, num_classes, num_anchors, max_batch, mem, out);
}
int train_buffers(y355_train *h) {
    return core_buffers(h, [] { return 0; }, [](int, size_t) { return 0; });
}
DevOwner &train_owner(y355_train *h) { return h->own; }
void train_free(y355_train *h) { core_free(h); }
void train_state(const y355_train *h, int *hw_batch) { core_state(h, hw_batch); }
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------------------- C ABI
extern "C" {

const char *y355_train_last_error(void) { return g_err.c_str(); }

int y355_train_create(int32_t max_h, int32_t max_w, int32_t num_classes, int32_t num_anchors, int32_t max_batch, y355_train **out) {
    return core_create(max_h, max_w, num_classes, num_anchors, max_batch, out, train_open, train_buffers);
}
void y355_train_destroy(y355_train *h) { core_destroy(h); }
int y355_train_set_size(y355_train *h, int32_t height, int32_t width) { return core_set_size(h, height, width); }
int y355_train_layer_shape(const y355_train *h, int32_t k, int32_t *shape) { return core_layer_shape(h, k, shape); }
int y355_train_load_layer(y355_train *h, int32_t k, const float *w, const float *b) { return core_load_layer(h, k, w, b); }
int y355_train_get_layer(y355_train *h, int32_t k, float *w, float *b) { return core_get_layer(h, k, w, b); }
int y355_train_get_grad(y355_train *h, int32_t k, float *dw, float *db) { return core_get_grad(h, k, dw, db); }
int y355_train_get_momentum(y355_train *h, int32_t k, float *mw, float *mb) { return core_get_momentum(h, k, mw, mb); }
int y355_train_get_packed(y355_train *h, int32_t k, uint16_t *w_bf16) { return core_get_packed(h, k, w_bf16); }
int y355_train_pred(y355_train *h, void **out) { return core_pred(h, out); }
int y355_train_wgrad_plan(const y355_train *h, int32_t k, int32_t batch, int32_t *out) { return core_wgrad_plan(h, k, batch, out); }
int y355_train_tensor_shape(const y355_train *h, int32_t kind, int32_t t, int32_t *shape) { return core_tensor_shape(h, kind, t, shape); }
int y355_train_get_tensor(y355_train *h, int32_t kind, int32_t t, void *out) { return core_get_tensor(h, kind, t, out); }
int y355_train_sgd_step(y355_train *h, float lr, float momentum, float weight_decay, void *stream) {
    return core_sgd_step(h, lr, momentum, weight_decay, stream, [](int) { return hipSuccess; });
}

int y355_train_forward(y355_train *h, const void *x_dev, int32_t batch, void *stream) {
    if (int rc = forward_args(h, x_dev, batch)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_input(h, x_dev, batch, s));
    for (int k = 1; k < NL; ++k)
        HIPCHK(kPool[k - 1] ? launch_forward<M_FWD_POOL>(h, k, batch, h->act[k], h->idx[k], s) : launch_forward<M_FWD>(h, k, batch, h->act[k], nullptr, s));
    HIPCHK(launch_forward<M_PRED>(h, NL, batch, h->pred, nullptr, s));
    h->batch = batch;
    return Y355_TRAIN_OK;
}

int y355_train_backward(y355_train *h, const void *dpred_dev, void *stream) {
    if (int rc = backward_args(h, dpred_dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DeviceGuard g;
    HIPCHK(g.set(h->device_id));
    HIPCHK(launch_dpred(h, dpred_dev, s));
    for (int k = NL; k >= 1; --k) {
        HIPCHK(launch_wgrad(h, k, s));
        if (k > 1) HIPCHK(launch_dgrad(h, k, h->grad[k - 1], s));     // the gradient with respect to the image is not computed
    }
    h->have_grad = true;
    return Y355_TRAIN_OK;
}

}  // extern "C"
