// The host side of libyolo355_bntrain.so on the CPU under the address and undefined-behaviour sanitizers
// (make -C csrc hostcheck-bntrain): the rules of y355_bntrain_create (its device-free half), the handle's buffers -- all of them
// or none -- under an allocator that fails at every allocation in turn, BatchNorm2d's initial values in them, every refusal the
// entry points make before a device call (the N < 2 rule of the forward among them), the set_size bookkeeping, and the
// reductions' plan (y355_bntrain_stats_plan: its refusals, its rule, the plans of the two shapes tools/bntrain_bench.py times),
// on a handle whose "device" memory is the host heap.  A stand-alone program; needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../include/yolo355_bntrain.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/y355_host.h"

static std::string g_text;
int y355_fail(int code, const std::string &msg) {      // the library's own is left out under -DY355_HOSTCHECK
    g_text = msg;
    return code;
}

// bntrain.hip's two halves of a create and what goes with them (the struct stays the library's)
int bntrain_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_bntrain **out);
int bntrain_buffers(y355_bntrain *h);
DevOwner &bntrain_owner(y355_bntrain *h);
void bntrain_free(y355_bntrain *h);
void bntrain_state(const y355_bntrain *h, int *hw_batch);

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_text.c_str()); \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// the host heap as device memory: every block is tracked, the fail_at-th allocation from now (0-based) fails
static std::set<void *> live;
static int fail_at = -1, allocs_seen = 0;
static DevMem host_mem() {
    DevMem m;
    m.alloc = [](void **p, size_t bytes, bool zero) {
        if (allocs_seen++ == fail_at) return y355_fail(Y355_EHIP, "allocation refused");
        *p = zero ? std::calloc(1, bytes ? bytes : 16) : std::malloc(bytes ? bytes : 16);
        live.insert(*p);
        return 0;
    };
    m.release = [](void *p) {
        EXPECT(live.erase(p) == 1);                       // never twice, never a stranger
        std::free(p);
    };
    m.upload = [](void *dst, const void *src, size_t bytes, hipStream_t) {
        std::memcpy(dst, src, bytes);
        return 0;
    };
    return m;
}

static void refused_create(const char *text, int h, int w, int c, int a, int b) {
    y355_bntrain *t = (y355_bntrain *)16;
    g_text.clear();
    const int rc = bntrain_open(h, w, c, a, b, host_mem(), &t);
    if (rc != Y355_BNTRAIN_EINVAL || t || g_text.find(text) == std::string::npos || !live.empty()) {
        std::printf("expected a create refused with \"%s\", got %d \"%s\"\n", text, rc, g_text.c_str());
        ++failures;
    }
}

static void check_rules() {
    EXPECT(bntrain_open(64, 64, 2, 5, 1, host_mem(), nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_create: null argument");
    refused_create("multiples of 16", 60, 64, 2, 5, 1);
    refused_create("multiples of 16", 64, 72, 2, 5, 1);
    refused_create("multiples of 16", 0, 64, 2, 5, 1);
    refused_create("multiples of 16", 64, 4112, 2, 5, 1);
    refused_create("num_classes must be 1..200", 64, 64, 0, 5, 1);
    refused_create("num_classes must be 1..200", 64, 64, 201, 5, 1);
    refused_create("num_anchors must be 1..16", 64, 64, 2, 0, 1);
    refused_create("num_anchors must be 1..16", 64, 64, 2, 17, 1);
    refused_create("max_batch must be 1..1024", 64, 64, 2, 5, 0);
    refused_create("max_batch must be 1..1024", 64, 64, 2, 5, 1025);
}

// all of the buffers or none, whichever allocation fails; returns the number of allocations of a whole handle
static int check_all_or_none(int h, int w, int c, int a, int b) {
    y355_bntrain *t = nullptr;
    fail_at = -1;
    allocs_seen = 0;
    EXPECT(bntrain_open(h, w, c, a, b, host_mem(), &t) == 0 && t && live.empty());
    EXPECT(bntrain_buffers(t) == 0);
    const int total = allocs_seen;
    EXPECT(total > 0 && (int)live.size() == total && bntrain_owner(t).allocs.size() == (size_t)total);
    bntrain_free(t);
    EXPECT(live.empty());
    for (int k = 0; k < total; ++k) {
        t = nullptr;
        EXPECT(bntrain_open(h, w, c, a, b, host_mem(), &t) == 0 && t);
        allocs_seen = 0;
        fail_at = k;
        g_text.clear();
        EXPECT(bntrain_buffers(t) == Y355_EHIP && g_text == "allocation refused");
        EXPECT(live.empty() && bntrain_owner(t).allocs.empty());        // none
        fail_at = -1;
        EXPECT(bntrain_buffers(t) == 0 && (int)live.size() == total);    // the handle can still get them
        bntrain_free(t);
        EXPECT(live.empty());
    }
    fail_at = -1;
    return total;
}

static void check_refusals_and_sizes() {
    y355_bntrain *t = nullptr;
    EXPECT(bntrain_open(96, 160, 2, 5, 2, host_mem(), &t) == 0 && bntrain_buffers(t) == 0);
    int st[4];
    bntrain_state(t, st);
    EXPECT(st[0] == 96 && st[1] == 160 && st[2] == 0 && st[3] == 0);
    float x[4] = {0, 0, 0, 0};
    int32_t shape[4];
    int64_t n = -1;
    void *p = nullptr;

    EXPECT(y355_bntrain_set_size(nullptr, 64, 64) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_set_size: null handle");
    EXPECT(y355_bntrain_set_size(t, 60, 64) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_set_size: height and width must be multiples of 16");
    EXPECT(y355_bntrain_set_size(t, 64, 8) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_set_size: height and width must be multiples of 16");
    EXPECT(y355_bntrain_set_size(t, 112, 160) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_set_size: size beyond the handle's maximum");
    EXPECT(y355_bntrain_set_size(t, 96, 176) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_set_size: size beyond the handle's maximum");
    bntrain_state(t, st);
    EXPECT(st[0] == 96 && st[1] == 160);                                  // a refused size changes nothing
    EXPECT(y355_bntrain_set_size(t, 64, 64) == 0);
    bntrain_state(t, st);
    EXPECT(st[0] == 64 && st[1] == 64 && st[2] == 0 && st[3] == 0);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_ACT, 0, shape) == 0 && shape[0] == 0 && shape[1] == 64 && shape[2] == 64 && shape[3] == 8);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_ACT, 9, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 256);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_IDX, 6, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 128);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_GRAD, 1, shape) == 0 && shape[1] == 64 && shape[2] == 64 && shape[3] == 16);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_GRAD, 10, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 64);    // 35 -> 64
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_Z, 6, shape) == 0 && shape[1] == 8 && shape[2] == 8 && shape[3] == 128);       // the pre-pool grid
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_DY, 1, shape) == 0 && shape[1] == 64 && shape[2] == 64 && shape[3] == 16);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_Z, 10, shape) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_tensor_shape: no such tensor");
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_DY, 0, shape) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_IDX, 3, shape) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_tensor_shape(t, 5, 1, shape) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_tensor_shape(t, Y355_BNTRAIN_ACT, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_tensor_shape: null argument");

    EXPECT(y355_bntrain_layer_shape(t, 10, shape) == 0 && shape[0] == 35 && shape[1] == 256);
    EXPECT(y355_bntrain_layer_shape(t, 0, shape) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_layer_shape: layer index must be 1..10");
    EXPECT(y355_bntrain_layer_shape(nullptr, 1, shape) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_layer_shape: null handle");
    EXPECT(y355_bntrain_layer_shape(t, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_layer_shape: null argument");
    EXPECT(y355_bntrain_load_layer(t, 11, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_layer: layer index must be 1..10");
    EXPECT(y355_bntrain_load_layer(t, 1, nullptr, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_layer: null argument");
    EXPECT(y355_bntrain_get_layer(nullptr, 1, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_layer: null handle");
    EXPECT(y355_bntrain_get_momentum(t, -1, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_momentum: layer index must be 1..10");
    EXPECT(y355_bntrain_get_packed(t, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_packed: null argument");
    EXPECT(y355_bntrain_get_grad(t, 1, x, x) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_get_grad: no backward pass has run");
    EXPECT(y355_bntrain_load_bn(t, 10, x, x, x, x, 0) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_bn: layer index must be 1..9");
    EXPECT(y355_bntrain_load_bn(t, 0, x, x, x, x, 0) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_load_bn(nullptr, 1, x, x, x, x, 0) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_bn: null handle");
    EXPECT(y355_bntrain_load_bn(t, 1, x, nullptr, x, x, 0) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_bn: null argument");
    EXPECT(y355_bntrain_load_bn(t, 1, x, x, x, x, -1) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_load_bn: num_batches_tracked must not be negative");
    EXPECT(y355_bntrain_get_bn(t, 10, x, x, x, x, &n) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_bn: layer index must be 1..9" && n == -1);
    EXPECT(y355_bntrain_get_bn_grad(t, 10, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_bn_grad: layer index must be 1..9");
    EXPECT(y355_bntrain_get_bn_grad(t, 1, x, x) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_get_bn_grad: no backward pass has run");
    EXPECT(y355_bntrain_get_bn_momentum(t, 0, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_bn_momentum: layer index must be 1..9");
    EXPECT(y355_bntrain_get_batch_stats(t, 10, x, x, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_batch_stats: layer index must be 1..9");
    EXPECT(y355_bntrain_get_batch_stats(t, 1, x, x, x) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_get_batch_stats: no forward pass has run");

    EXPECT(y355_bntrain_forward(nullptr, x, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_forward: null argument");
    EXPECT(y355_bntrain_forward(t, nullptr, 1, nullptr) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_forward(t, x, 0, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_forward: batch must be 1..max_batch");
    EXPECT(y355_bntrain_forward(t, x, 3, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_forward: batch must be 1..max_batch");
    EXPECT(y355_bntrain_set_size(t, 16, 16) == 0);                         // one value per channel at stride 16: no variance
    EXPECT(y355_bntrain_forward(t, x, 1, nullptr) == Y355_BNTRAIN_EINVAL &&
           g_text.find("y355_bntrain_forward: BatchNorm in training mode needs more than one value per channel") == 0);
    bntrain_state(t, st);
    EXPECT(st[0] == 16 && st[1] == 16 && st[2] == 0 && st[3] == 0);
    EXPECT(y355_bntrain_set_size(t, 64, 64) == 0);
    EXPECT(y355_bntrain_backward(nullptr, x, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_backward: null argument");
    EXPECT(y355_bntrain_backward(t, x, nullptr) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_backward: no forward pass has run at this size");
    EXPECT(y355_bntrain_sgd_step(nullptr, 0.1f, 0.9f, 0.f, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_sgd_step: null handle");
    EXPECT(y355_bntrain_sgd_step(t, std::nanf(""), 0.9f, 0.f, nullptr) == Y355_BNTRAIN_EINVAL &&
           g_text == "y355_bntrain_sgd_step: lr, momentum and weight_decay must be numbers");
    EXPECT(y355_bntrain_sgd_step(t, 0.1f, 0.9f, 0.f, nullptr) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_sgd_step: no backward pass has run");
    EXPECT(y355_bntrain_pred(t, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_pred: null argument");
    EXPECT(y355_bntrain_pred(t, &p) == 0 && p != nullptr && live.count(p) == 1);
    EXPECT(y355_bntrain_get_tensor(t, Y355_BNTRAIN_ACT, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_tensor: null argument");
    EXPECT(y355_bntrain_get_tensor(t, Y355_BNTRAIN_Z, 10, x) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_get_tensor: no such tensor");
    EXPECT(y355_bntrain_get_tensor(t, Y355_BNTRAIN_Z, 1, x) == Y355_BNTRAIN_ENOTREADY && g_text == "y355_bntrain_get_tensor: no forward pass has run at this size");

    bntrain_state(t, st);
    EXPECT(st[0] == 64 && st[1] == 64 && st[2] == 0 && st[3] == 0);       // after all these refusals the handle is as it was
    bntrain_free(t);
    EXPECT(live.empty());
    y355_bntrain_destroy(nullptr);
}

// y355_bntrain_stats_plan: its refusals, its own rule on every BatchNorm layer (at most 1024 runs, chunk a multiple of 128, the
// runs cover the pixels and none is empty, no longer chunks than 1024 runs need), printed
static void check_plan_rule(y355_bntrain *t, int batch) {
    int st[4];
    bntrain_state(t, st);
    static const int div[9] = {1, 2, 4, 4, 8, 8, 16, 16, 16};
    std::printf("stats plan %d x %d x %d:", batch, st[0], st[1]);
    for (int k = 1; k <= 9; ++k) {
        int32_t p[3] = {-1, -1, -1};
        EXPECT(y355_bntrain_stats_plan(t, k, batch, p) == 0);
        const long long N = (long long)batch * (st[0] / div[k - 1]) * (st[1] / div[k - 1]);
        EXPECT(p[0] == N && p[1] >= 1 && p[1] <= 1024 && p[2] >= 128 && p[2] % 128 == 0);
        EXPECT((long long)p[1] * p[2] >= N && (long long)(p[1] - 1) * p[2] < N);
        EXPECT(1024LL * (p[2] - 128) < N);
        std::printf(" %d:{N %d, runs %d, chunk %d, last %lld}", k, p[0], p[1], p[2], N - (long long)(p[1] - 1) * p[2]);
    }
    std::printf("\n");
}

static void check_plans() {
    y355_bntrain *t = nullptr;
    EXPECT(bntrain_open(416, 416, 20, 5, 64, host_mem(), &t) == 0 && t);      // the rules alone: no buffers
    int32_t p[3] = {7, 7, 7};
    EXPECT(y355_bntrain_stats_plan(nullptr, 1, 1, p) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_stats_plan: null handle");
    EXPECT(y355_bntrain_stats_plan(t, 0, 1, p) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_stats_plan: layer index must be 1..9");
    EXPECT(y355_bntrain_stats_plan(t, 10, 1, p) == Y355_BNTRAIN_EINVAL);
    EXPECT(y355_bntrain_stats_plan(t, 1, 1, nullptr) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_stats_plan: null argument");
    EXPECT(y355_bntrain_stats_plan(t, 1, 0, p) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_stats_plan: batch must be 1..max_batch");
    EXPECT(y355_bntrain_stats_plan(t, 1, 65, p) == Y355_BNTRAIN_EINVAL);
    EXPECT(p[0] == 7 && p[1] == 7 && p[2] == 7);                              // a refusal writes nothing
    int32_t w[4] = {7, 7, 7, 7};
    EXPECT(y355_bntrain_wgrad_plan(t, 11, 1, w) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_wgrad_plan: layer index must be 1..10" && w[0] == 7);
    EXPECT(y355_bntrain_wgrad_plan(t, 10, 64, w) == 0 && w[0] == 64 * 26 * 26 && w[3] == 704);     // libyolo355_train.so's plan
    check_plan_rule(t, 64);
    check_plan_rule(t, 1);
    EXPECT(y355_bntrain_set_size(t, 240, 320) == 0);                          // the plan follows the current size
    check_plan_rule(t, 32);
    EXPECT(y355_bntrain_set_size(t, 16, 16) == 0);                            // 1 x 1 maps at stride 16: one run of 128
    check_plan_rule(t, 2);
    EXPECT(y355_bntrain_stats_plan(t, 9, 2, p) == 0 && p[0] == 2 && p[1] == 1 && p[2] == 128);
    bntrain_free(t);
    EXPECT(live.empty());
    EXPECT(bntrain_open(4096, 4096, 2, 5, 1024, host_mem(), &t) == 0 && t);   // 2^34 pixels do not fit the int32 answer
    EXPECT(y355_bntrain_stats_plan(t, 1, 1024, p) == Y355_BNTRAIN_EINVAL && g_text == "y355_bntrain_stats_plan: more than 2^31 - 1 pixels");
    check_plan_rule(t, 127);                                                  // the largest that does
    bntrain_free(t);
}

// BatchNorm2d's initial values are in the buffers of a fresh handle: gamma = 1, beta = 0, running_mean = 0, running_var = 1
// (the "device" is the host heap; read from the owner's blocks, in the order bntrain_buffers asks for them)
static void check_initial_values() {
    y355_bntrain *t = nullptr;
    fail_at = -1;
    EXPECT(bntrain_open(32, 32, 2, 5, 1, host_mem(), &t) == 0 && bntrain_buffers(t) == 0);
    const std::vector<void *> &a = bntrain_owner(t).allocs;                   // p, g, m, bnp, bng, bnm, rstat, ...
    EXPECT(a.size() > 7);
    const size_t cs = 16 + 32 + 64 + 64 + 128 + 128 + 256 + 256 + 256;
    const float *bnp = (const float *)a[3], *rstat = (const float *)a[6];
    bool ok = true;
    for (size_t i = 0; i < cs; ++i) ok = ok && bnp[i] == 1.0f && bnp[cs + i] == 0.0f && rstat[i] == 0.0f && rstat[cs + i] == 1.0f;
    EXPECT(ok);
    bntrain_free(t);
    EXPECT(live.empty());
}

int main() {
    check_rules();
    check_plans();
    const int n = check_all_or_none(64, 96, 2, 5, 2);
    check_all_or_none(32, 16, 20, 5, 1);
    check_initial_values();
    check_refusals_and_sizes();
    if (failures) {
        std::printf("bntrain_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("bntrain_host_check ok (%d allocations per handle)\n", n);
    return 0;
}
