// The host side of libyolo355_qtrain.so on the CPU under the address and undefined-behaviour sanitizers
// (make -C csrc hostcheck-qtrain): the rules of y355_qtrain_create (its device-free half), the handle's buffers -- all of them
// or none -- under an allocator that fails at every allocation in turn, every refusal the entry points make before a device
// call (a forward without activation exponents among them) leaving the state alone, the state tensor's shapes, and the exponent
// rule on the host at m = 0, exact powers of two, ordinary values and denormals, on a handle whose "device" memory is the host
// heap.  A stand-alone program; needs no GPU.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "../include/yolo355_qtrain.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/y355_host.h"

static std::string g_text;
int y355_fail(int code, const std::string &msg) {      // the library's own is left out under -DY355_HOSTCHECK
    g_text = msg;
    return code;
}

// qtrain.hip's two halves of a create and what goes with them (the struct stays the library's)
int qtrain_open(int max_h, int max_w, int num_classes, int num_anchors, int max_batch, const DevMem &mem, y355_qtrain **out);
int qtrain_buffers(y355_qtrain *h);
DevOwner &qtrain_owner(y355_qtrain *h);
void qtrain_free(y355_qtrain *h);
void qtrain_state(const y355_qtrain *h, int *hw_batch);       // H, W, batch, have_grad, exponents set
int qtrain_exponent_host(float m);

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
    y355_qtrain *t = (y355_qtrain *)16;
    g_text.clear();
    const int rc = qtrain_open(h, w, c, a, b, host_mem(), &t);
    if (rc != Y355_QTRAIN_EINVAL || t || g_text.find(text) == std::string::npos || g_text.find("y355_qtrain_create: ") != 0 || !live.empty()) {
        std::printf("expected a create refused with \"%s\", got %d \"%s\"\n", text, rc, g_text.c_str());
        ++failures;
    }
}

static void check_rules() {
    EXPECT(qtrain_open(64, 64, 2, 5, 1, host_mem(), nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_create: null argument");
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
    y355_qtrain *t = nullptr;
    fail_at = -1;
    allocs_seen = 0;
    EXPECT(qtrain_open(h, w, c, a, b, host_mem(), &t) == 0 && t && live.empty());
    EXPECT(qtrain_buffers(t) == 0);
    const int total = allocs_seen;
    EXPECT(total > 0 && (int)live.size() == total && qtrain_owner(t).allocs.size() == (size_t)total);
    qtrain_free(t);
    EXPECT(live.empty());
    for (int k = 0; k < total; ++k) {
        t = nullptr;
        EXPECT(qtrain_open(h, w, c, a, b, host_mem(), &t) == 0 && t);
        allocs_seen = 0;
        fail_at = k;
        g_text.clear();
        EXPECT(qtrain_buffers(t) == Y355_EHIP && g_text == "allocation refused");
        EXPECT(live.empty() && qtrain_owner(t).allocs.empty());          // none
        int32_t shape[4];                                                 // ... and no pointer left behind: the shapes still answer
        EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 3, shape) == 0);
        fail_at = -1;
        EXPECT(qtrain_buffers(t) == 0 && (int)live.size() == total);      // the handle can still get them
        qtrain_free(t);
        EXPECT(live.empty());
    }
    fail_at = -1;
    return total;
}

static void check_refusals_and_sizes() {
    y355_qtrain *t = nullptr;
    EXPECT(qtrain_open(96, 160, 2, 5, 2, host_mem(), &t) == 0 && qtrain_buffers(t) == 0);
    int st[5];
    qtrain_state(t, st);
    EXPECT(st[0] == 96 && st[1] == 160 && st[2] == 0 && st[3] == 0 && st[4] == 0);
    float x[4] = {0, 0, 0, 0};
    int32_t shape[4], ea[11] = {5, 4, 3, 3, 3, 3, 3, 3, 3, 3, 2}, back[11];
    void *p = nullptr;

    EXPECT(y355_qtrain_set_size(nullptr, 64, 64) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_set_size: null handle");
    EXPECT(y355_qtrain_set_size(t, 60, 64) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_set_size: height and width must be multiples of 16");
    EXPECT(y355_qtrain_set_size(t, 112, 160) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_set_size: size beyond the handle's maximum");
    EXPECT(y355_qtrain_set_size(t, 64, 64) == 0);
    qtrain_state(t, st);
    EXPECT(st[0] == 64 && st[1] == 64 && st[2] == 0 && st[3] == 0);

    // S_t: on A_t's grid (the pooled one of layers 1, 2, 4, 6), S_10 on P's with the channels padded; one kind more than the others have
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 1, shape) == 0 && shape[0] == 0 && shape[1] == 32 && shape[2] == 32 && shape[3] == 16);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 3, shape) == 0 && shape[1] == 16 && shape[2] == 16 && shape[3] == 64);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 6, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 128);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 9, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 256);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 10, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 64);     // 35 -> 64
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_IDX, 6, shape) == 0 && shape[1] == 4 && shape[2] == 4 && shape[3] == 128);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_GRAD, 10, shape) == 0 && shape[3] == 64);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 0, shape) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_tensor_shape: no such tensor");
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_STATE, 11, shape) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_IDX, 3, shape) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_tensor_shape(t, 4, 1, shape) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_tensor_shape(t, Y355_QTRAIN_ACT, 1, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_tensor_shape: null argument");

    EXPECT(y355_qtrain_layer_shape(t, 10, shape) == 0 && shape[0] == 35 && shape[1] == 256);
    EXPECT(y355_qtrain_layer_shape(t, 0, shape) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_layer_shape: layer index must be 1..10");
    EXPECT(y355_qtrain_load_layer(t, 0, x, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_load_layer: layer index must be 1..10");
    EXPECT(y355_qtrain_load_layer(t, 11, x, x) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_load_layer(t, 1, nullptr, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_load_layer: null argument");
    EXPECT(y355_qtrain_get_layer(nullptr, 1, x, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_layer: null handle");
    EXPECT(y355_qtrain_get_packed(t, 1, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_packed: null argument");
    EXPECT(y355_qtrain_get_grad(t, 1, x, x) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_get_grad: no backward pass has run");
    EXPECT(y355_qtrain_get_qbias(t, 0, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_qbias: layer index must be 1..10");
    EXPECT(y355_qtrain_get_qbias(t, 1, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_qbias: null argument");
    EXPECT(y355_qtrain_get_qbias(nullptr, 1, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_qbias: null handle");
    EXPECT(y355_qtrain_get_weight_exponents(t, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_weight_exponents: null argument");
    EXPECT(y355_qtrain_get_act_stats(nullptr, x, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_act_stats: null handle");
    EXPECT(y355_qtrain_get_act_stats(t, x, nullptr) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_get_act_stats: no forward pass has run at this size");

    // the exponents: a forward is refused until they are set; a refused set changes nothing
    EXPECT(y355_qtrain_forward(nullptr, x, 1, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_forward: null argument");
    EXPECT(y355_qtrain_forward(t, x, 0, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_forward: batch must be 1..max_batch");
    EXPECT(y355_qtrain_forward(t, x, 1, nullptr) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_forward: the activation exponents are not set");
    EXPECT(y355_qtrain_get_act_exponents(t, back) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_get_act_exponents: the activation exponents are not set");
    EXPECT(y355_qtrain_set_act_exponents(t, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_set_act_exponents: null argument");
    EXPECT(y355_qtrain_set_act_exponents(nullptr, ea) == Y355_QTRAIN_EINVAL);
    ea[10] = 97;
    EXPECT(y355_qtrain_set_act_exponents(t, ea) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_set_act_exponents: an exponent beyond +-96");
    ea[10] = -97;
    EXPECT(y355_qtrain_set_act_exponents(t, ea) == Y355_QTRAIN_EINVAL);
    qtrain_state(t, st);
    EXPECT(st[4] == 0);
    EXPECT(y355_qtrain_forward(t, x, 1, nullptr) == Y355_QTRAIN_ENOTREADY);
    ea[10] = -96;
    EXPECT(y355_qtrain_set_act_exponents(t, ea) == 0);
    qtrain_state(t, st);
    EXPECT(st[4] == 1 && st[2] == 0 && st[3] == 0);
    EXPECT(y355_qtrain_get_act_exponents(t, back) == 0 && std::memcmp(back, ea, sizeof(ea)) == 0);
    ea[0] = 200;
    EXPECT(y355_qtrain_set_act_exponents(t, ea) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_get_act_exponents(t, back) == 0 && back[0] == 5 && back[10] == -96);          // the earlier set stays
    EXPECT(y355_qtrain_forward(t, x, 3, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_forward: batch must be 1..max_batch");

    EXPECT(y355_qtrain_backward(nullptr, x, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_backward: null argument");
    EXPECT(y355_qtrain_backward(t, x, nullptr) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_backward: no forward pass has run at this size");
    EXPECT(y355_qtrain_sgd_step(nullptr, 0.1f, 0.9f, 0.f, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_sgd_step: null handle");
    EXPECT(y355_qtrain_sgd_step(t, std::nanf(""), 0.9f, 0.f, nullptr) == Y355_QTRAIN_EINVAL);
    EXPECT(y355_qtrain_sgd_step(t, 0.1f, 0.9f, 0.f, nullptr) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_sgd_step: no backward pass has run");
    EXPECT(y355_qtrain_pred(t, &p) == 0 && p != nullptr && live.count(p) == 1);
    EXPECT(y355_qtrain_get_tensor(t, Y355_QTRAIN_STATE, 1, nullptr) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_tensor: null argument");
    EXPECT(y355_qtrain_get_tensor(t, Y355_QTRAIN_STATE, 0, x) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_get_tensor: no such tensor");
    EXPECT(y355_qtrain_get_tensor(t, Y355_QTRAIN_STATE, 1, x) == Y355_QTRAIN_ENOTREADY && g_text == "y355_qtrain_get_tensor: no forward pass has run at this size");
    int32_t plan[4];
    EXPECT(y355_qtrain_wgrad_plan(t, 1, 2, plan) == 0 && plan[0] == 2 * 64 * 64);
    EXPECT(y355_qtrain_wgrad_plan(t, 1, 3, plan) == Y355_QTRAIN_EINVAL && g_text == "y355_qtrain_wgrad_plan: batch must be 1..max_batch");

    // after all these refusals the handle is as it was
    qtrain_state(t, st);
    EXPECT(st[0] == 64 && st[1] == 64 && st[2] == 0 && st[3] == 0 && st[4] == 1);
    EXPECT(y355_qtrain_set_size(t, 96, 160) == 0);
    qtrain_state(t, st);
    EXPECT(st[0] == 96 && st[1] == 160 && st[4] == 1);                    // a new size keeps the exponents
    qtrain_free(t);
    EXPECT(live.empty());
    y355_qtrain_destroy(nullptr);
}

// e = floor(log2(fl32(127 / m))) as the exponent field of the quotient
static void check_exponent_rule() {
    EXPECT(qtrain_exponent_host(0.f) == 0 && qtrain_exponent_host(-0.f) == 0 && qtrain_exponent_host(std::nanf("")) == 0);
    for (int j = -120; j <= 127; ++j) {                       // m = 2^j: s = 127 2^-j, e = 6 - j
        const float m = std::ldexp(1.0f, j);
        EXPECT(qtrain_exponent_host(m) == 6 - j);
    }
    EXPECT(qtrain_exponent_host(FLT_MAX) == -122);
    EXPECT(qtrain_exponent_host(std::ldexp(1.0f, -121)) == 127);          // 127 2^121 is below FLT_MAX: still the field
    EXPECT(qtrain_exponent_host(std::ldexp(1.0f, -122)) == 127);          // the quotient overflows: the largest exponent
    EXPECT(qtrain_exponent_host(FLT_MIN) == 127);
    EXPECT(qtrain_exponent_host(std::ldexp(1.0f, -149)) == 127 && qtrain_exponent_host(1e-40f) == 127);      // denormals
    EXPECT(qtrain_exponent_host(1.0f) == 6 && qtrain_exponent_host(0.99f) == 7 && qtrain_exponent_host(127.0f) == 0 && qtrain_exponent_host(127.5f) == -1);
    // s within rounding of a power of two from below: m just above 127 / 16; the field keeps e = 3
    const float m = std::nextafter(127.0f / 16.0f, 100.0f);
    EXPECT(127.0f / m < 16.0f && qtrain_exponent_host(m) == 3);
    // against floor(log2) in double on a sweep of ordinary maxima (no power of two of s among them)
    unsigned int r = 12345u;
    for (int i = 0; i < 20000; ++i) {
        r = r * 1664525u + 1013904223u;
        const float v = std::ldexp(1.0f + (float)(r >> 9) / 8388608.0f, (int)(r % 41) - 20);
        const float s = 127.0f / v;
        EXPECT(qtrain_exponent_host(v) == (int)std::floor(std::log2((double)s)));
    }
}

int main() {
    check_rules();
    check_exponent_rule();
    const int n = check_all_or_none(64, 96, 2, 5, 2);
    check_all_or_none(32, 16, 20, 5, 1);
    check_refusals_and_sizes();
    if (failures) {
        std::printf("qtrain_host_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("qtrain_host_check ok (%d allocations per handle)\n", n);
    return 0;
}
