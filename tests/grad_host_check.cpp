// The host side of libyolo355_grad.so on the CPU under the address and undefined-behaviour sanitizers
// (make -C csrc hostcheck-grad): the rules of a configuration (y355_grad_create's device-free half), the handle's buffers --
// all of them or none -- under an allocator that fails at every allocation in turn, and every refusal the entry points make
// before a device call, on a handle whose "device" memory is the host heap.  A stand-alone program; needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../include/yolo355_grad.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/y355_host.h"

static std::string g_text;
int y355_fail(int code, const std::string &msg) {      // the library's own is left out under -DY355_HOSTCHECK
    g_text = msg;
    return code;
}

// grad.hip's two halves of a create and what goes with them (the struct stays the library's)
int grad_open(const y355_loss_config *cfg, const DevMem &mem, y355_grad **out);
int grad_buffers(y355_grad *h);
DevOwner &grad_owner(y355_grad *h);
void grad_free(y355_grad *h);

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
static size_t live_bytes = 0;
static int fail_at = -1, allocs_seen = 0;
static DevMem host_mem() {
    DevMem m;
    m.alloc = [](void **p, size_t bytes, bool zero) {
        if (allocs_seen++ == fail_at) return y355_fail(Y355_EHIP, "allocation refused");
        *p = zero ? std::calloc(1, bytes ? bytes : 16) : std::malloc(bytes ? bytes : 16);
        live.insert(*p);
        live_bytes += bytes;
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

static y355_loss_config config(int levels) {
    y355_loss_config c;
    std::memset(&c, 0, sizeof(c));
    c.num_levels = levels;
    c.num_anchors = 3;
    c.num_classes = 20;
    c.in_h = c.in_w = 64;
    for (int l = 0; l < levels; ++l) {
        c.stride[l] = 8 << l;
        c.hs[l] = c.ws[l] = 64 / c.stride[l];
    }
    for (int i = 0; i < 2 * levels * 3; ++i) c.anchors[i] = 4.0 + 3.0 * i;
    c.wh_mul = 1.0f;
    c.anchors_in_grid_units = 0;
    c.ignore_thresh = 0.5;
    c.obj_weight = 5.0;
    c.noobj_weight = 1.0;
    c.max_batch = 4;
    c.max_labels_per_image = 3;
    return c;
}

template <typename F>
static void refused_config(const char *text, int levels, F change) {
    y355_loss_config c = config(levels);
    change(c);
    y355_grad *h = (y355_grad *)16;
    g_text.clear();
    const int rc = grad_open(&c, host_mem(), &h);
    if (rc != Y355_GRAD_EINVAL || h || g_text.find(text) == std::string::npos || !live.empty()) {
        std::printf("expected a configuration refused with \"%s\", got %d \"%s\"\n", text, rc, g_text.c_str());
        ++failures;
    }
}

static void check_rules() {
    y355_grad *h = nullptr;
    y355_loss_config c = config(1);
    EXPECT(grad_open(nullptr, host_mem(), &h) == Y355_GRAD_EINVAL && g_text == "y355_grad_create: null argument");
    EXPECT(grad_open(&c, host_mem(), nullptr) == Y355_GRAD_EINVAL && g_text == "y355_grad_create: null argument");
    refused_config("device_id < 0", 1, [](y355_loss_config &c) { c.device_id = -1; });
    refused_config("num_levels must be 1..3", 1, [](y355_loss_config &c) { c.num_levels = 4; });
    refused_config("num_levels must be 1..3", 1, [](y355_loss_config &c) { c.num_levels = 0; });
    refused_config("num_anchors must be 1..16", 1, [](y355_loss_config &c) { c.num_anchors = 17; });
    refused_config("num_classes must be 1..4096", 1, [](y355_loss_config &c) { c.num_classes = 0; });
    refused_config("num_classes must be 1..4096", 1, [](y355_loss_config &c) { c.num_classes = 4097; });
    refused_config("in_h / in_w", 1, [](y355_loss_config &c) { c.in_w = 0; });
    refused_config("wh_mul must be finite and > 0", 1, [](y355_loss_config &c) { c.wh_mul = 0.f; });
    refused_config("wh_mul must be finite and > 0", 1, [](y355_loss_config &c) { c.wh_mul = NAN; });
    refused_config("one level only", 2, [](y355_loss_config &c) { c.anchors_in_grid_units = 1; });
    refused_config("must be finite", 1, [](y355_loss_config &c) { c.obj_weight = INFINITY; });
    refused_config("must be finite", 1, [](y355_loss_config &c) { c.ignore_thresh = NAN; });
    refused_config("max_batch must be 1..65535", 1, [](y355_loss_config &c) { c.max_batch = 0; });
    refused_config("max_labels_per_image must be 1..2^20", 1, [](y355_loss_config &c) { c.max_labels_per_image = 0; });
    refused_config("hs / ws must be 1..4096", 3, [](y355_loss_config &c) { c.ws[2] = 0; });
    refused_config("stride must be >= 1", 2, [](y355_loss_config &c) { c.stride[1] = 0; });
    refused_config("anchor sizes must be finite and > 0", 3, [](y355_loss_config &c) { c.anchors[17] = 0.0; });
    refused_config("exceed 2^31 elements", 3, [](y355_loss_config &c) {
        c.num_anchors = 16;
        c.num_classes = 4096;
        for (int l = 0; l < 3; ++l) c.hs[l] = c.ws[l] = 4096;
        for (int i = 0; i < 96; ++i) c.anchors[i] = 1.0;
    });
    refused_config("exceeds 2^26", 1, [](y355_loss_config &c) {
        c.max_batch = 65535;
        c.max_labels_per_image = 1 << 20;
    });
}

// the six arrays of a handle: all of them, or after a refusal at any of them none; the sizes are the loss library's
static void check_buffers(int levels) {
    const y355_loss_config c = config(levels);
    size_t N = 0;
    for (int l = 0; l < levels; ++l) N += (size_t)c.hs[l] * c.ws[l] * c.num_anchors;
    const size_t nblk = std::min<size_t>((N + 255) / 256, 32), mb = c.max_batch, ml = c.max_labels_per_image;
    const size_t want = mb * N * 11 * 4 + mb * ml * 5 * 8 + (mb + 1) * 4 + mb * nblk * 5 * 8 + mb * 5 * 8 + 4 * 8;
    for (int k = -1; k < 6; ++k) {
        y355_grad *h = nullptr;
        fail_at = -1;
        EXPECT(grad_open(&c, host_mem(), &h) == 0 && h && live.empty() && y355_grad_num_anchors_total(h) == (int)N);
        fail_at = k;
        allocs_seen = 0;
        live_bytes = 0;
        const int rc = grad_buffers(h);
        if (k < 0) {
            EXPECT(rc == 0 && live.size() == 6 && grad_owner(h).allocs.size() == 6 && live_bytes == want && allocs_seen == 6);
        } else {
            EXPECT(rc == Y355_EHIP && g_text == "allocation refused" && live.empty() && grad_owner(h).allocs.empty() && allocs_seen == k + 1);
        }
        fail_at = -1;
        grad_free(h);
        EXPECT(live.empty());
    }
}

static void refused(int rc, int code, const char *text) {
    if (rc != code || g_text.find(text) == std::string::npos) {
        std::printf("expected %d with \"%s\", got %d \"%s\"\n", code, text, rc, g_text.c_str());
        ++failures;
    }
    g_text.clear();
}

// every refusal of the entry points comes before a device call: this program has no device
static void check_refusals() {
    const y355_loss_config c = config(2);
    y355_grad *h = nullptr;
    fail_at = -1;
    EXPECT(grad_open(&c, host_mem(), &h) == 0 && grad_buffers(h) == 0);
    float word = 0.f;
    const void *pred[2] = {&word, &word}, *pred_hole[2] = {&word, nullptr};
    void *grad[2] = {&word, &word}, *grad_hole[2] = {nullptr, &word};
    double out[4], parts[20];
    const int32_t off[3] = {0, 1, 2}, off_bad0[3] = {1, 1, 2}, off_dec[3] = {0, 2, 1}, off_many[3] = {0, 4, 4};
    const double lab[10] = {0.1, 0.1, 0.5, 0.5, 3, 0.2, 0.2, 0.9, 0.9, 19};

    EXPECT(y355_grad_num_anchors_total(nullptr) == Y355_GRAD_EINVAL);
    y355_grad_destroy(nullptr);
    refused(y355_grad_set_labels(nullptr, off, lab, 2), Y355_GRAD_EINVAL, "y355_grad_set_labels: null argument");
    refused(y355_grad_set_labels(h, nullptr, lab, 2), Y355_GRAD_EINVAL, "y355_grad_set_labels: null argument");
    refused(y355_grad_set_labels(h, off, lab, 0), Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    refused(y355_grad_set_labels(h, off, lab, 5), Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    refused(y355_grad_set_labels(h, off_bad0, lab, 2), Y355_GRAD_EINVAL, "offsets[0] must be 0");
    refused(y355_grad_set_labels(h, off_dec, lab, 2), Y355_GRAD_EINVAL, "offsets must not decrease");
    refused(y355_grad_set_labels(h, off_many, lab, 2), Y355_GRAD_EINVAL, "image 0 has 4 labels, max_labels_per_image is 3");
    refused(y355_grad_set_labels(h, off, nullptr, 2), Y355_GRAD_EINVAL, "y355_grad_set_labels: null labels");
    auto bad_label = [&](int i, double v, const char *text) {
        double l2[10];
        std::memcpy(l2, lab, sizeof(lab));
        l2[i] = v;
        refused(y355_grad_set_labels(h, off, l2, 2), Y355_GRAD_EINVAL, text);
    };
    bad_label(1, NAN, "label 0: non-finite value");
    bad_label(7, 1.5, "label 1: coordinate outside [0, 1]");
    bad_label(5, -0.1, "label 1: coordinate outside [0, 1]");
    bad_label(4, 20, "label 0: class outside 0..19");
    bad_label(9, -1, "label 1: class outside 0..19");

    const void *t = &word;
    refused(y355_grad_targets_dev(nullptr, 1, &t), Y355_GRAD_EINVAL, "y355_grad_targets_dev: null argument");
    refused(y355_grad_targets_dev(h, 1, nullptr), Y355_GRAD_EINVAL, "y355_grad_targets_dev: null argument");
    refused(y355_grad_targets_dev(h, 1, &t), Y355_GRAD_ENOTREADY, "y355_grad_targets_dev: no labels set");
    EXPECT(t == nullptr);

    refused(y355_grad_forward_backward(nullptr, pred, &word, 1, nullptr, grad, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_forward_backward: null argument");
    refused(y355_grad_forward_backward(h, nullptr, &word, 1, nullptr, grad, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_forward_backward: null argument");
    refused(y355_grad_forward_backward(h, pred, &word, 1, nullptr, grad, nullptr, nullptr, parts), Y355_GRAD_EINVAL, "y355_grad_forward_backward: null argument");
    refused(y355_grad_forward_backward(h, pred, &word, 0, nullptr, grad, nullptr, out, parts), Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    refused(y355_grad_forward_backward(h, pred, &word, 5, nullptr, grad, nullptr, out, parts), Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    refused(y355_grad_forward_backward(h, pred_hole, &word, 1, nullptr, grad, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_forward_backward: null prediction map");
    refused(y355_grad_forward_backward(h, pred, &word, 1, nullptr, grad_hole, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_forward_backward: null gradient map");
    refused(y355_grad_forward_backward(h, pred, nullptr, 1, nullptr, grad, nullptr, out, parts), Y355_GRAD_ENOTREADY, "y355_grad_forward_backward: no labels set and no target given");

    refused(y355_grad_backward(nullptr, pred, &word, 1, nullptr, grad, nullptr), Y355_GRAD_EINVAL, "y355_grad_backward: null argument");
    refused(y355_grad_backward(h, nullptr, &word, 1, nullptr, grad, nullptr), Y355_GRAD_EINVAL, "y355_grad_backward: null argument");
    refused(y355_grad_backward(h, pred, &word, 1, nullptr, nullptr, nullptr), Y355_GRAD_EINVAL, "y355_grad_backward: null argument");
    refused(y355_grad_backward(h, pred, &word, 5, nullptr, grad, nullptr), Y355_GRAD_EINVAL, "batch must be 1..max_batch");
    refused(y355_grad_backward(h, pred_hole, &word, 1, nullptr, grad, nullptr), Y355_GRAD_EINVAL, "y355_grad_backward: null prediction map");
    refused(y355_grad_backward(h, pred, &word, 1, nullptr, grad_hole, nullptr), Y355_GRAD_EINVAL, "y355_grad_backward: null gradient map");
    refused(y355_grad_backward(h, pred, nullptr, 1, nullptr, grad, nullptr), Y355_GRAD_ENOTREADY, "y355_grad_backward: no labels set and no target given");

    void *w = &word;
    refused(y355_grad_flat(-1, w, w, w, w, 1, 1, 1, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_flat: null argument");
    refused(y355_grad_flat(0, w, nullptr, w, w, 1, 1, 1, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_flat: null argument");
    refused(y355_grad_flat(0, w, w, w, nullptr, 1, 1, 1, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_flat: null argument");
    refused(y355_grad_flat(0, w, w, w, w, 1, 1, 1, 5, 1, nullptr, w, nullptr, w, nullptr, out, parts), Y355_GRAD_EINVAL, "all three gradient tensors or none");
    refused(y355_grad_flat(0, w, w, w, w, 1, 1, 1, 5, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), Y355_GRAD_EINVAL, "neither out nor gradient tensors");
    refused(y355_grad_flat(0, w, w, w, w, 1, 1, 1, 5, 1, nullptr, w, w, w, nullptr, nullptr, parts), Y355_GRAD_EINVAL, "per_image without out");
    refused(y355_grad_flat(0, w, w, w, w, 0, 1, 1, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_flat: batch must be 1..65535");
    refused(y355_grad_flat(0, w, w, w, w, 1, 0, 1, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "num_anchors_total >= 1");
    refused(y355_grad_flat(0, w, w, w, w, 1, 1, 4097, 5, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "num_classes 1..4096");
    refused(y355_grad_flat(0, w, w, w, w, 1, 1, 1, NAN, 1, nullptr, w, w, w, nullptr, out, parts), Y355_GRAD_EINVAL, "y355_grad_flat: weights must be finite");
    grad_free(h);
    EXPECT(live.empty());
}

int main() {
    check_rules();
    for (int levels = 1; levels <= 3; ++levels) check_buffers(levels);
    check_refusals();
    if (failures) {
        std::printf("grad_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("grad_host_check ok\n");
    return 0;
}
