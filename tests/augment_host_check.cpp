// The host side of libyolo355_augment.so on the CPU under the address and undefined-behaviour sanitizers
// (make -C csrc hostcheck-augment): y355_augment_check's refusals, and the table expressions the kernel computes inline
// (csrc/augment_tables.h) on a sweep of sizes -- every index inside its axis, every fraction in [0, 1), the horizontal
// clamp-and-zero rule, the vertical clip-the-row-indices rule, what equal sizes and an exact 2x decimation give.  Needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/yolo355_augment.h"
#include "../yolo-compression-and-deployment-in-fpga_amd/csrc/augment_tables.h"

static std::string g_text;
int y355_fail(int code, const std::string &msg) {      // the library's own is left out under -DY355_HOSTCHECK
    g_text = msg;
    return code;
}

static int failures = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static void sweep_axis(int src, int dst) {
    const double scale = (double)src / (double)dst;
    int prev = 0;
    for (int vertical = 0; vertical < 2; ++vertical) {
        prev = 0;
        for (int d = 0; d < dst; ++d) {
            const AugTap t = y355_aug_tap(d, src, dst, vertical != 0);
            EXPECT(t.i0 >= 0 && t.i0 < src && t.i1 >= 0 && t.i1 < src);
            EXPECT(t.c1 >= 0.f && t.c1 < 1.f && t.c0 == 1.f - t.c1);
            EXPECT(t.i0 >= prev && (t.i1 == t.i0 || t.i1 == t.i0 + 1));
            prev = t.i0;
            float f = (float)((d + 0.5) * scale - 0.5);
            const int s = (int)std::floor(f);
            f -= (float)s;
            if (vertical) {
                EXPECT(!t.single && t.c1 == f);                         // the fraction is kept at the borders
                EXPECT(t.i0 == std::min(std::max(s, 0), src - 1) && t.i1 == std::min(std::max(s + 1, 0), src - 1));
            } else {
                EXPECT(t.single == (std::max(s, 0) >= src - 1));        // OpenCV tests s + 1 >= width after the left clamp
                if (s < 0 || s >= src - 1) EXPECT(t.c1 == 0.f && t.c0 == 1.f && t.i0 == (s < 0 ? 0 : src - 1));
                else EXPECT(t.c1 == f && t.i0 == s && t.i1 == s + 1);
                if (t.single) EXPECT(t.i1 == t.i0);
            }
            if (src == dst) EXPECT(t.i0 == d && t.c1 == 0.f);           // equal sizes: the tables alone already copy
            if (src == 2 * dst && !vertical) EXPECT(t.i0 == 2 * d && t.c1 == 0.5f);
        }
    }
}

static y355_augment_frame frame(const void *p, int h, int w, long long pitch) {
    y355_augment_frame f;
    f.data_dev = p;
    f.height = h;
    f.width = w;
    f.row_bytes = pitch;
    return f;
}

static y355_augment_params params(int vh, int vw) {
    y355_augment_params p;
    std::memset(&p, 0, sizeof(p));
    p.contrast = p.saturation = 1.f;
    p.vh = vh;
    p.vw = vw;
    return p;
}

static void refused(const char *text, const y355_augment_frame *f, const y355_augment_params *p, int n, int dh, int dw, const float *mean,
                    const float *sd) {
    g_text.clear();
    const int rc = y355_augment_check(f, p, n, dh, dw, mean, sd);
    if (rc != Y355_AUGMENT_EINVAL || g_text.find(text) == std::string::npos) {
        std::printf("expected a refusal with \"%s\", got %d \"%s\"\n", text, rc, g_text.c_str());
        ++failures;
    }
}

int main() {
    const int sizes[][4] = {{1, 1, 32, 64}, {64, 48, 32, 64}, {5, 7, 32, 64}, {37, 53, 32, 64}, {37, 53, 64, 32}, {32, 64, 32, 64}, {64, 128, 32, 64},
                            {375, 500, 416, 416}, {1500, 2000, 416, 416}, {112, 150, 416, 416}, {16384, 16384, 1, 1}, {1, 1, 16384, 3}, {3, 2, 5, 7}};
    for (const auto &s : sizes) {
        sweep_axis(s[0], s[2]);
        sweep_axis(s[1], s[3]);
    }
    for (int src = 1; src <= 40; ++src)
        for (int dst = 1; dst <= 40; ++dst) sweep_axis(src, dst);

    int32_t fb = 0, pb = 0;
    EXPECT(y355_augment_abi(&fb, &pb) >= 1 && fb == (int32_t)sizeof(y355_augment_frame) && pb == (int32_t)sizeof(y355_augment_params));
    EXPECT(y355_augment_abi(nullptr, nullptr) >= 1);

    const float mean[3] = {0.406f, 0.456f, 0.485f}, sd[3] = {0.225f, 0.224f, 0.229f};
    std::vector<unsigned char> px(64 * 48 * 3, 7);
    std::vector<y355_augment_frame> f = {frame(px.data(), 1, 1, 0), frame(px.data(), 64, 48, 0), frame(px.data(), 48, 60, 192)};
    std::vector<y355_augment_params> p = {params(1, 1), params(70, 50), params(3, 9)};
    p[1].oy = -5;
    p[1].ox = 12;
    p[2].flags = Y355_AUG_ALL_FLAGS;
    EXPECT(y355_augment_check(f.data(), p.data(), 3, 32, 64, mean, sd) == Y355_AUGMENT_OK);
    refused("null argument", nullptr, p.data(), 3, 32, 64, mean, sd);
    refused("null argument", f.data(), nullptr, 3, 32, 64, mean, sd);
    refused("null argument", f.data(), p.data(), 3, 32, 64, nullptr, sd);
    refused("null argument", f.data(), p.data(), 3, 32, 64, mean, nullptr);
    refused("n must be >= 1", f.data(), p.data(), 0, 32, 64, mean, sd);
    refused("dst_h and dst_w", f.data(), p.data(), 3, 0, 64, mean, sd);
    refused("dst_h and dst_w", f.data(), p.data(), 3, 32, 16385, mean, sd);
    const float zero_sd[3] = {0.225f, 0.f, 0.229f}, nan_mean[3] = {0.406f, NAN, 0.485f}, inf_sd[3] = {INFINITY, 0.224f, 0.229f};
    refused("std must be finite and non-zero", f.data(), p.data(), 3, 32, 64, mean, zero_sd);
    refused("std must be finite and non-zero", f.data(), p.data(), 3, 32, 64, mean, inf_sd);
    refused("mean must be finite", f.data(), p.data(), 3, 32, 64, nan_mean, sd);
    auto with = [&](auto change, const char *text) {
        std::vector<y355_augment_frame> ff = f;
        std::vector<y355_augment_params> pp = p;
        change(ff, pp);
        refused(text, ff.data(), pp.data(), 3, 32, 64, mean, sd);
    };
    with([](auto &ff, auto &) { ff[1].data_dev = nullptr; }, "frame 1: null frame pointer");
    with([](auto &ff, auto &) { ff[2].height = 0; }, "frame 2: height and width");
    with([](auto &ff, auto &) { ff[0].width = 16385; }, "frame 0: height and width");
    with([](auto &ff, auto &) { ff[2].row_bytes = 179; }, "frame 2: row_bytes below width * 3");
    with([](auto &, auto &pp) { pp[1].vh = 0; }, "frame 1: vh and vw");
    with([](auto &, auto &pp) { pp[0].vw = 16385; }, "frame 0: vh and vw");
    with([](auto &, auto &pp) { pp[1].ox = (1 << 24) + 1; }, "frame 1: oy and ox");
    with([](auto &, auto &pp) { pp[2].flags = 128; }, "frame 2: unknown flags");
    with([](auto &, auto &pp) { pp[2].hue = NAN; }, "frame 2: brightness, contrast, saturation and hue must be finite");
    with([](auto &, auto &pp) { pp[0].brightness = INFINITY; }, "frame 0: brightness, contrast, saturation and hue must be finite");
    with([](auto &, auto &pp) { pp[1].fill[2] = NAN; }, "frame 1: fill must be finite");
    // the refusals made no device call: a run with a bad argument is refused the same way, whatever the device
    g_text.clear();
    EXPECT(y355_augment_run(0, f.data(), p.data(), 0, 32, 64, mean, sd, 1, px.data(), nullptr) == Y355_AUGMENT_EINVAL && g_text == "n must be >= 1");
    EXPECT(y355_augment_run(-1, f.data(), p.data(), 3, 32, 64, mean, sd, 1, px.data(), nullptr) == Y355_AUGMENT_EINVAL && g_text == "device_id < 0");
    EXPECT(y355_augment_run(0, f.data(), p.data(), 3, 32, 64, mean, sd, 1, nullptr, nullptr) == Y355_AUGMENT_EINVAL &&
           g_text == "y355_augment_run: null destination");
    if (failures) {
        std::printf("augment_host_check: %d failures\n", failures);
        return 1;
    }
    std::printf("augment_host_check ok\n");
    return 0;
}
