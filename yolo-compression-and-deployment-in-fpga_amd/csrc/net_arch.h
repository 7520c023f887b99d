// yolo355 -- the op tables of the five y355_net graphs (net.hip): tensors, ops and weight slots in forward order
#pragma once
#include <vector>

namespace {
enum { OP_CONV1 = 0, OP_CONV, OP_POOL, OP_UPSAMPLE, OP_INPUT, OP_REORG, OP_SPP };
enum { ACT_NONE = 0, ACT_L125, ACT_L100 };     // LeakyReLU(0.125) utils/modules.py:15; (0.1) backbone/darknet.py:18

struct TensorDef { int C, div, pred; };        // channels; H = height / div; pred: prediction map (no halo)
struct OpDef {
    int type, in, out;
    int choff;        // first channel written in `out` (concat by construction)
    int layer;        // weight slot
    int cin, cout;    // cout 0 = A * (5 + C); cin may be a leading channel range of a wider (concat) buffer
    int ksize, pool, act;
    int stride2;      // 1: 3x3 / pad 1 / stride 2 (backbone/darknet.py:124-141)
    int res1;         // residual tensor + 1 added after the activation (darknet.py:36), 0 = none
};
struct ArchDef { int ntensors; const TensorDef *t; int nops; const OpDef *ops; int nlayers; int nlev; int pred_t[3]; float stride[3]; };

// ---- SlimYOLOv2 (models/slim_yolo_v2.py:403-419, 551-567)
const TensorDef kSlimT[] = {{16, 2, 0}, {32, 4, 0}, {64, 4, 0}, {64, 8, 0}, {128, 8, 0}, {128, 16, 0},
                            {256, 16, 0}, {256, 16, 0}, {256, 16, 0}, {0, 16, 1}};
const OpDef kSlimOps[] = {
    {OP_CONV1, -1, 0, 0, 0, 3, 16, 3, 1, ACT_L125},
    {OP_CONV, 0, 1, 0, 1, 16, 32, 3, 1, ACT_L125},
    {OP_CONV, 1, 2, 0, 2, 32, 64, 3, 0, ACT_L125},
    {OP_CONV, 2, 3, 0, 3, 64, 64, 3, 1, ACT_L125},
    {OP_CONV, 3, 4, 0, 4, 64, 128, 3, 0, ACT_L125},
    {OP_CONV, 4, 5, 0, 5, 128, 128, 3, 1, ACT_L125},
    {OP_CONV, 5, 6, 0, 6, 128, 256, 3, 0, ACT_L125},
    {OP_CONV, 6, 7, 0, 7, 256, 256, 3, 0, ACT_L125},
    {OP_CONV, 7, 8, 0, 8, 256, 256, 3, 0, ACT_L125},
    {OP_CONV, 8, 9, 0, 9, 256, 0, 3, 0, ACT_NONE},
};
// ---- YOLOv3tiny (backbone/darknet.py:215-253, models/tiny_yolo_v3.py:27-39, 176-200)
// tensor 4 is the concat buffer [C_4 (256) | up(conv_1x1_2(C_5)) (128)] (:190)
const TensorDef kTinyT[] = {{16, 2, 0}, {32, 4, 0}, {64, 8, 0}, {128, 16, 0}, {384, 16, 0}, {256, 32, 0}, {512, 32, 0},
                            {512, 32, 0}, {1024, 32, 0}, {256, 32, 0}, {128, 32, 0}, {256, 16, 0}, {512, 32, 0},
                            {0, 16, 1}, {0, 32, 1}};
const OpDef kTinyOps[] = {
    {OP_CONV1, -1, 0, 0, 0, 3, 16, 3, 1, ACT_L100},        // conv_1 + maxpool_1
    {OP_CONV, 0, 1, 0, 1, 16, 32, 3, 1, ACT_L100},         // conv_2 + maxpool_2
    {OP_CONV, 1, 2, 0, 2, 32, 64, 3, 1, ACT_L100},         // conv_3 + maxpool_3
    {OP_CONV, 2, 3, 0, 3, 64, 128, 3, 1, ACT_L100},        // conv_4 + maxpool_4
    {OP_CONV, 3, 4, 0, 4, 128, 256, 3, 0, ACT_L100},       // conv_5 = C_4
    {OP_POOL, 4, 5, 0, -1, 256, 256, 2, 0, 0},             // maxpool_5 (2x2, stride 2)
    {OP_CONV, 5, 6, 0, 5, 256, 512, 3, 0, ACT_L100},       // conv_6
    {OP_POOL, 6, 7, 0, -1, 512, 512, 2, 1, 0},             // maxpool_6: ZeroPad2d((0,1,0,1)) + MaxPool(2, 1)
    {OP_CONV, 7, 8, 0, 6, 512, 1024, 3, 0, ACT_L100},      // conv_7 = C_5
    {OP_CONV, 8, 9, 0, 7, 1024, 256, 3, 0, ACT_L125},      // conv_set_2
    {OP_CONV, 9, 10, 0, 8, 256, 128, 1, 0, ACT_L125},      // conv_1x1_2
    {OP_UPSAMPLE, 10, 4, 256, -1, 128, 128, 0, 0, 0},      // bilinear x2, align_corners (:188)
    {OP_CONV, 4, 11, 0, 9, 384, 256, 3, 0, ACT_L125},      // conv_set_1
    {OP_CONV, 9, 12, 0, 10, 256, 512, 3, 0, ACT_L125},     // extra_conv_2
    {OP_CONV, 12, 14, 0, 11, 512, 0, 1, 0, ACT_NONE},      // pred_2 (stride 32)
    {OP_CONV, 11, 13, 0, 12, 256, 0, 1, 0, ACT_NONE},      // pred_1 (stride 16)
};
// ---- myYOLOv2 (models/yolo_v2.py:26-39, 165-179) on DarkNet-19 (backbone/darknet.py:40-110)
const TensorDef kV2T[] = {
    {3, 1, 0},                                                   //  0 input: bf16 NHWC16 / int8 NHWC32
    {32, 2, 0}, {64, 4, 0},                                      //  1 conv_1+pool, 2 conv_2+pool
    {128, 4, 0}, {64, 4, 0}, {128, 8, 0},                        //  3..5 conv_3 (last pooled)
    {256, 8, 0}, {128, 8, 0}, {256, 8, 0}, {256, 16, 0},         //  6..8 conv_4 (8 = C_4), 9 maxpool_4
    {512, 16, 0}, {256, 16, 0}, {512, 16, 0}, {256, 16, 0}, {512, 16, 0},   // 10..14 conv_5 (14 = C_5)
    {512, 32, 0},                                                // 15 maxpool_5
    {1024, 32, 0}, {512, 32, 0}, {1024, 32, 0}, {512, 32, 0}, {1024, 32, 0},   // 16..20 conv_6 (20 = C_6)
    {1024, 32, 0},                                               // 21 convsets_1[0]
    {64, 16, 0},                                                 // 22 route_layer
    {1280, 32, 0},                                               // 23 cat(reorg(route) [0:256), convsets_1 [256:1280))
    {1024, 32, 0},                                               // 24 convsets_2
    {0, 32, 1},                                                  // 25 pred
};
const OpDef kV2Ops[] = {
    {OP_INPUT, -1, 0, 0, -1, 3, 3, 0, 0, 0},
    {OP_CONV, 0, 1, 0, 0, 3, 32, 3, 1, ACT_L100},
    {OP_CONV, 1, 2, 0, 1, 32, 64, 3, 1, ACT_L100},
    {OP_CONV, 2, 3, 0, 2, 64, 128, 3, 0, ACT_L100},
    {OP_CONV, 3, 4, 0, 3, 128, 64, 1, 0, ACT_L100},
    {OP_CONV, 4, 5, 0, 4, 64, 128, 3, 1, ACT_L100},
    {OP_CONV, 5, 6, 0, 5, 128, 256, 3, 0, ACT_L100},
    {OP_CONV, 6, 7, 0, 6, 256, 128, 1, 0, ACT_L100},
    {OP_CONV, 7, 8, 0, 7, 128, 256, 3, 0, ACT_L100},
    {OP_POOL, 8, 9, 0, -1, 256, 256, 2, 0, 0},
    {OP_CONV, 9, 10, 0, 8, 256, 512, 3, 0, ACT_L100},
    {OP_CONV, 10, 11, 0, 9, 512, 256, 1, 0, ACT_L100},
    {OP_CONV, 11, 12, 0, 10, 256, 512, 3, 0, ACT_L100},
    {OP_CONV, 12, 13, 0, 11, 512, 256, 1, 0, ACT_L100},
    {OP_CONV, 13, 14, 0, 12, 256, 512, 3, 0, ACT_L100},
    {OP_POOL, 14, 15, 0, -1, 512, 512, 2, 0, 0},
    {OP_CONV, 15, 16, 0, 13, 512, 1024, 3, 0, ACT_L100},
    {OP_CONV, 16, 17, 0, 14, 1024, 512, 1, 0, ACT_L100},
    {OP_CONV, 17, 18, 0, 15, 512, 1024, 3, 0, ACT_L100},
    {OP_CONV, 18, 19, 0, 16, 1024, 512, 1, 0, ACT_L100},
    {OP_CONV, 19, 20, 0, 17, 512, 1024, 3, 0, ACT_L100},
    {OP_CONV, 20, 21, 0, 18, 1024, 1024, 3, 0, ACT_L125},        // convsets_1[0]
    {OP_CONV, 21, 23, 256, 19, 1024, 1024, 3, 0, ACT_L125},      // convsets_1[1] -> cat[256:1280)
    {OP_CONV, 14, 22, 0, 20, 512, 64, 1, 0, ACT_L125},           // route_layer on C_5
    {OP_REORG, 22, 23, 0, -1, 64, 256, 2, 0, 0},                 // reorg(stride 2) -> cat[0:256)
    {OP_CONV, 23, 24, 0, 21, 1280, 1024, 3, 0, ACT_L125},        // convsets_2
    {OP_CONV, 24, 25, 0, 22, 1024, 0, 1, 0, ACT_NONE},           // pred (1x1)
};
// ---- myYOLOv3 / myYOLOv3Spp (models/yolo_v3.py:26-61, 203-231; models/yolo_v3_spp.py:31-36) on DarkNet-53
// (backbone/darknet.py:112-161): built programmatically, weight slots in forward order
struct V3Graph {
    std::vector<TensorDef> t;
    std::vector<OpDef> ops;
    int nlayers = 0;
    int pred[3] = {0, 0, 0};
    int T(int C, int div, int pred_ = 0) { t.push_back(TensorDef{C, div, pred_}); return (int)t.size() - 1; }
    void conv(int in, int out, int choff, int cin, int cout, int k, int act, int stride2 = 0, int res = -1) {
        ops.push_back(OpDef{OP_CONV, in, out, choff, nlayers++, cin, cout, k, 0, act, stride2, res + 1});
    }
    // resblock(ch) x n on tensor x (div d); the last block may write into `last_out` (a concat buffer, channel offset 0)
    int resblocks(int x, int ch, int d, int n, int last_out = -1) {
        for (int i = 0; i < n; ++i) {
            const int mid = T(ch / 2 < 64 ? 64 : ch / 2, d);                 // >= 64 channels: the kernels write 64-channel blocks
            conv(x, mid, 0, ch, ch / 2, 1, ACT_L100);
            const int out = (i == n - 1 && last_out >= 0) ? last_out : T(ch, d);
            conv(mid, out, 0, ch / 2, ch, 3, ACT_L100, 0, x);
            x = out;
        }
        return x;
    }
    explicit V3Graph(bool spp) {
        const int in = T(3, 1);
        ops.push_back(OpDef{OP_INPUT, -1, in, 0, -1, 3, 3, 0, 0, 0, 0, 0});
        int x = T(64, 1);                                                   // 32 real channels
        conv(in, x, 0, 3, 32, 3, ACT_L100);
        int y = T(64, 2);
        conv(x, y, 0, 32, 64, 3, ACT_L100, 1);
        x = resblocks(y, 64, 2, 1);
        y = T(128, 4); conv(x, y, 0, 64, 128, 3, ACT_L100, 1);
        x = resblocks(y, 128, 4, 2);
        y = T(256, 8); conv(x, y, 0, 128, 256, 3, ACT_L100, 1);
        const int cat1 = T(384, 8);                                          // [C_3 (256) | up(conv_1x1_2) (128)]
        const int c3 = resblocks(y, 256, 8, 8, cat1);
        y = T(512, 16); conv(c3, y, 0, 256, 512, 3, ACT_L100, 1);
        const int cat2 = T(768, 16);                                         // [C_4 (512) | up(conv_1x1_3) (256)]
        const int c4 = resblocks(y, 512, 16, 8, cat2);
        y = T(1024, 32); conv(c4, y, 0, 512, 1024, 3, ACT_L100, 1);
        int c5;
        if (spp) {
            const int sppb = T(4096, 32);                                    // [C_5 | pool5 | pool9 | pool13]
            c5 = resblocks(y, 1024, 32, 4, sppb);
            ops.push_back(OpDef{OP_SPP, c5, c5, 1024, -1, 1024, 3072, 0, 0, 0, 0, 0});
        } else {
            c5 = resblocks(y, 1024, 32, 4);
        }
        // conv_set_3
        int a = T(512, 32); conv(c5, a, 0, spp ? 4096 : 1024, 512, 1, ACT_L125);
        int b = T(1024, 32); conv(a, b, 0, 512, 1024, 3, ACT_L125);
        a = T(512, 32); conv(b, a, 0, 1024, 512, 1, ACT_L125);
        b = T(1024, 32); conv(a, b, 0, 512, 1024, 3, ACT_L125);
        const int f3 = T(512, 32); conv(b, f3, 0, 1024, 512, 1, ACT_L125);
        a = T(256, 32); conv(f3, a, 0, 512, 256, 1, ACT_L125);               // conv_1x1_3
        ops.push_back(OpDef{OP_UPSAMPLE, a, cat2, 512, -1, 256, 256, 0, 0, 0, 0, 0});
        // conv_set_2
        a = T(256, 16); conv(cat2, a, 0, 768, 256, 1, ACT_L125);
        b = T(512, 16); conv(a, b, 0, 256, 512, 3, ACT_L125);
        a = T(256, 16); conv(b, a, 0, 512, 256, 1, ACT_L125);
        b = T(512, 16); conv(a, b, 0, 256, 512, 3, ACT_L125);
        const int f2 = T(256, 16); conv(b, f2, 0, 512, 256, 1, ACT_L125);
        a = T(128, 16); conv(f2, a, 0, 256, 128, 1, ACT_L125);               // conv_1x1_2
        ops.push_back(OpDef{OP_UPSAMPLE, a, cat1, 256, -1, 128, 128, 0, 0, 0, 0, 0});
        // conv_set_1
        a = T(128, 8); conv(cat1, a, 0, 384, 128, 1, ACT_L125);
        b = T(256, 8); conv(a, b, 0, 128, 256, 3, ACT_L125);
        a = T(128, 8); conv(b, a, 0, 256, 128, 1, ACT_L125);
        b = T(256, 8); conv(a, b, 0, 128, 256, 3, ACT_L125);
        const int f1 = T(128, 8); conv(b, f1, 0, 256, 128, 1, ACT_L125);
        // heads: extra_conv_3 + pred_3, extra_conv_2 + pred_2, extra_conv_1 + pred_1 (models/yolo_v3.py:219-231)
        a = T(1024, 32); conv(f3, a, 0, 512, 1024, 3, ACT_L125);
        pred[2] = T(0, 32, 1); conv(a, pred[2], 0, 1024, 0, 1, ACT_NONE);
        a = T(512, 16); conv(f2, a, 0, 256, 512, 3, ACT_L125);
        pred[1] = T(0, 16, 1); conv(a, pred[1], 0, 512, 0, 1, ACT_NONE);
        a = T(256, 8); conv(f1, a, 0, 128, 256, 3, ACT_L125);
        pred[0] = T(0, 8, 1); conv(a, pred[0], 0, 256, 0, 1, ACT_NONE);
    }
    ArchDef arch() const {
        return ArchDef{(int)t.size(), t.data(), (int)ops.size(), ops.data(), nlayers, 3, {pred[0], pred[1], pred[2]}, {8.f, 16.f, 32.f}};
    }
};
const V3Graph kV3(false), kV3Spp(true);
const ArchDef kArch[5] = {
    {10, kSlimT, 10, kSlimOps, 10, 1, {9, -1, -1}, {16.f, 0.f, 0.f}},
    {15, kTinyT, 16, kTinyOps, 13, 2, {13, 14, -1}, {16.f, 32.f, 0.f}},
    {26, kV2T, 27, kV2Ops, 23, 1, {25, -1, -1}, {32.f, 0.f, 0.f}},
    kV3.arch(),
    kV3Spp.arch(),
};
}  // namespace
