"""TEST INFRASTRUCTURE -- integer CPU restatement of the int8 form of the three DarkNet graphs of csrc/net.hip:
myYOLOv2 (kV2Ops: DarkNet-19, reorg route into a concat buffer), myYOLOv3 and myYOLOv3Spp (V3Graph: DarkNet-53 with
stride-2 convolutions and residual blocks, SPP, bilinear x2 into concat buffers, three prediction levels), under the
per-tensor power-of-two recipe of retune_bias_quantize.py:73-119.

PARITY UNPINNED by construction: the reference has no int8 form of these models, so nothing of the reference pins these
integer semantics.  They are build-defined (DESIGN.md "int8 DarkNet"), restated here from their definition independently
of the HIP code, and additionally held to the reference's fp32 maps (tests/golden/models_wide.npz) within a measured
relative L2 bound (tests/test_int8_wide_models.py).

Semantics (value = q / 2^s for a tensor of exponent s):
  input     q = clamp(RNE(x * 2^sa_in), +-127); tensor 0's exponent is sa_in
  conv      as oracle/net_int8_oracle.py: acc = sum q_a q_w (stride 1 or 2, pad k // 2); F = max(sa_in + e_w, e_b);
            t = acc * 2^(F - sa_in - e_w) + q_b * 2^(F - e_b);  t' = t >= 0 ? t * 2^lk : t * m
            (0.125: lk 3, m 1;  0.1: lk 11, m 205;  none: lk 0, m 1);  q = clamp(RNE(t' * 2^(s_out - F - lk)), +-127)
  residual  (x + block(x)) one rounding after the add: E = F + lk, G = max(E, s_r),
            u = t' * 2^(G - E) + q_r * 2^(G - s_r) exactly, q = clamp(RNE(u * 2^(s_out - G)), +-127)
  pool      2x2 / stride 2 max on q (a pooled conv pools before its clamp: it counts the clamps of its pooled outputs);
            the output takes the input's exponent
  reorg     byte permutation (out channel (sy*s + sx)*C + c), then q = clamp(RNE(q_in * 2^(s_out - s_in)), +-127)
  SPP       max-pools 5 / 9 / 13, stride 1, windows clipped to the map, on q; in place, one exponent
  upsample  oracle/net_int8_oracle.upsample_int (bilinear x2 of the integers in fp32, rescale, RNE); its clamps are not
            counted (as for YOLOv3tiny)
  A concat buffer has one exponent; every clamp of input, conv, residual and reorg counts in `sat`.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import fp32_oracle as FP
from oracle import net_int8_oracle as N
from oracle import yolo_oracle as O

L100, L125, NONE = 0.1, 0.125, None
ACT = {NONE: (0, 1), L125: (3, 1), L100: (11, 205)}


class Graph:
    """tensors: channel counts (None = prediction map) and divisors; ops: dicts in execution order"""

    def __init__(self):
        self.C, self.div, self.ops, self.pred, self.nlayers = [], [], [], [], 0

    def T(self, C, div):
        self.C.append(C)
        self.div.append(div)
        return len(self.C) - 1

    def conv(self, i, o, choff, cin, cout, k, act, pool=0, stride2=0, res=-1):
        self.ops.append(dict(op="conv", i=i, o=o, choff=choff, layer=self.nlayers, cin=cin, cout=cout, k=k, act=act,
                             pool=pool, s2=stride2, res=res))
        self.nlayers += 1

    def add(self, op, i, o, **kw):
        self.ops.append(dict(op=op, i=i, o=o, **kw))


def v2_graph():
    """kV2Ops / kV2T of csrc/net_arch.h (models/yolo_v2.py:165-179)"""
    g = Graph()
    for C, d in [(3, 1), (32, 2), (64, 4), (128, 4), (64, 4), (128, 8), (256, 8), (128, 8), (256, 8), (256, 16),
                 (512, 16), (256, 16), (512, 16), (256, 16), (512, 16), (512, 32), (1024, 32), (512, 32), (1024, 32),
                 (512, 32), (1024, 32), (1024, 32), (64, 16), (1280, 32), (1024, 32), (None, 32)]:
        g.T(C, d)
    g.add("input", -1, 0)
    g.conv(0, 1, 0, 3, 32, 3, L100, pool=1)
    g.conv(1, 2, 0, 32, 64, 3, L100, pool=1)
    g.conv(2, 3, 0, 64, 128, 3, L100)
    g.conv(3, 4, 0, 128, 64, 1, L100)
    g.conv(4, 5, 0, 64, 128, 3, L100, pool=1)
    g.conv(5, 6, 0, 128, 256, 3, L100)
    g.conv(6, 7, 0, 256, 128, 1, L100)
    g.conv(7, 8, 0, 128, 256, 3, L100)
    g.add("pool", 8, 9)
    for i, (ci, co, k) in enumerate([(256, 512, 3), (512, 256, 1), (256, 512, 3), (512, 256, 1), (256, 512, 3)]):
        g.conv(9 + i, 10 + i, 0, ci, co, k, L100)
    g.add("pool", 14, 15)
    for i, (ci, co, k) in enumerate([(512, 1024, 3), (1024, 512, 1), (512, 1024, 3), (1024, 512, 1), (512, 1024, 3)]):
        g.conv(15 + i, 16 + i, 0, ci, co, k, L100)
    g.conv(20, 21, 0, 1024, 1024, 3, L125)
    g.conv(21, 23, 256, 1024, 1024, 3, L125)
    g.conv(14, 22, 0, 512, 64, 1, L125)
    g.add("reorg", 22, 23, choff=0, s=2)
    g.conv(23, 24, 0, 1280, 1024, 3, L125)
    g.conv(24, 25, 0, 1024, None, 1, NONE)
    g.pred = [25]
    g.strides = [32]
    return g


def v3_graph(spp):
    """V3Graph of csrc/net_arch.h (models/yolo_v3.py:203-231, yolo_v3_spp.py:31-36, backbone/darknet.py:112-161)"""
    g = Graph()

    def resblocks(x, ch, d, n, last_out=-1):
        for i in range(n):
            mid = g.T(max(ch // 2, 64), d)
            g.conv(x, mid, 0, ch, ch // 2, 1, L100)
            out = last_out if (i == n - 1 and last_out >= 0) else g.T(ch, d)
            g.conv(mid, out, 0, ch // 2, ch, 3, L100, res=x)
            x = out
        return x

    inp = g.T(3, 1)
    g.add("input", -1, inp)
    x = g.T(64, 1)
    g.conv(inp, x, 0, 3, 32, 3, L100)
    y = g.T(64, 2)
    g.conv(x, y, 0, 32, 64, 3, L100, stride2=1)
    x = resblocks(y, 64, 2, 1)
    y = g.T(128, 4)
    g.conv(x, y, 0, 64, 128, 3, L100, stride2=1)
    x = resblocks(y, 128, 4, 2)
    y = g.T(256, 8)
    g.conv(x, y, 0, 128, 256, 3, L100, stride2=1)
    cat1 = g.T(384, 8)
    c3 = resblocks(y, 256, 8, 8, cat1)
    y = g.T(512, 16)
    g.conv(c3, y, 0, 256, 512, 3, L100, stride2=1)
    cat2 = g.T(768, 16)
    c4 = resblocks(y, 512, 16, 8, cat2)
    y = g.T(1024, 32)
    g.conv(c4, y, 0, 512, 1024, 3, L100, stride2=1)
    if spp:
        sppb = g.T(4096, 32)
        c5 = resblocks(y, 1024, 32, 4, sppb)
        g.add("spp", c5, c5, C=1024)
    else:
        c5 = resblocks(y, 1024, 32, 4)
    a = g.T(512, 32); g.conv(c5, a, 0, 4096 if spp else 1024, 512, 1, L125)
    b = g.T(1024, 32); g.conv(a, b, 0, 512, 1024, 3, L125)
    a = g.T(512, 32); g.conv(b, a, 0, 1024, 512, 1, L125)
    b = g.T(1024, 32); g.conv(a, b, 0, 512, 1024, 3, L125)
    f3 = g.T(512, 32); g.conv(b, f3, 0, 1024, 512, 1, L125)
    a = g.T(256, 32); g.conv(f3, a, 0, 512, 256, 1, L125)
    g.add("up", a, cat2, choff=512)
    a = g.T(256, 16); g.conv(cat2, a, 0, 768, 256, 1, L125)
    b = g.T(512, 16); g.conv(a, b, 0, 256, 512, 3, L125)
    a = g.T(256, 16); g.conv(b, a, 0, 512, 256, 1, L125)
    b = g.T(512, 16); g.conv(a, b, 0, 256, 512, 3, L125)
    f2 = g.T(256, 16); g.conv(b, f2, 0, 512, 256, 1, L125)
    a = g.T(128, 16); g.conv(f2, a, 0, 256, 128, 1, L125)
    g.add("up", a, cat1, choff=256)
    a = g.T(128, 8); g.conv(cat1, a, 0, 384, 128, 1, L125)
    b = g.T(256, 8); g.conv(a, b, 0, 128, 256, 3, L125)
    a = g.T(128, 8); g.conv(b, a, 0, 256, 128, 1, L125)
    b = g.T(256, 8); g.conv(a, b, 0, 128, 256, 3, L125)
    f1 = g.T(128, 8); g.conv(b, f1, 0, 256, 128, 1, L125)
    pred = [0, 0, 0]
    a = g.T(1024, 32); g.conv(f3, a, 0, 512, 1024, 3, L125)
    pred[2] = g.T(None, 32); g.conv(a, pred[2], 0, 1024, None, 1, NONE)
    a = g.T(512, 16); g.conv(f2, a, 0, 256, 512, 3, L125)
    pred[1] = g.T(None, 16); g.conv(a, pred[1], 0, 512, None, 1, NONE)
    a = g.T(256, 8); g.conv(f1, a, 0, 128, 256, 3, L125)
    pred[0] = g.T(None, 8); g.conv(a, pred[0], 0, 256, None, 1, NONE)
    g.pred = pred
    g.strides = [8, 16, 32]
    return g


GRAPHS = {"yolo_v2": lambda: v2_graph(), "yolo_v3": lambda: v3_graph(False), "yolo_v3_spp": lambda: v3_graph(True)}


def layers_of(model):
    """{w, b, bn} per weight slot (the drop-in's _conv_modules order) for oracle.net_int8_oracle.fold_bn"""
    out = []
    for m in model._conv_modules():
        conv = m[0] if isinstance(m, torch.nn.Sequential) else m
        w = conv.weight.detach().float().cpu().numpy()
        b = conv.bias.detach().float().cpu().numpy() if conv.bias is not None else np.zeros(w.shape[0], np.float32)
        bn = None
        if isinstance(m, torch.nn.Sequential) and len(m) > 1 and isinstance(m[1], torch.nn.BatchNorm2d):
            bn = tuple(t.detach().float().cpu().numpy() for t in (m[1].weight, m[1].bias, m[1].running_mean, m[1].running_var))
        out.append(dict(w=w, b=b, bn=bn))
    return out


def _shape(g, t, B, H, W, predc):
    return (B, predc if g.C[t] is None else g.C[t], H // g.div[t], W // g.div[t])


# ---------------------------------------------------------------------------------------------------- integer rules
def quantize_input(x, sa_in):
    r = np.rint(np.asarray(x, np.float32) * np.float32(2.0 ** sa_in))
    return np.clip(r, -127, 127).astype(np.int64), int((np.abs(r) > 127).sum())


def conv_int(q_in, q_w, stride):
    x = torch.as_tensor(q_in.astype(np.float64))
    w = torch.as_tensor(q_w.astype(np.float64))
    return F.conv2d(x, w, None, stride, w.shape[2] // 2).numpy().astype(np.int64)


def requant(acc, L, sa_in, sa_out, act, q_res=None, s_r=None):
    """the conv epilogue (with the residual when q_res is given): unclamped q, exact on int64"""
    Fb = max(sa_in + L["e_w"], L["e_b"])
    t = acc * (np.int64(1) << np.int64(Fb - sa_in - L["e_w"])) + \
        (L["q_b"].astype(np.int64) * (np.int64(1) << np.int64(Fb - L["e_b"])))[None, :, None, None]
    lk, m = ACT[act]
    tp = np.where(t >= 0, t * (np.int64(1) << np.int64(lk)), t * np.int64(m))
    E = Fb + lk
    if q_res is None:
        return O.rne_shift(tp, E - sa_out)
    G = max(E, s_r)
    bound = float(np.abs(tp).max(initial=0)) * 2.0 ** (G - E) + 127 * 2.0 ** (G - s_r)
    assert bound < 2.0 ** 62, "the residual sum leaves int64"
    u = tp * (np.int64(1) << np.int64(G - E)) + q_res.astype(np.int64) * (np.int64(1) << np.int64(G - s_r))
    return O.rne_shift(u, G - sa_out)


def residual_rule(tp, E, q_res, s_r, s_out):
    """the residual rule on given t' (int64) of exponent E: (q clamped, clamp count)"""
    G = max(E, s_r)
    u = np.asarray(tp, np.int64) * (np.int64(1) << np.int64(G - E)) + \
        np.asarray(q_res, np.int64) * (np.int64(1) << np.int64(G - s_r))
    q = O.rne_shift(u, G - s_out)
    return np.clip(q, -127, 127), int((np.abs(q) > 127).sum())


def rescale(q, d):
    """reorg's rescale q * 2^d, RNE, clamped: (q, clamp count)"""
    r = O.rne_shift(np.asarray(q, np.int64), -d)
    return np.clip(r, -127, 127), int((np.abs(r) > 127).sum())


def reorg(x, s):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // s, s, W // s, s).transpose(0, 3, 5, 1, 2, 4).reshape(B, s * s * C, H // s, W // s)


def spp_pools(x):
    """max-pools 5 / 9 / 13, stride 1, windows clipped (torch pads with -inf); works for ints and floats"""
    t = torch.as_tensor(np.asarray(x, np.float64))
    return [F.max_pool2d(t, k, 1, k // 2).numpy().astype(x.dtype) for k in (5, 9, 13)]


def pool2(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def effective_exponents(g, sa_in, sa):
    """what set_act_exponents keeps: pool outputs take their inputs' exponents, the input tensor sa_in"""
    sa = list(sa)
    for o in g.ops:
        if o["op"] == "pool":
            sa[o["o"]] = sa[o["i"]]
        elif o["op"] == "input":
            sa[o["o"]] = sa_in
    return sa


def forward_int(arch, x, qlayers, sa_in, sa, predc):
    """int8 graph: dict(t = int64 tensors in graph order (buffer channels, zero padding), sat, sa)"""
    g = GRAPHS[arch]()
    x = np.asarray(x, np.float32)
    B, _, H, W = x.shape
    sa = effective_exponents(g, sa_in, sa)
    T = [np.zeros(_shape(g, t, B, H, W, predc), np.int64) for t in range(len(g.C))]
    sat = 0
    for o in g.ops:
        i, out = o["i"], o["o"]
        if o["op"] == "input":
            q, s = quantize_input(x, sa_in)
            T[out][:, :3] = q
            sat += s
        elif o["op"] == "conv":
            L = qlayers[o["layer"]]
            acc = conv_int(T[i][:, :o["cin"]], L["q_w"], 2 if o["s2"] else 1)
            if o["res"] >= 0:
                q = requant(acc, L, sa[i], sa[out], o["act"], T[o["res"]], sa[o["res"]])
            else:
                q = requant(acc, L, sa[i], sa[out], o["act"])
            if o["pool"]:
                q = pool2(q)
            sat += int((np.abs(q) > 127).sum())
            q = np.clip(q, -127, 127)
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
        elif o["op"] == "pool":
            T[out] = pool2(T[i])
        elif o["op"] == "reorg":
            q, s = rescale(reorg(T[i], o["s"]), sa[out] - sa[i])
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
            sat += s
        elif o["op"] == "spp":
            C = o["C"]
            for k, p in enumerate(spp_pools(T[i][:, :C])):
                T[i][:, (k + 1) * C:(k + 2) * C] = p
        elif o["op"] == "up":
            up = N.upsample_int(T[i], 2.0 ** (sa[out] - sa[i]))
            T[out][:, o["choff"]:o["choff"] + up.shape[1]] = up
    return dict(t=T, sat=sat, sa=sa, pred=g.pred)


# ---------------------------------------------------------------------------------------------------- float64 graph
def forward_f64(arch, x, folded, predc):
    """the same graph in float64 on the BN-folded weights (the reference's fp32 model, evaluated exactly): tensors in
    graph order.  Calibration maxima and the fp32 yardstick of the CPU tests."""
    g = GRAPHS[arch]()
    x = np.asarray(x, np.float64)
    B, _, H, W = x.shape
    T = [np.zeros(_shape(g, t, B, H, W, predc), np.float64) for t in range(len(g.C))]
    for o in g.ops:
        i, out = o["i"], o["o"]
        if o["op"] == "input":
            T[out][:, :3] = x
        elif o["op"] == "conv":
            w, b = (torch.as_tensor(np.asarray(a, np.float64)) for a in folded[o["layer"]])
            y = F.conv2d(torch.as_tensor(T[i][:, :o["cin"]]), w, b, 2 if o["s2"] else 1, w.shape[2] // 2)
            if o["act"] is not None:
                y = F.leaky_relu(y, o["act"])
            if o["res"] >= 0:
                y = y + torch.as_tensor(T[o["res"]])
            if o["pool"]:
                y = F.max_pool2d(y, 2, 2)
            T[out][:, o["choff"]:o["choff"] + y.shape[1]] = y.numpy()
        elif o["op"] == "pool":
            T[out] = pool2(T[i])
        elif o["op"] == "reorg":
            r = reorg(T[i], o["s"])
            T[out][:, o["choff"]:o["choff"] + r.shape[1]] = r
        elif o["op"] == "spp":
            C = o["C"]
            for k, p in enumerate(spp_pools(T[i][:, :C])):
                T[i][:, (k + 1) * C:(k + 2) * C] = p
        elif o["op"] == "up":
            up = F.interpolate(torch.as_tensor(T[i]), scale_factor=2.0, mode="bilinear", align_corners=True).numpy()
            T[out][:, o["choff"]:o["choff"] + up.shape[1]] = up
    return T


def calibrate_f64(arch, x, folded, predc):
    """(sa_in, sa): floor(log2(127 / max|.|)) of the input and of every float64 tensor"""
    T = forward_f64(arch, x, folded, predc)
    sa_in = O.floor_log2_scale(np.abs(np.asarray(x, np.float32)).max())[0]
    return sa_in, [O.floor_log2_scale(max(float(np.abs(t).max()), 1e-30))[0] for t in T], T


def preds_float(r):
    """the int8 prediction maps as fp32 values (finest level first)"""
    return [r["t"][p].astype(np.float32) * np.float32(2.0 ** (-r["sa"][p])) for p in r["pred"]]


def detect(arch, r, input_size, anchors, num_classes, conf_thresh, nms_thresh):
    """candidates (box [B,N,4], cls_scores [B,N,C]) and per-image detections of the int8 maps"""
    preds = preds_float(r)
    if arch == "yolo_v2":
        box, sc = FP.head_decode_v2(preds[0], input_size, anchors, num_classes, 32)
    else:
        box, sc = FP.tiny_head_decode(preds, input_size, anchors, num_classes, level_strides=(8, 16, 32))
    dets = [O.postprocess(box[i], sc[i], conf_thresh, nms_thresh, num_classes) for i in range(box.shape[0])]
    return np.asarray(box), np.asarray(sc), dets
