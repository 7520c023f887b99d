"""TEST INFRASTRUCTURE -- CPU restatement of one calibration step on the int8 y355_net graphs (DESIGN.md section 6,
include/yolo355.h y355_net_calibrate), independent of the HIP code: the graphs of tests/int8_wide_ref.py (DarkNet) and of
oracle/net_int8_oracle.py (YOLOv3tiny; SlimYOLOv2 is the same conv rule on a chain), on unclamped int64, with the tracker
state machine of AveragedRangeTracker (models/slim_yolo_v2.py:9-38) and the multi-producer rule.

One step = one pass over the ops in graph order:
  tracker 0 sees max |x|; tracker 1 + t sees the maximum of everything written into tensor t before requantisation --
  conv max |t'| / 2^(F + lk) over the un-pooled outputs (per-channel shifts included), with a residual max |u| / 2^G,
  bilinear the maximum of the blended fp32 values times 2^-s_in, reorg the maximum of the source bytes times 2^-s_in, SPP
  nothing; pool outputs and the DarkNet input tensor mirror their source's entry.  The update happens inline at the
  tensor's FIRST producer (that exponent holds for the rest of the step); a buffer with later producers is written by
  them with it, and at the end its update is redone from the pre-step state with the maximum over all producers.
"""
import numpy as np
import torch

import int8_wide_ref as W
from oracle import net_int8_oracle as N
from oracle import yolo_oracle as O

ARCHS = ("slim_yolo_v2", "tiny_yolo_v3", "yolo_v2", "yolo_v3", "yolo_v3_spp")


def slim_graph():
    """kSlimOps / kSlimT of csrc/net_arch.h (models/slim_yolo_v2.py:551-567)"""
    g = W.Graph()
    for C, d in [(16, 2), (32, 4), (64, 4), (64, 8), (128, 8), (128, 16), (256, 16), (256, 16), (256, 16), (None, 16)]:
        g.T(C, d)
    chain = [(3, 16, 1), (16, 32, 1), (32, 64, 0), (64, 64, 1), (64, 128, 0), (128, 128, 1), (128, 256, 0), (256, 256, 0), (256, 256, 0)]
    for i, (ci, co, pool) in enumerate(chain):
        g.conv(i - 1, i, 0, ci, co, 3, W.L125, pool=pool)
    g.conv(8, 9, 0, 256, None, 3, W.NONE)
    g.pred, g.strides = [9], [16]
    return g


def tiny_graph():
    """kTinyOps / kTinyT of csrc/net_arch.h = oracle.net_int8_oracle.TINY_OPS"""
    g = W.Graph()
    for C, d in zip(N.TINY_CH, [2, 4, 8, 16, 16, 32, 32, 32, 32, 32, 32, 16, 32, 16, 32]):
        g.T(C, d)
    cin = {0: 3, 1: 16, 2: 32, 3: 64, 4: 128, 5: 256, 6: 512, 7: 1024, 8: 256, 9: 384, 10: 256, 11: 512, 12: 256}
    for op, i, o, choff, li, k, pool, slope in N.TINY_OPS:
        if op == "conv":
            cout = {4: 256}.get(li, N.TINY_CH[o])
            g.conv(i, o, choff, cin[li], cout, k, slope, pool=pool)
            assert g.ops[-1]["layer"] == li
        elif op == "pool":
            g.add("pool", i, o, C=N.TINY_POOL_IN_C[o], pad1=(pool == 1))
        else:
            g.add("up", i, o, choff=choff)
    g.pred, g.strides = [13, 14], [16, 32]
    return g


def graph(arch):
    return {"slim_yolo_v2": slim_graph, "tiny_yolo_v3": tiny_graph}.get(arch, W.GRAPHS.get(arch))()


class Tracker:
    """AveragedRangeTracker.quantize_activation's state (models/slim_yolo_v2.py:16-33) in torch's fp32 arithmetic"""

    def __init__(self, scale=0.0, first_a=0):
        self.scale = torch.tensor([scale], dtype=torch.float32)
        self.first_a = int(first_a)

    def copy(self):
        return Tracker(float(self.scale.item()), self.first_a)

    def update(self, max_abs, freeze, momentum=0.1):
        m = torch.as_tensor(np.float32(max_abs), dtype=torch.float32).reshape(())
        s = (2 ** (8 - 1) - 1) / m
        if self.first_a == 0:
            self.first_a = 1
            self.scale = self.scale + s
        elif not freeze:
            self.scale = self.scale * (1 - momentum) + s * momentum
        return self.exponent()

    def exponent(self):
        return int(torch.floor(torch.log2(self.scale)).item())

    @property
    def bits(self):
        return int(self.scale.numpy().view(np.uint32)[0])


def f32_of(int_max, frac_bits):
    """an integer maximum of exponent frac_bits as the float32 y355_calibrate forms: (float)M * 2^-frac_bits"""
    return np.array(int(int_max), np.uint64).astype(np.float32) * np.float32(2.0 ** -frac_bits)


def pre_requant(acc, L, s_in, act):
    """t' (int64) and its exponent E = F + lk; e_w one exponent or one per output channel"""
    e_w = np.asarray(L["e_w"], np.int64).reshape(-1)
    Fb = max(s_in + int(e_w.max()), int(L["e_b"]))
    shl = (Fb - s_in - e_w) * np.ones(acc.shape[1], np.int64)
    t = acc * (np.int64(1) << shl)[None, :, None, None] + \
        (np.asarray(L["q_b"], np.int64) * (np.int64(1) << np.int64(Fb - int(L["e_b"]))))[None, :, None, None]
    lk, m = W.ACT[act]
    return np.where(t >= 0, t * (np.int64(1) << np.int64(lk)), t * np.int64(m)), Fb + lk


def blend(q_in):
    """the fp32 two-tap blend of the bilinear x2 (align_corners), operation for operation as N.upsample_int, before the
    rescale and the rounding"""
    B, C, H, Wd = q_in.shape
    Ho, Wo = 2 * H, 2 * Wd
    f = np.float32
    ry, rx = f(H - 1) / f(Ho - 1), f(Wd - 1) / f(Wo - 1)
    sy, sx = ry * np.arange(Ho, dtype=np.float32), rx * np.arange(Wo, dtype=np.float32)
    y0, x0 = sy.astype(np.int32), sx.astype(np.int32)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, Wd - 1)
    ly, lx = sy - y0.astype(np.float32), sx - x0.astype(np.float32)
    hy, hx = f(1) - ly, f(1) - lx
    v = q_in.astype(np.float32)
    HX, LX, HY, LY = hx[None, None, None, :], lx[None, None, None, :], hy[None, None, :, None], ly[None, None, :, None]
    top = HX * v[:, :, y0][:, :, :, x0] + LX * v[:, :, y0][:, :, :, x1]
    bot = HX * v[:, :, y1][:, :, :, x0] + LX * v[:, :, y1][:, :, :, x1]
    out = HY * top + LY * bot
    assert out.dtype == np.float32
    return out


def _pool(x, pad1):
    if not pad1:
        return W.pool2(x)
    p = np.pad(x, ((0, 0), (0, 0), (0, 1), (0, 1)))             # ZeroPad2d((0,1,0,1)) + MaxPool2d(2, 1)
    return np.maximum(np.maximum(p[:, :, :-1, :-1], p[:, :, :-1, 1:]), np.maximum(p[:, :, 1:, :-1], p[:, :, 1:, 1:]))


def step(arch, x, qlayers, trackers, freeze, momentum=0.1, predc=None):
    """One calibration step; `trackers` ([1 + num_tensors] Tracker) is updated in place.
    Returns dict(sa_in, sa, max (float32 [1 + num_tensors]), t (the int64 tensors the pass wrote), first_sa (the
    exponents the pass ran on: those of the first producers))."""
    g = graph(arch)
    x = np.asarray(x, np.float32)
    B, _, H, Wd = x.shape
    nt = len(g.C)
    assert len(trackers) == nt + 1
    pre = [t.copy() for t in trackers]
    mx = np.zeros(nt + 1, np.float32)
    sa = [None] * nt
    mx[0] = np.abs(x).max()
    sa_in = trackers[0].update(mx[0], freeze, momentum)
    q_x, _ = W.quantize_input(x, sa_in)
    T = [np.zeros(W._shape(g, t, B, H, Wd, predc), np.int64) for t in range(nt)]
    first, late = {}, set()

    def produced(t, m):
        if t not in first:
            first[t] = True
            mx[t + 1] = m
            sa[t] = trackers[t + 1].update(m, freeze, momentum)
        else:
            late.add(t)
            mx[t + 1] = max(mx[t + 1], np.float32(m))

    for o in g.ops:
        i, out = o["i"], o["o"]
        if o["op"] == "input":
            T[out][:, :3] = q_x
            trackers[out + 1], mx[out + 1], sa[out] = trackers[0].copy(), mx[0], sa_in
            first[out] = True
        elif o["op"] == "conv":
            L = qlayers[o["layer"]]
            src, s_i = (q_x, sa_in) if i < 0 else (T[i][:, :o["cin"]], sa[i])
            u, fb = pre_requant(W.conv_int(src, np.asarray(L["q_w"]), 2 if o["s2"] else 1), L, s_i, o["act"])
            if o["res"] >= 0:
                s_r = sa[o["res"]]
                G = max(fb, s_r)
                u = u * (np.int64(1) << np.int64(G - fb)) + T[o["res"]] * (np.int64(1) << np.int64(G - s_r))
                fb = G
            produced(out, f32_of(np.abs(u).max(), fb))
            q = O.rne_shift(u, fb - sa[out])
            if o["pool"]:
                q = W.pool2(q)
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = np.clip(q, -127, 127)
        elif o["op"] == "pool":
            T[out] = _pool(T[i][:, :o.get("C", T[i].shape[1])], o.get("pad1", False))
            trackers[out + 1], mx[out + 1], sa[out] = trackers[i + 1].copy(), mx[i + 1], sa[i]
            first[out] = True
        elif o["op"] == "reorg":
            produced(out, np.float32(np.abs(T[i]).max()) * np.float32(2.0 ** -sa[i]))
            q, _ = W.rescale(W.reorg(T[i], o["s"]), sa[out] - sa[i])
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
        elif o["op"] == "spp":
            C = o["C"]
            for k, p in enumerate(W.spp_pools(T[i][:, :C])):
                T[i][:, (k + 1) * C:(k + 2) * C] = p
        elif o["op"] == "up":
            v = blend(T[i])
            produced(out, np.abs(v).max() * np.float32(2.0 ** -sa[i]))
            q = np.clip(np.rint(v * np.float32(2.0 ** (sa[out] - sa[i]))), -127, 127).astype(np.int64)
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
    first_sa = list(sa)
    for t in sorted(late):                                      # redone from the pre-step state, maximum over all producers
        trackers[t + 1] = pre[t + 1].copy()
        sa[t] = trackers[t + 1].update(mx[t + 1], freeze, momentum)
    for o in g.ops:
        if o["op"] == "pool":
            trackers[o["o"] + 1], mx[o["o"] + 1], sa[o["o"]] = trackers[o["i"] + 1].copy(), mx[o["i"] + 1], sa[o["i"]]
    return dict(sa_in=sa_in, sa=sa, max=mx, t=T, first_sa=first_sa, late=sorted(late))


def forward_int(arch, x, qlayers, sa_in, sa, predc=None):
    """the int8 forward under given exponents with this module's rules (a step whose trackers are pinned): dict(t, sat)"""
    g = graph(arch)
    x = np.asarray(x, np.float32)
    B, _, H, Wd = x.shape
    q_x, sat = W.quantize_input(x, sa_in)
    T = [np.zeros(W._shape(g, t, B, H, Wd, predc), np.int64) for t in range(len(g.C))]
    for o in g.ops:
        i, out = o["i"], o["o"]
        if o["op"] == "input":
            T[out][:, :3] = q_x
        elif o["op"] == "conv":
            L = qlayers[o["layer"]]
            src, s_i = (q_x, sa_in) if i < 0 else (T[i][:, :o["cin"]], sa[i])
            u, fb = pre_requant(W.conv_int(src, np.asarray(L["q_w"]), 2 if o["s2"] else 1), L, s_i, o["act"])
            if o["res"] >= 0:
                G = max(fb, sa[o["res"]])
                u = u * (np.int64(1) << np.int64(G - fb)) + T[o["res"]] * (np.int64(1) << np.int64(G - sa[o["res"]]))
                fb = G
            q = O.rne_shift(u, fb - sa[out])
            if o["pool"]:
                q = W.pool2(q)
            sat += int((np.abs(q) > 127).sum())
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = np.clip(q, -127, 127)
        elif o["op"] == "pool":
            T[out] = _pool(T[i][:, :o.get("C", T[i].shape[1])], o.get("pad1", False))
        elif o["op"] == "reorg":
            q, s = W.rescale(W.reorg(T[i], o["s"]), sa[out] - sa[i])
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
            sat += s
        elif o["op"] == "spp":
            C = o["C"]
            for k, p in enumerate(W.spp_pools(T[i][:, :C])):
                T[i][:, (k + 1) * C:(k + 2) * C] = p
        elif o["op"] == "up":
            q = N.upsample_int(T[i], 2.0 ** (sa[out] - sa[i]))
            T[out][:, o["choff"]:o["choff"] + q.shape[1]] = q
    return dict(t=T, sat=sat, sa=list(sa), pred=g.pred)


def make_folded(arch, seed, predc, gain=2.0, pred_gain=1.5):
    """synthetic BN-folded fp32 (w, b) per weight slot of the graph (synth.uniform_pm1 streams, He-like bounds)"""
    from yolo355 import synth
    out = []
    for o in graph(arch).ops:
        if o["op"] != "conv":
            continue
        cout = predc if o["cout"] is None else o["cout"]
        li, k = o["layer"], o["k"]
        bound = 1.0 / np.sqrt(o["cin"] * k * k)
        g_ = pred_gain if o["act"] is None else gain
        w = synth.uniform_pm1(seed * 1000 + 2 * li, (cout, o["cin"], k, k)) * np.float32(bound * g_)
        b = synth.uniform_pm1(seed * 1000 + 2 * li + 1, (cout,)) * np.float32(0.2)
        out.append((w.astype(np.float32), b.astype(np.float32)))
    return out
