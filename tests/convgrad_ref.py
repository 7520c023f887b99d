"""The arithmetic contract of libyolo355_convgrad.so restated in torch on any floating type, and the
cases tests/test_convgrad_ref.py and tests/test_convgrad.py share.  The operands come in already rounded (rb); the rounding of
G is a switch; the backward is written out by hand on the im2col matrix (unfold / fold), not through autograd.  The same
functions on the operands' absolute values give S, the sum of absolute products of an element, for the interval of the
element-wise checks."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

Geo = collections.namedtuple("Geo", "kh kw stride_h stride_w dil_h dil_w pad_top pad_bottom pad_left pad_right")
Case = collections.namedtuple("Case", "geo cin cout B H W")


def geo(k, stride=1, padding=0, dilation=1):
    """Geo of nn.Conv2d's arguments; padding: int, pair, four pads (top, bottom, left, right), 'same' or 'valid'"""
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
    (kh, kw), (sh, sw), (dh, dw) = pair(k), pair(stride), pair(dilation)
    if padding == "valid":
        pads = (0, 0, 0, 0)
    elif padding == "same":
        th, tw = dh * (kh - 1), dw * (kw - 1)
        pads = (th // 2, th - th // 2, tw // 2, tw - tw // 2)
    elif isinstance(padding, int) or len(padding) == 2:
        ph, pw = pair(padding)
        pads = (ph, ph, pw, pw)
    else:
        pads = tuple(padding)
    return Geo(kh, kw, sh, sw, dh, dw, *pads)


# the issue's table; h: 81 pixels at 9 waves per run give 3 runs of 32, 32 and 17 pixels (asserted from the plan query)
CASES = collections.OrderedDict([
    ("a", Case(geo(3, 1, 1), 3, 16, 2, 9, 11)),
    ("b", Case(geo(1), 40, 35, 3, 7, 5)),
    ("c", Case(geo(3, 2, 1), 16, 32, 2, 13, 10)),
    ("d", Case(geo((5, 3), (1, 2), (2, 1, 0, 3), (2, 1)), 8, 24, 2, 12, 9)),
    ("e", Case(geo(4, 1, "same"), 16, 16, 1, 6, 6)),
    ("f", Case(geo(3, 1, 1), 384, 256, 1, 4, 4)),
    ("g", Case(geo((6, 5), 1, "valid"), 8, 8, 2, 6, 5)),
    ("h", Case(geo(3, 1, 1), 16, 16, 1, 9, 9)),
])
# beside the table, for the exact zeros of dx: input pixels that no window reads (between the windows of a 1x1 at stride 2; the
# trailing row and column of a 3x3 at stride 2 without padding on an 8 x 8 map)
CASES["s2k1"] = Case(geo(1, 2, 0), 8, 8, 1, 5, 6)
CASES["s2p0"] = Case(geo(3, 2, 0), 8, 8, 1, 8, 8)
TABLE = tuple("abcdefgh")
# the weight gradient's pixel loop more than one iteration deep: chunks of 64 and 96 pixels (two and three iterations of 32 per
# run), a last run that is shorter and no multiple of 8, runs that cross an image boundary; r2 and r3 with the 255 output channels
# of a YOLOv3 pred layer; p64 at the pad limit, 178 runs.  (chunk, runs, last) are asserted from the plan query.
CASES["r1"] = Case(geo(3, 1, 1), 256, 64, 2, 15, 17)
CASES["r2"] = Case(geo(3, 1, 1), 128, 255, 3, 13, 13)
CASES["r3"] = Case(geo(1), 1024, 255, 2, 13, 13)
CASES["r4"] = Case(geo(3, 2, 1), 128, 128, 2, 33, 29)
CASES["p64"] = Case(geo(3, 1, 64), 4, 6, 1, 5, 4)
RUNS = ("r1", "r2", "r3", "r4", "p64")
RUN_SLOPES = (0.1, 1.0)
# the limits of the geometry (kernel 32, stride 16, dilation 32, pad 64) and what lies between: 1024 taps on one real channel in
# eight; a kernel wider than the map; strides above the kernel, different and both above 1; every parameter different on the
# two axes with 24 and 40 padded channels, so that a k-step of 32 starts inside one tap and ends in the next
CASES["k32"] = Case(geo(32), 1, 1, 1, 33, 34)
CASES["k1x32"] = Case(geo((1, 32), 1, (0, 0, 16, 15)), 3, 5, 2, 4, 20)
CASES["s16"] = Case(geo(3, 16, 1), 8, 8, 1, 40, 37)
CASES["s53"] = Case(geo((2, 3), (5, 3), (1, 0, 0, 2)), 8, 16, 2, 14, 13)
CASES["mix"] = Case(geo((3, 4), (3, 2), (4, 0, 1, 5), (2, 3)), 20, 36, 2, 17, 19)
CASES["d32"] = Case(geo(2, 1, "same", 32), 8, 8, 1, 20, 18)
EDGES = ("k32", "k1x32", "s16", "s53", "mix", "d32", "p64")
SLOPES = (0.125, 0.1, 0.0, 1.0)
U = 2.0 ** -24


def out_size(g, H, W):
    return ((H + g.pad_top + g.pad_bottom - g.dil_h * (g.kh - 1) - 1) // g.stride_h + 1,
            (W + g.pad_left + g.pad_right - g.dil_w * (g.kw - 1) - 1) // g.stride_w + 1)


def rb(t):
    """round to nearest even to bf16, as float32"""
    return torch.as_tensor(t, dtype=torch.float32).to(torch.bfloat16).to(torch.float32)


def inputs(name, seed=0):
    """(x, w, bias, dy) of a case as float32 tensors from the seeded generator"""
    return make_inputs(CASES[name], 1000 * (list(CASES).index(name) + 1) + 10 * seed)


def make_inputs(c, s):
    """(x, w, bias, dy) of any Case from the generator's seeds s + 1 .. s + 4: |x|, |dy| < 1, |w| < 1 / sqrt(cin kh kw)"""
    from yolo355 import synth
    ho, wo = out_size(c.geo, c.H, c.W)
    x = torch.from_numpy(synth.uniform_pm1(s + 1, (c.B, c.cin, c.H, c.W)))
    w = torch.from_numpy(synth.uniform_pm1(s + 2, (c.cout, c.cin, c.geo.kh, c.geo.kw))) * float(1.0 / np.sqrt(c.cin * c.geo.kh * c.geo.kw))
    b = torch.from_numpy(synth.uniform_pm1(s + 3, (c.cout,))) * 0.25
    dy = torch.from_numpy(synth.uniform_pm1(s + 4, (c.B, c.cout, ho, wo)))
    return x, w, b, dy


def _pad(x, g):
    return F.pad(x, (g.pad_left, g.pad_right, g.pad_top, g.pad_bottom))


def _cols(x, g):
    """the im2col matrix [B, cin * kh * kw, Ho * Wo] of the padded x"""
    return F.unfold(_pad(x, g), (g.kh, g.kw), dilation=(g.dil_h, g.dil_w), padding=0, stride=(g.stride_h, g.stride_w))


def forward(x, w, bias, g, slope):
    """(z, y): z = sum x w + bias, y = z > 0 ? z : z * slope, in the operands' type"""
    B, _, H, W = x.shape
    ho, wo = out_size(g, H, W)
    z = torch.matmul(w.reshape(w.shape[0], -1), _cols(x, g)).reshape(B, w.shape[0], ho, wo)
    if bias is not None:
        z = z + bias.view(1, -1, 1, 1)
    return z, torch.where(z > 0, z, z * slope)


def grad_out(dy, y, slope, round_g=True):
    """G = rb(dy * (y > 0 ? 1 : slope)), the product in float32 as the kernel forms it; round_g=False: unrounded, in dy's type"""
    if not round_g:
        return dy * torch.where(y > 0, torch.ones_like(dy), torch.full_like(dy, slope))
    m = torch.where(y > 0, torch.ones(y.shape, dtype=torch.float32), torch.full(y.shape, slope, dtype=torch.float32))
    return rb(dy.to(torch.float32) * m)


def backward(x, w, G, g):
    """(dx, dw, db) of the contract from G, written out: dw = G cols^T, dx = fold(W^T G) without the padding, db = sum G"""
    B, cin, H, W = x.shape
    cout = w.shape[0]
    Gm = G.reshape(B, cout, -1)
    dw = torch.einsum("bol,bkl->ok", Gm, _cols(x, g)).reshape(w.shape)
    dcols = torch.matmul(w.reshape(cout, -1).t(), Gm)
    Hp, Wp = H + g.pad_top + g.pad_bottom, W + g.pad_left + g.pad_right
    dxp = F.fold(dcols, (Hp, Wp), (g.kh, g.kw), dilation=(g.dil_h, g.dil_w), padding=0, stride=(g.stride_h, g.stride_w))
    dx = dxp[:, :, g.pad_top:g.pad_top + H, g.pad_left:g.pad_left + W]
    return dx, dw, Gm.sum((0, 2))


def torch_forward(x, w, bias, g, slope):
    """F.leaky_relu / relu / identity of F.conv2d on the explicitly padded input: what autograd differentiates"""
    z = F.conv2d(_pad(x, g), w, bias, stride=(g.stride_h, g.stride_w), padding=0, dilation=(g.dil_h, g.dil_w))
    return z if slope == 1.0 else (F.relu(z) if slope == 0.0 else F.leaky_relu(z, slope))


def bound(K, S, value):
    """the project's interval of an fp32 sum of K - 1 exact products: 2 K u S 1.001 + u |value|"""
    return 2.0 * K * U * S * 1.001 + U * value.abs()


def untouched(g, H, W):
    """bool [H, W]: the input pixels no window of the geometry reads (dx is exactly zero there)"""
    ho, wo = out_size(g, H, W)
    ys = {oy * g.stride_h + ky * g.dil_h - g.pad_top for oy in range(ho) for ky in range(g.kh)}
    xs = {ox * g.stride_w + kx * g.dil_w - g.pad_left for ox in range(wo) for kx in range(g.kw)}
    m = np.ones((H, W), bool)
    for yy in ys:
        for xx in xs:
            if 0 <= yy < H and 0 <= xx < W:
                m[yy, xx] = False
    return m


def pixel(c, q):
    """(image, oy, ox) of the flat output pixel q, the order in which the weight gradient walks them"""
    ho, wo = out_size(c.geo, c.H, c.W)
    return q // (ho * wo), q % (ho * wo) // wo, q % wo


def patch(c, xr, bi, oy, ox):
    """[cin, kh, kw] float32: xr under the window of output pixel (oy, ox) of image bi, zeros where the window leaves the map"""
    g = c.geo
    out = torch.zeros(c.cin, g.kh, g.kw)
    for ky in range(g.kh):
        for kx in range(g.kw):
            iy, ix = oy * g.stride_h + ky * g.dil_h - g.pad_top, ox * g.stride_w + kx * g.dil_w - g.pad_left
            if 0 <= iy < c.H and 0 <= ix < c.W:
                out[:, ky, kx] = xr[bi, :, iy, ix].float()
    return out


def dead_taps(g, H, W):
    """bool [kh, kw]: the taps that lie in the padding under every window (their rows of dw are exactly zero)"""
    ho, wo = out_size(g, H, W)
    rows = [any(0 <= oy * g.stride_h + ky * g.dil_h - g.pad_top < H for oy in range(ho)) for ky in range(g.kh)]
    cols = [any(0 <= ox * g.stride_w + kx * g.dil_w - g.pad_left < W for ox in range(wo)) for kx in range(g.kw)]
    return ~np.outer(np.array(rows, bool), np.array(cols, bool))
