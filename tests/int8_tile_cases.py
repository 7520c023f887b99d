"""TEST INFRASTRUCTURE -- which kernel an int8 y355_net layer runs on, restated on the CPU, and the cases of
tests/test_int8_production_tiles.py.

The rules restated here: y355_convg_select and CONVG_SET (csrc/convg.hip), y355_convr_select with the int8 ring instantiations
I0 .. I5 and the launchers' own conditions (csrc/convr.hip), and in_kbytes, cout_pad, the pointwise rule, the route of run_op and
the 32-bit / 64-bit decision of y355_rq_net and y355_rq_res (csrc/y355_requant.h, applied by refresh_layer_i8 of csrc/net.hip).
The C selectors have no Python binding, so this is a restatement and not a query: if the C rules change, it has to be changed with them, or the GPU cases stop reaching the tiles
they are there for without a failure in the CPU tests.  Two things keep it honest: the family y355_net_layer_route reports is
compared with predict()'s after every forward of the GPU tests, with the EPI64 / RESIDUAL / PER_CHANNEL flags, and
test_net_calibration's sizes must predict exactly the tiles the issue behind these tests found them to take.

A deployed net runs at 416 x 416 with max_batch 64 (max_batch is the selector's batch hint: it decides between tile 5 and tile 10
on 13 x 13 maps of 256-byte chunks).  CASES are the smallest inputs that select those tiles: a stride-32 map needs 13 rows and
columns, hence 416; at 416 x 448 every level has a column past its tiles (13 x 14, 26 x 28, 52 x 56); the runs themselves have
one or two images.
"""
from fractions import Fraction

import numpy as np

import net_calib_ref as R

# CONVG_SET of csrc/convg.hip: id -> (chb, bn, th, tw, pool, wm, wn, stride)
G_TILES = {0: (32, 32, 16, 52, 1, 4, 1, 1), 1: (32, 64, 13, 26, 0, 2, 2, 1), 2: (64, 64, 13, 26, 0, 4, 2, 1),
           3: (64, 64, 26, 26, 1, 8, 1, 1), 4: (128, 128, 13, 26, 0, 4, 2, 1), 5: (256, 256, 13, 13, 0, 2, 4, 1),
           6: (256, 64, 13, 13, 0, 4, 1, 1), 7: (64, 64, 8, 16, 0, 4, 1, 1), 8: (64, 64, 8, 16, 1, 4, 1, 1),
           9: (64, 64, 8, 16, 0, 4, 1, 2), 10: (128, 64, 13, 13, 0, 4, 2, 1)}
# the int8 ring instantiations of csrc/convr.hip in the order y355_convr_select walks them: name -> (cinb, bn, th, tw, pool)
RINGS = [("I0", 64, 64, 26, 26, 1), ("I1", 256, 256, 13, 13, 0), ("I2", 128, 128, 13, 26, 0), ("I3", 384, 128, 13, 26, 0),
         ("I4", 512, 256, 13, 13, 0), ("I5", 1024, 128, 13, 13, 0)]
FIRST, FRONT, RING, POINTWISE, GENERIC4, GENERIC8 = "FIRST", "FRONT", "RING", "POINTWISE", "GENERIC4", "GENERIC8"
# Y355_ROUTE_* of include/yolo355.h (route & 0xff)
FAMILY = {1: FIRST, 2: FRONT, 3: RING, 4: POINTWISE, 5: GENERIC4, 6: GENERIC8}
EPI64, RESIDUAL, PER_CHANNEL = 0x100, 0x200, 0x400


def convg_select(in_pb, cout, pool, H, W, stride=1, batch_hint=0):
    if stride == 2:
        return 9 if (in_pb % 64 == 0 and not pool) else -1
    small = H < 13 or W < 13
    if in_pb == 32:
        return 0 if pool else 1
    if pool:
        return 8 if small else 3
    if small:
        return 7
    if cout <= 64:
        return 6 if in_pb % 256 == 0 else 2
    if cout <= 128:
        return 4 if in_pb % 128 == 0 else 2
    if in_pb % 256 == 0:
        wgs = ((H + 12) // 13) * ((W + 12) // 13) * ((cout + 255) // 256) * (batch_hint if batch_hint > 0 else 1 << 20)
        return 5 if wgs >= 192 else 10
    return 4 if in_pb % 128 == 0 else 2


def convr_select(in_pb, cout_pad, pool, H, W):
    """the int8 ring of a 3x3 / stride-1 layer, by name, or None"""
    if pool and ((H | W) & 1):
        return None
    for name, cinb, bn, th, tw, rp in RINGS:
        if cinb == in_pb and rp == pool and cout_pad % bn == 0 and H >= th and W >= tw:
            return name
    return None


def in_kbytes(o):
    """bytes of input channels an int8 convolution consumes per pixel"""
    c = (o["cin"] + 31) // 32 * 32
    if o["s2"]:
        c = (c + 63) // 64 * 64
    return c


def cout_pad(cout, kid):
    bn = G_TILES[kid][1]
    return (cout + bn - 1) // bn * bn


def _pitch(g, t):
    """bytes per pixel of (non-prediction) tensor t"""
    return (g.C[t] + 31) // 32 * 32


def predict(arch, size, max_batch, predc, wide=(), fused_front=False):
    """Per conv layer (list index = layer = weight slot) a dict:
      stat      the tile whose STAT instantiation takes the layer's maximum in a calibration step, which is also the tile
                whose plain variants run the layer in the write pass (None: the first-layer kernel of slim / tiny)
      family    the Y355_ROUTE_* family of a forward
      tile      the generic tile id or the ring's name (None for FIRST, FRONT and POINTWISE)
      residual  the layer adds a residual (from the graph)
      chunks    chunks of the generic tile the layer reads (in_kbytes / chb)
    `wide`: the layers whose epilogue needs 64 bits (narrow_of), which keeps them off the ring and the pointwise kernel;
    fused_front: a plain forward of slim / tiny whose first two layers the fused front end runs."""
    g = R.graph(arch)
    H, W = size
    out = []
    for o in g.ops:
        if o["op"] != "conv":
            continue
        li = o["layer"]
        res = o["res"] >= 0
        if o["i"] < 0:                                           # OP_CONV1: the network input, slim and tiny
            out.append(dict(stat=None, family=FRONT if fused_front else FIRST, tile=None, residual=False, chunks=0))
            continue
        cout = predc if o["cout"] is None else o["cout"]
        hi, wi = H // g.div[o["i"]], W // g.div[o["i"]]
        kb = in_kbytes(o)
        kid = convg_select(kb, cout, o["pool"], hi, wi, 2 if o["s2"] else 1, max_batch)
        assert kid >= 0 and kb % G_TILES[kid][0] == 0, (arch, li)
        cp = cout_pad(cout, kid)
        e = dict(stat=kid, residual=res, chunks=kb // G_TILES[kid][0])
        narrow = li not in wide
        ring = convr_select(kb, cp, o["pool"], hi, wi) if (o["k"] == 3 and not o["s2"] and not res) else None
        if fused_front and li == 1:
            e.update(family=FRONT, tile=None)
        elif (o["k"] == 1 and not o["s2"] and not res and not o["pool"] and _pitch(g, o["i"]) == kb and cp % 64 == 0 and
              kb % 64 == 0 and kb <= 1024 and narrow):
            e.update(family=POINTWISE, tile=None)
        elif ring is not None and _pitch(g, o["i"]) == kb and narrow:      # (the launcher wants the whole pixel)
            e.update(family=RING, tile=ring)
        else:
            wm, wn = G_TILES[kid][5:7]
            e.update(family=GENERIC8 if wm * wn == 8 else GENERIC4, tile=kid)
        out.append(e)
    return out


def stat_set(pred):
    return {(e["stat"], e["residual"]) for e in pred if e["stat"] is not None}


def forward_set(pred):
    return {(e["family"], e["tile"], e["residual"]) for e in pred}


# ------------------------------------------------------------------------------------------ the 32-bit / 64-bit decision
def narrow_rule(sa_i, e_wc, e_b, qb_max, wabs, lk, nm, sa_o, s_r=None):
    """One layer's 32-bit / 64-bit decision from plain numbers, in exact rationals: the input's exponent, every output channel's
    weight exponent and sum |q_w|, the bias exponent and max |q_b|, the slope nm / 2^lk, the output's exponent and, for a
    residual layer, the residual's.  True = y355_rq_net's narrow (fits32 on the layer's own weights, else the split form of the
    negative branch); a residual layer by y355_rq_res's 32-bit form alone (csrc/y355_requant.h)."""
    two = Fraction(2)
    F = max(sa_i + max(int(e) for e in e_wc), int(e_b))
    E = F + lk
    bmax = int(qb_max) * two ** (F - int(e_b))
    tb = max(127 * int(w) * two ** (F - sa_i - int(e)) for w, e in zip(wabs, e_wc)) + bmax
    lim = two ** 31
    if s_r is not None:
        shp = E - sa_o
        dp, dn = max(shp - lk, s_r - sa_o, 0), max(shp, s_r - sa_o, 0)
        p_t, p_r, n_t, n_r = lk - shp + dp, sa_o - s_r + dp, dn - shp, sa_o - s_r + dn
        return bool(max(dp, dn, p_t, p_r, n_t, n_r) <= 30 and tb < lim and bmax < lim and
                    tb * two ** p_t + 127 * two ** p_r + two ** dp < lim and
                    tb * nm * two ** n_t + 127 * two ** n_r + two ** dn < lim)
    sh = E - sa_o
    fits = tb * max(two ** max(0, lk - sh), nm * two ** max(0, -sh)) + two ** max(sh, 0) < lim and bmax < lim
    if not fits and 9 <= sh <= 31 and 1 <= nm < 4096:
        pos = tb * two ** max(0, lk - sh) + two ** max(sh - lk, 0)
        neg = (tb / 256 + 1) * nm + 256 + two ** (sh - 9)
        fits = tb < two ** 30 and pos < lim and neg < lim and bmax < lim
    return bool(fits)


def narrow_of(arch, qlayers, sa_in, sa, only=None):
    """[layer] -> True when refresh_layer_i8 (csrc/net.hip, by the rules of csrc/y355_requant.h) gives the layer the 32-bit
    epilogue under these exponents: narrow_rule on the layer's numbers (the C code's long doubles hold these integers times
    powers of two exactly).  only: one layer, returns its bool."""
    g = R.graph(arch)
    out = {}
    for o in g.ops:
        if o["op"] != "conv" or (only is not None and o["layer"] != only):
            continue
        L = qlayers[o["layer"]]
        e_wc = np.asarray(L["e_w"], np.int64).reshape(-1)
        qw = np.asarray(L["q_w"], np.int64)
        if e_wc.size == 1:
            e_wc = np.full(qw.shape[0], int(e_wc[0]), np.int64)
        lk, nm = R.W.ACT[o["act"]]
        out[o["layer"]] = narrow_rule(sa_in if o["i"] < 0 else sa[o["i"]], e_wc, L["e_b"], np.abs(np.asarray(L["q_b"], np.int64)).max(),
                                      np.abs(qw).reshape(qw.shape[0], -1).sum(axis=1), lk, nm, sa[o["o"]],
                                      sa[o["res"]] if o["res"] >= 0 else None)
    return out[only] if only is not None else [out[i] for i in range(len(out))]


def is_per_channel(L):
    """a layer loaded through the per-channel entry point runs the per-channel kernels only when its exponents differ"""
    e = np.asarray(L["e_w"]).reshape(-1)
    return bool(e.size > 1 and e.max() != e.min())


# ------------------------------------------------------------------------------------------ the cases
ANCH_NLEV = {"slim_yolo_v2": 1, "tiny_yolo_v3": 2, "yolo_v2": 1, "yolo_v3": 3, "yolo_v3_spp": 3}
GAIN = {"yolo_v3": 1.3, "yolo_v3_spp": 1.3}          # as test_net_calibration.GAIN
CONF = 0.05
# (tag, arch, [H, W], classes, max_batch, B, per-channel)
CASES = [
    ("v3_448_mb64", "yolo_v3", [416, 448], 2, 64, 2, False),
    ("v3_448_mb64_pc", "yolo_v3", [416, 448], 2, 64, 1, True),
    ("v3_416_mb2", "yolo_v3", [416, 416], 20, 2, 2, False),        # the drop-in's handle: tile 10
    ("spp_416_mb64", "yolo_v3_spp", [416, 416], 20, 64, 1, False),
    ("v2_416_mb64", "yolo_v2", [416, 416], 20, 64, 2, False),
    ("v2_448_mb2", "yolo_v2", [416, 448], 2, 2, 2, False),
    ("tiny_448_mb64", "tiny_yolo_v3", [416, 448], 2, 64, 2, False),
    ("tiny_448_mb64_pc", "tiny_yolo_v3", [416, 448], 2, 64, 1, True),
    ("slim_448_mb64", "slim_yolo_v2", [416, 448], 2, 64, 2, False),
    # with 20 classes SlimYOLOv2's 3x3 prediction layer has 125 output channels and takes tile 4 in the forward (with 2 it takes
    # tile 6): the one triple of required("forward") the rows above do not reach
    ("slim_448_mb64_c20", "slim_yolo_v2", [416, 448], 20, 64, 1, False),
]
TAGS = [c[0] for c in CASES]
DEPLOYED = ([416, 416], 64)                              # size and max_batch of a deployed net


def anchors_of(arch):
    from yolo355 import synth
    return {"slim_yolo_v2": synth.ANCHOR_SIZE_MASK, "tiny_yolo_v3": synth.TINY_MULTI_ANCHOR_SIZE, "yolo_v2": synth.ANCHOR_SIZE,
            "yolo_v3": synth.MULTI_ANCHOR_SIZE, "yolo_v3_spp": synth.MULTI_ANCHOR_SIZE}[arch]


def predc_of(arch, classes):
    return len(anchors_of(arch)) // ANCH_NLEV[arch] * (5 + classes)


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def predict_case(tag, wide=(), fused_front=False):
    _, arch, size, classes, mb, _, _ = case(tag)
    return predict(arch, size, mb, predc_of(arch, classes), wide, fused_front)


def required(which):
    """what the five graphs select at 416 x 416 with max_batch 64, classes 2 and 20: "stat" -> {(tile, residual)},
    "forward" -> {(family, tile or ring, residual)} (every epilogue narrow, tap forward)"""
    fn = {"stat": stat_set, "forward": forward_set}[which]
    out = set()
    for arch in R.ARCHS:
        for classes in (2, 20):
            out |= fn(predict(arch, DEPLOYED[0], DEPLOYED[1], predc_of(arch, classes)))
    return out


def qlayers_of(tag, seed):
    """the case's int8 layers: net_calib_ref.make_folded through prep.quantize_folded; the per-channel rows on channels spread
    over 6 more bits (int8_pc_ref.spread_channels(folded, 7), exponents capped at a spread of 8)"""
    import int8_pc_ref as P
    from yolo355 import prep
    _, arch, size, classes, mb, B, pc = case(tag)
    folded = R.make_folded(arch, seed, predc_of(arch, classes), GAIN.get(arch, 2.0))
    if not pc:
        return prep.quantize_folded(folded, False, None)
    ql = prep.quantize_folded(P.spread_channels(folded, 7), True, 8)
    assert P.max_spread_of(ql) >= 6, "the fixture no longer spreads the channels: the shifts would not matter"
    return ql


def images_of(seed, B, size):
    from yolo355 import synth
    return np.concatenate([synth.make_images(seed + i, 1, size[0], size[1]) for i in range(B)])
