"""Cases of the operator-level API whose outputs are pinned bit for bit to a recorded run (tests/golden/ops_parent.json,
written by tests/golden/gen_golden_ops_parent.py; compared by tests/test_ops_parent_bits.py).

Each case is (id, function); the function runs on the GPU and returns {name: numpy array | int | None}.  A name that starts
with "none_" is a forward_i8 that has to decline (return None); every other value has to be there.  The shapes are the
smallest at which each shared piece of the operator layer can go wrong: maps that are no multiple of a tile, sizes that
select another tile (a repack), a workspace that grows and one that is re-zeroed for a smaller map, a requantisation cache
that misses three times in a row."""
import hashlib

import numpy as np

from yolo355.synth import uniform_pm1, uniform_u8


def _i8(seed, shape):
    return np.maximum(uniform_u8(seed, shape).view(np.int8), -127)


def _w(seed, cout, cin, kh, kw):
    return (uniform_pm1(seed, (cout, cin, kh, kw)) * np.float32(1.0 / np.sqrt(cin * kh * kw))).astype(np.float32)


def _bias_i32(seed, cout):
    return (uniform_u8(seed, (cout,)).astype(np.int32) - 128) * 37


def summarise(result):
    """what the golden file keeps of a case's result: arrays as digest + shape + dtype, scalars and None as they are"""
    out = {}
    for k, v in result.items():
        if isinstance(v, np.ndarray):
            a = np.ascontiguousarray(v)
            out[k] = {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "dtype": str(a.dtype)}
        else:
            out[k] = None if v is None else int(v)
    return out


# ---- element-wise ----------------------------------------------------------------------------------------------------------
def _x_elem():
    return uniform_pm1(1, (2, 3, 6, 10))


def _elementwise():
    import torch
    from yolo355 import engine as E
    x = _x_elem()
    xd = torch.from_numpy(x).cuda()
    r = {"reorg": E.reorg_f32(x, 2), "spp": E.spp_f32(x), "maxpool": E.maxpool2x2_f32(x), "upsample": E.upsample2x_f32(x),
         "reorg_dev": E.reorg_f32_dev(xd, 2).cpu().numpy(), "spp_dev": E.spp_f32_dev(xd).cpu().numpy(),
         "maxpool_dev": E.maxpool2x2_f32_dev(xd).cpu().numpy(), "upsample_dev": E.upsample2x_f32_dev(xd).cpu().numpy()}
    r["maxpool_i8"] = E.maxpool2x2_i8(_i8(2, (2, 3, 6, 10)))
    r["quantize"], r["quantize_clamped"] = E.quantize_input_f32_i8(np.float32(3.0) * x, 6)
    return r


# ---- bf16 convolutions -----------------------------------------------------------------------------------------------------
# (tag, cin, cout, k, stride, residual, out_fp32, slope, shapes in the order one operator object sees them)
BF16_GROUPS = [
    ("thin", 3, 24, 3, 1, False, False, 0.1, [(2, 3, 14, 27), (1, 3, 9, 11)]),
    ("repack", 24, 40, 3, 1, False, False, 0.1, [(2, 24, 14, 27), (1, 24, 9, 11), (3, 24, 14, 27)]),
    ("s2res", 24, 40, 3, 2, True, False, 0.1, [(2, 24, 9, 11), (1, 24, 14, 27)]),
    ("pred1x1", 40, 24, 1, 1, False, True, 1.0, [(2, 40, 14, 27)]),
]
# (tag, geom arguments (kernel, stride, dilation, padding), cin, cout, residual, out_fp32, shapes)
GEOM_GROUPS = [
    ("5x5p2", (5, 1, 1, 2), 13, 35, True, False, [(1, 13, 13, 17), (2, 13, 9, 11)]),
    ("7x7s2p3", (7, 2, 1, 3), 3, 8, False, True, [(3, 3, 13, 17)]),
]


def _bf16_group(seed, cout, shapes, residual, out_fp32, out_hw, host, make_op):
    """every shape through the host-pointer form, and all of them in order through ONE operator object"""
    import torch
    r = {}
    op = make_op()
    try:
        for i, shp in enumerate(shapes):
            x = uniform_pm1(seed + 10 * i, shp)
            res = uniform_pm1(seed + 10 * i + 1, (shp[0], cout) + tuple(out_hw(shp[2], shp[3]))) if residual else None
            r["host%d" % i] = host(x, res)
            rd = None if res is None else torch.from_numpy(res).cuda()
            r["op%d" % i] = op.forward(torch.from_numpy(x).cuda(), residual=rd, out_fp32=out_fp32).cpu().numpy()
    finally:
        op.close()
    return r


def _bf16_case(group):
    tag, cin, cout, k, stride, residual, out_fp32, slope, shapes = group

    def run():
        from yolo355 import engine as E
        seed = 100 + 1000 * [g[0] for g in BF16_GROUPS].index(tag)
        w, b = _w(seed + 5, cout, cin, k, k), uniform_pm1(seed + 6, (cout,))
        return _bf16_group(seed, cout, shapes, residual, out_fp32,
                           lambda h, ww: ((h + 1) // 2, (ww + 1) // 2) if stride == 2 else (h, ww),
                           lambda x, res: E.conv2d_bf16(x, w, b, residual=res, stride=stride, neg_slope=slope, out_fp32=out_fp32),
                           lambda: E.ConvOp.bf16(w, b, stride=stride, neg_slope=slope))
    return "bf16_" + tag, run


def _geom_case(group):
    tag, ga, cin, cout, residual, out_fp32, shapes = group

    def run():
        from yolo355 import engine as E
        seed = 5100 + 1000 * [g[0] for g in GEOM_GROUPS].index(tag)
        g = E.conv_geom(*ga)
        w, b = _w(seed + 5, cout, cin, ga[0], ga[0]), uniform_pm1(seed + 6, (cout,))
        return _bf16_group(seed, cout, shapes, residual, out_fp32, lambda h, ww: E.geom_out_size(g, h, ww),
                           lambda x, res: E.conv2d_geom_bf16(x, w, g, b, residual=res, neg_slope=0.1, out_fp32=out_fp32),
                           lambda: E.ConvOp.bf16(w, b, neg_slope=0.1, geom=g))
    return "bf16_geom_" + tag, run


# ---- int8, host-pointer forms ----------------------------------------------------------------------------------------------
SA, E_W, E_B = 4, 9, 6
ACTS = [("leaky", True, False), ("relu", False, True), ("none", False, False)]


def _i8_raw():
    from yolo355 import engine as E
    r = {}
    for cin, cout in ((3, 8), (40, 35)):
        q, w, b = _i8(7000 + cin, (2, cin, 7, 9)), _i8(7100 + cin, (cout, cin, 3, 3)), _bias_i32(7200 + cin, cout)
        for name, leaky, relu in ACTS:
            r["c%d_%s" % (cin, name)], r["c%d_%s_frac_bits" % (cin, name)] = E.conv3x3_i8_raw(q, w, b, SA, E_W, E_B, leaky=leaky, relu=relu)
    return r


def _i8_geom_raw():
    from yolo355 import engine as E
    r = {}
    for tag, ga, cin, cout, shp in (("7x7s2p3", (7, 2, 1, 3), 3, 8, (3, 3, 13, 17)), ("3x3d2p2", (3, 1, 2, 2), 64, 130, (1, 64, 9, 11))):
        q, w, b = _i8(7300 + cin, shp), _i8(7400 + cin, (cout, cin, ga[0], ga[0])), _bias_i32(7500 + cin, cout)
        r[tag], r[tag + "_frac_bits"] = E.conv_geom_i8_raw(q, w, b, SA, E_W, E_B, E.conv_geom(*ga))
    return r


def _i8_fused():
    """sa_out such that a share of the outputs saturates: the real values have a standard deviation of about
    sqrt(9 cin) * 74^2 / 2^13 (3.4 for cin 3, 12.5 for cin 40), so 2^4 resp. 2^3 puts the +-127 clamp near two sigma"""
    from yolo355 import engine as E
    r = {}
    for cin, cout, shp, sa_out, kw in ((3, 8, (2, 3, 8, 10), 4, dict(leaky=True, pool=True)), (40, 35, (2, 40, 7, 9), 3, dict(leaky=False, relu=True))):
        q, w, b = _i8(7600 + cin, shp), _i8(7700 + cin, (cout, cin, 3, 3)), _bias_i32(7800 + cin, cout)
        out, st = E.conv3x3_i8_fused(q, w, b, SA, E_W, E_B, sa_out, **kw)
        r["c%d" % cin] = out
        for k in ("absmax_t", "frac_bits", "saturated", "guard"):
            r["c%d_%s" % (cin, k)] = st[k]
    return r


# ---- int8 operator objects -------------------------------------------------------------------------------------------------
I8_OP_STEPS = [(4, (2, 32, 16, 24)), (6, (1, 32, 7, 9)), (4, (3, 32, 16, 24))]      # (exponent of the dyadic input, shape)


def _i8_op_case(tag, ga):
    def run():
        import torch
        from yolo355 import engine as E
        w, b = _i8(8100, (48, 32, 3, 3)), _bias_i32(8200, 48)
        op = E.ConvOp.int8(w, b, E_W, E_B, leaky=True, geom=None if ga is None else E.conv_geom(*ga))
        r = {}
        try:
            for i, (e, shp) in enumerate(I8_OP_STEPS):
                q = _i8(8300 + i, shp)
                q.flat[0] = 127                                   # max |q| = 127: the operator has to find exactly the exponent e
                y = op.forward_i8(torch.from_numpy(q.astype(np.float32) / np.float32(2 ** e)).cuda())
                r["step%d" % i] = None if y is None else y.cpu().numpy()
            shp = I8_OP_STEPS[1][1]
            r["none_nondyadic"] = op.forward_i8(torch.from_numpy(uniform_pm1(8400, shp)).cuda())
            r["none_zero"] = op.forward_i8(torch.zeros(shp, device="cuda"))
        finally:
            op.close()
        return r
    return "i8_op_" + tag, run


CASES = ([("elementwise", _elementwise)] + [_bf16_case(g) for g in BF16_GROUPS] + [_geom_case(g) for g in GEOM_GROUPS] +
         [("i8_raw", _i8_raw), ("i8_geom_raw", _i8_geom_raw), ("i8_fused", _i8_fused),
          _i8_op_case("3x3", None), _i8_op_case("3x3d2p2", (3, 1, 2, 2))])
