"""General convolution geometry (y355_conv_geom, convgeom.hip): any kernel size, stride, dilation and zero padding through the C
ABI, the ctypes layer and the drop-in modules.  The oracle is torch.nn.functional.conv2d on the CPU in float64 -- the function the
reference's nn.Conv2d calls.  CPU tests: the geometry helper and the argument checks of the new entry points.  GPU tests: the
exact int8 route, the bf16 route, cross-checks against the 3x3 / 1x1 kernels, the device-resident forms and a composed model."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

# bf16 operands (rel. 2^-9 each) and a bf16 result (2^-9) on O(1) outputs: the tolerance of the bf16 operator tests
BF16_RTOL, BF16_ATOL = 2.0 ** -7, 0.03

# (id, kernel_size, stride, dilation, padding, cin, cout, batch, H, W)
GEOMS = [
    ("5x5_p2", 5, 1, 1, 2, 13, 35, 1, 13, 17),
    ("7x7_s2_p3", 7, 2, 1, 3, 3, 8, 3, 13, 17),
    ("3x3_d2_p2", 3, 1, 2, 2, 64, 130, 1, 9, 11),
    ("3x3_d3_p1", 3, 1, 3, 1, 96, 35, 3, 13, 17),
    ("1x1_s2", 1, 2, 1, 0, 160, 130, 3, 13, 17),
    ("3x3_p0", 3, 1, 1, 0, 13, 8, 3, 9, 11),
    ("2x2_s2", 2, 2, 1, 0, 64, 35, 1, 13, 17),
    ("1x3_p01", (1, 3), 1, 1, (0, 1), 96, 8, 1, 9, 11),
    ("3x1_p10", (3, 1), 1, 1, (1, 0), 3, 130, 3, 9, 11),
    ("4x4_same", 4, 1, 1, "same", 160, 35, 1, 13, 17),
    ("3x3_s21_p1", 3, (2, 1), 1, 1, 13, 130, 1, 13, 17),
    ("3x3_p4", 3, 1, 1, 4, 64, 8, 3, 9, 11),
]
IDS = [r[0] for r in GEOMS]


def _conv(row, bias=True):
    _, k, s, d, p, cin, cout = row[:7]
    return nn.Conv2d(cin, cout, k, stride=s, padding=p, dilation=d, bias=bias)


def _ref(conv, x, act=None):
    """float64 torch conv of `conv` on x (+ LeakyReLU(slope) / ReLU), rounded to fp32"""
    w = conv.weight.detach().double().cpu()
    b = None if conv.bias is None else conv.bias.detach().double().cpu()
    y = F.conv2d(x.detach().double().cpu(), w, b, stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
    if act == "relu":
        y = F.relu(y)
    elif act is not None:
        y = F.leaky_relu(y, act)
    return y.float().numpy()


def _dyadic(rng, shape, e):
    q = rng.integers(-127, 128, size=shape)
    q.flat[0] = 127                                       # the exponent the tensor's max implies is e
    return torch.from_numpy((q / 2.0 ** e).astype(np.float32))


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", GEOMS, ids=IDS)
def test_conv_geometry_matches_torch_output_shape(row):
    from yolo355.engine import geom_out_size
    from yolo355.utils.modules import conv_geometry
    conv = _conv(row)
    g = conv_geometry(conv)
    B, H, W = row[7:]
    want = F.conv2d(torch.zeros(B, row[5], H, W), conv.weight.detach(), None, stride=conv.stride, padding=conv.padding,
                    dilation=conv.dilation).shape
    assert geom_out_size(g, H, W) == tuple(want[2:])
    if row[4] == "same":                                  # 4x4 'same': the odd pixel of d * (k - 1) = 3 goes bottom / right
        assert (g.pad_top, g.pad_bottom, g.pad_left, g.pad_right) == (1, 2, 1, 2)


def test_conv_geometry_valid_and_same_with_dilation():
    from yolo355.engine import geom_out_size
    from yolo355.utils.modules import conv_geometry
    for k, d, p in ((3, 2, "same"), (5, 1, "valid"), ((2, 3), (3, 1), "same"), ((1, 4), 1, "valid")):
        conv = nn.Conv2d(4, 4, k, padding=p, dilation=d)
        want = F.conv2d(torch.zeros(1, 4, 11, 10), conv.weight.detach(), None, padding=p, dilation=d).shape
        assert geom_out_size(conv_geometry(conv), 11, 10) == tuple(want[2:]), (k, d, p)


def test_conv_geometry_names_the_limits():
    from yolo355.utils.modules import conv_geometry
    with pytest.raises(NotImplementedError, match="groups"):
        conv_geometry(nn.Conv2d(4, 4, 3, padding=1, groups=2))
    with pytest.raises(NotImplementedError, match="padding_mode"):
        conv_geometry(nn.Conv2d(4, 4, 3, padding=1, padding_mode="reflect"))
    with pytest.raises(NotImplementedError, match="kernel_size .* 1..32"):
        conv_geometry(nn.Conv2d(1, 1, (33, 1)))
    with pytest.raises(NotImplementedError, match="stride .* 1..16"):
        conv_geometry(nn.Conv2d(1, 1, 3, stride=17))
    with pytest.raises(NotImplementedError, match="dilation .* 1..32"):
        conv_geometry(nn.Conv2d(1, 1, 3, dilation=33))
    with pytest.raises(NotImplementedError, match="padding .* 0..64"):
        conv_geometry(nn.Conv2d(1, 1, 3, padding=65))


def test_still_loud_groups_and_padding_modes():
    """grouped convolution and non-zero padding modes raise from every drop-in, before any GPU work"""
    from yolo355.backbone.darknet import Conv_BN_LeakyReLU
    from yolo355.utils.modules import Conv2d, Conv2d_fuse, Conv2d_fuse_nobias
    x = torch.zeros(1, 4, 9, 9)
    for cls in (Conv2d, Conv2d_fuse, Conv2d_fuse_nobias):
        for bad in (dict(groups=2), dict(padding_mode="reflect")):
            m = cls(4, 8, 5, padding=2, leakyReLU=True).eval()
            m.convs[0] = nn.Conv2d(4, 8, 5, padding=2, bias=cls is not Conv2d_fuse_nobias, **bad)
            with torch.no_grad(), pytest.raises(NotImplementedError):
                m(x)
    m = Conv_BN_LeakyReLU(4, 8, 3, padding=1).eval()
    m.convs[0] = nn.Conv2d(4, 8, 3, padding=1, padding_mode="circular")
    with torch.no_grad(), pytest.raises(NotImplementedError, match="padding_mode"):
        m(x)


def test_geometry_entry_points_reject_bad_arguments_without_a_gpu():
    """argument checks of the general-geometry C ABI come before any HIP call"""
    from yolo355 import _ffi
    lib = _ffi.lib()
    h = C.c_void_p()
    ho, wo = C.c_int(), C.c_int()
    g = _ffi.ConvGeom(5, 5, 1, 1, 1, 1, 2, 2, 2, 2)
    assert lib.y355_conv_geom_out_size(C.byref(g), 13, 17, C.byref(ho), C.byref(wo)) == 0 and (ho.value, wo.value) == (13, 17)
    assert lib.y355_conv_geom_out_size(None, 13, 17, C.byref(ho), C.byref(wo)) == _ffi.EINVAL
    assert lib.y355_conv_geom_out_size(C.byref(g), 13, 17, None, C.byref(wo)) == _ffi.EINVAL
    for bad in ((0, 5, 1, 1, 1, 1, 0, 0, 0, 0), (33, 1, 1, 1, 1, 1, 0, 0, 0, 0), (3, 3, 17, 1, 1, 1, 0, 0, 0, 0),
                (3, 3, 1, 0, 1, 1, 0, 0, 0, 0), (3, 3, 1, 1, 33, 1, 0, 0, 0, 0), (3, 3, 1, 1, 1, 1, 65, 0, 0, 0),
                (3, 3, 1, 1, 1, 1, 0, 0, 0, -1)):
        gb = _ffi.ConvGeom(*bad)
        assert lib.y355_conv_geom_out_size(C.byref(gb), 13, 17, C.byref(ho), C.byref(wo)) == _ffi.EINVAL, bad
        assert lib.y355_conv_op_create_bf16_geom(0, C.c_void_p(8), None, 3, 8, C.byref(gb), 0.1, C.byref(h)) == _ffi.EINVAL, bad
    # the dilated kernel larger than the padded map: Ho < 1
    gs = _ffi.ConvGeom(3, 3, 1, 1, 3, 3, 1, 1, 1, 1)                 # reach 7 > 4 + 2
    assert lib.y355_conv_geom_out_size(C.byref(gs), 4, 9, C.byref(ho), C.byref(wo)) == _ffi.EINVAL
    assert b"Ho or Wo" in lib.y355_last_error()
    x = np.zeros(64, np.float32)
    q = np.zeros(64, np.int8)
    qb = np.zeros(8, np.int32)
    o = np.zeros(64, np.int64)
    fb = C.c_int32()
    out = np.zeros(64, np.float32)
    assert lib.y355_conv2d_geom_bf16(0, None, x.ctypes.data, None, None, 1, 3, 8, 13, 17, C.byref(g), 0.1, 0, out.ctypes.data) == _ffi.EINVAL
    assert lib.y355_conv2d_geom_bf16(0, x.ctypes.data, x.ctypes.data, None, None, 1, 3, 8, 13, 17, None, 0.1, 0, out.ctypes.data) == _ffi.EINVAL
    assert lib.y355_conv2d_geom_bf16(0, x.ctypes.data, x.ctypes.data, None, None, 1, 3, 8, 4, 9, C.byref(gs), 0.1, 0,
                                     out.ctypes.data) == _ffi.EINVAL
    assert lib.y355_conv2d_geom_bf16(0, x.ctypes.data, x.ctypes.data, None, x.ctypes.data, 1, 3, 8, 13, 17, C.byref(g), 0.1, 1,
                                     out.ctypes.data) == _ffi.EINVAL                 # fp32 output takes no residual
    args = (q.ctypes.data, q.ctypes.data, qb.ctypes.data, 1, 3, 8, 13, 17)
    assert lib.y355_conv_geom_i8_raw(0, None, *args[1:], C.byref(g), 4, 7, 5, _ffi.OP_LEAKY, o.ctypes.data, C.byref(fb)) == _ffi.EINVAL
    assert lib.y355_conv_geom_i8_raw(0, *args, C.byref(g), 4, 7, 5, _ffi.OP_LEAKY, None, C.byref(fb)) == _ffi.EINVAL
    assert lib.y355_conv_geom_i8_raw(0, *args, C.byref(g), 4, 7, 5, _ffi.OP_LEAKY | _ffi.OP_POOL, o.ctypes.data, C.byref(fb)) == _ffi.EINVAL
    assert lib.y355_conv_geom_i8_raw(0, *args, C.byref(g), 4, 7, 5, _ffi.OP_LEAKY | _ffi.OP_RELU, o.ctypes.data, C.byref(fb)) == _ffi.EINVAL
    assert lib.y355_conv_geom_i8_raw(0, q.ctypes.data, q.ctypes.data, qb.ctypes.data, 1, 3, 8, 4, 9, C.byref(gs), 4, 7, 5, 0,
                                     o.ctypes.data, C.byref(fb)) == _ffi.EINVAL
    # 127 * 127 * cin * kh * kw must fit the int32 accumulator: cin * 25 = 133 150 > 133 144
    big = (q.ctypes.data, q.ctypes.data, qb.ctypes.data, 1, 5326, 8, 13, 17)
    assert lib.y355_conv_geom_i8_raw(0, *big, C.byref(g), 4, 7, 5, _ffi.OP_LEAKY, o.ctypes.data, C.byref(fb)) == _ffi.ERANGE
    assert lib.y355_conv_op_create_i8_geom(0, q.ctypes.data, qb.ctypes.data, 5326, 8, C.byref(g), 7, 5, 0, C.byref(h)) == _ffi.ERANGE
    assert lib.y355_conv_op_create_i8_geom(0, q.ctypes.data, qb.ctypes.data, 5325, 8, C.byref(g), 7, 5, _ffi.OP_POOL, C.byref(h)) == _ffi.EINVAL
    assert lib.y355_conv_op_create_i8_geom(0, None, qb.ctypes.data, 3, 8, C.byref(g), 7, 5, 0, C.byref(h)) == _ffi.EINVAL
    assert lib.y355_conv_op_create_i8_geom(0, q.ctypes.data, qb.ctypes.data, 3, 8, None, 7, 5, 0, C.byref(h)) == _ffi.EINVAL
    assert lib.y355_conv_op_create_bf16_geom(0, None, None, 3, 8, C.byref(g), 0.1, C.byref(h)) == _ffi.EINVAL
    assert lib.y355_conv_op_create_bf16_geom(0, x.ctypes.data, None, 0, 8, C.byref(g), 0.1, C.byref(h)) == _ffi.EINVAL


# ---- GPU: exact int8 route -----------------------------------------------------------------------------------------------
def _fused(cls, row, leaky, seed):
    """a Conv2d_fuse / Conv2d_fuse_nobias of the row's geometry with dyadic weights / bias, and a dyadic input"""
    _, k, s, d, p, cin, cout, B, H, W = row
    m = cls(cin, cout, k, padding=p, stride=s, dilation=d, leakyReLU=leaky).eval()
    rng = np.random.default_rng(seed)
    conv = m.convs[0]
    with torch.no_grad():
        conv.weight.copy_(_dyadic(rng, tuple(conv.weight.shape), 9))
        if conv.bias is not None:
            conv.bias.copy_(_dyadic(rng, (cout,), 5))
    return m, _dyadic(rng, (B, cin, H, W), 4)


@pytest.mark.gpu
@pytest.mark.parametrize("row", GEOMS, ids=IDS)
def test_fused_int8_route_is_exact(row):
    from yolo355.utils.modules import Conv2d_fuse, Conv2d_fuse_nobias
    for i, (cls, leaky) in enumerate(((Conv2d_fuse, True), (Conv2d_fuse_nobias, False), (Conv2d_fuse, False), (Conv2d_fuse_nobias, True))):
        m, x = _fused(cls, row, leaky, 10 * i + len(row[0]))
        want = _ref(m.convs[0], x, 0.125 if leaky else "relu")
        with torch.no_grad():
            ycpu = m(x)
            ydev = m(x.cuda())
        assert not ycpu.is_cuda and ydev.is_cuda
        assert ycpu.shape == want.shape
        assert np.array_equal(ycpu.numpy(), want), (row[0], cls.__name__, leaky, float(np.abs(ycpu.numpy() - want).max()))
        assert np.array_equal(ydev.cpu().numpy(), want), (row[0], cls.__name__, leaky)


# ---- GPU: bf16 route -----------------------------------------------------------------------------------------------------
def _bf16_block(cls, row, seed, leaky=True):
    _, k, s, d, p, cin, cout, B, H, W = row
    m = cls(cin, cout, k, padding=p, stride=s, dilation=d, leakyReLU=leaky) if cls.__name__ != "Conv_BN_LeakyReLU" else \
        cls(cin, cout, k, padding=p, stride=s, dilation=d)
    g = torch.Generator().manual_seed(seed)
    conv = m.convs[0]
    K = cin * conv.kernel_size[0] * conv.kernel_size[1]
    with torch.no_grad():
        conv.weight.copy_((torch.rand(conv.weight.shape, generator=g) * 2 - 1) * (3.0 / K) ** 0.5)
        if conv.bias is not None:
            conv.bias.copy_(torch.rand(cout, generator=g) * 0.2 - 0.1)
        bn = m.convs[1] if isinstance(m.convs[1], nn.BatchNorm2d) else None
        if bn is not None:
            bn.weight.copy_(torch.rand(cout, generator=g) + 0.5)
            bn.bias.copy_(torch.rand(cout, generator=g) * 0.4 - 0.2)
            bn.running_mean.copy_(torch.rand(cout, generator=g) * 0.2 - 0.1)
            bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    x = torch.rand((B, cin, H, W), generator=g) * 2 - 1
    return m.eval(), x


def _ref_block(convs, x):
    """float64 eval-mode forward of nn.Sequential(conv, [BatchNorm2d], act) with torch's own functions"""
    y = x.detach().double().cpu()
    for mod in convs:
        if isinstance(mod, nn.Conv2d):
            y = F.conv2d(y, mod.weight.detach().double(), None if mod.bias is None else mod.bias.detach().double(), stride=mod.stride,
                         padding=mod.padding, dilation=mod.dilation)
        elif isinstance(mod, nn.BatchNorm2d):
            y = F.batch_norm(y, mod.running_mean.double(), mod.running_var.double(), mod.weight.detach().double(),
                             mod.bias.detach().double(), False, 0.0, mod.eps)
        elif isinstance(mod, nn.LeakyReLU):
            y = F.leaky_relu(y, mod.negative_slope)
        elif isinstance(mod, nn.ReLU):
            y = F.relu(y)
    return y


def _within_bf16(got, want, tag):
    err = np.abs(got - want)
    assert (err <= BF16_ATOL + BF16_RTOL * np.abs(want)).all(), (tag, float(err.max()), float(np.abs(want).max()))
    assert err.mean() < 0.01, tag


@pytest.mark.gpu
@pytest.mark.parametrize("row", GEOMS, ids=IDS)
def test_bf16_route_within_tolerance(row):
    from yolo355 import engine as E
    from yolo355.backbone.darknet import Conv_BN_LeakyReLU
    from yolo355.utils.modules import Conv2d, Conv2d_fuse, conv_geometry, folded_f32
    # Conv2d (BN folded in eval mode), ReLU and LeakyReLU
    for i, leaky in enumerate((True, False)):
        m, x = _bf16_block(Conv2d, row, 100 + i, leaky)
        want = _ref_block(m.convs, x).float().numpy()
        with torch.no_grad():
            y = m(x)
        assert y.shape == want.shape
        _within_bf16(y.numpy(), want, (row[0], "Conv2d", leaky))
    # Conv_BN_LeakyReLU with a residual, through conv2d_geom_bf16
    m, x = _bf16_block(Conv_BN_LeakyReLU, row, 200)
    want = _ref_block(m.convs, x)
    res = torch.rand(want.shape, generator=torch.Generator().manual_seed(201)) - 0.5
    with torch.no_grad():
        y = m(x, residual=res)
    w, b = folded_f32(m.convs)
    direct = E.conv2d_geom_bf16(x.numpy(), w, conv_geometry(m.convs[0]), b, residual=res.numpy(), neg_slope=0.1)
    assert np.array_equal(y.numpy(), direct)
    _within_bf16(direct, (want + res.double()).float().numpy(), (row[0], "residual"))
    # Conv2d_fuse on an input that is not a dyadic int8 tensor: the bf16 route
    m, x = _bf16_block(Conv2d_fuse, row, 300)
    with torch.no_grad():
        y = m(x)
    _within_bf16(y.numpy(), _ref(m.convs[0], x, 0.125), (row[0], "Conv2d_fuse bf16"))


@pytest.mark.gpu
@pytest.mark.parametrize("row", GEOMS, ids=IDS)
def test_bf16_route_is_exact_on_small_integers(row):
    """small integers are exact in bf16 and their sums exact in fp32: the fp32 result equals the float64 conv; with a residual and a
    bf16 result, too, while |y| < 256"""
    from yolo355 import engine as E
    from yolo355.utils.modules import conv_geometry
    _, k, s, d, p, cin, cout, B, H, W = row
    conv = _conv(row)
    rng = np.random.default_rng(7)
    x = rng.integers(-4, 5, size=(B, cin, H, W)).astype(np.float32)
    w = rng.integers(-2, 3, size=tuple(conv.weight.shape)).astype(np.float32)
    b = rng.integers(-8, 9, size=(cout,)).astype(np.float32)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w))
        conv.bias.copy_(torch.from_numpy(b))
    g = conv_geometry(conv)
    want = _ref(conv, torch.from_numpy(x))
    got = E.conv2d_geom_bf16(x, w, g, b, out_fp32=True)
    assert np.array_equal(got, want), (row[0], float(np.abs(got - want).max()))
    got = E.conv2d_geom_bf16(x, w, g, b, neg_slope=0.5, out_fp32=True)
    assert np.array_equal(got, np.where(want >= 0, want, want * 0.5).astype(np.float32))
    x1 = rng.integers(-1, 2, size=(B, cin, H, W)).astype(np.float32)
    w1 = rng.integers(-1, 2, size=tuple(conv.weight.shape)).astype(np.float32)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w1))
    want = _ref(conv, torch.from_numpy(x1))
    res = rng.integers(-16, 17, size=want.shape).astype(np.float32)
    want = want + res
    if np.abs(want).max() < 256:
        assert np.array_equal(E.conv2d_geom_bf16(x1, w1, g, b, residual=res), want.astype(np.float32))


# ---- GPU: cross-check against the existing kernels ------------------------------------------------------------------------
CROSS = [("3x3_p1", 3, 1, 1, 48, 40, 9, 11), ("3x3_p1_wide", 3, 1, 1, 200, 130, 13, 17), ("1x1", 1, 1, 0, 96, 35, 13, 17),
         ("3x3_s2_p1", 3, 2, 1, 64, 70, 9, 11)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CROSS, ids=[c[0] for c in CROSS])
def test_general_kernel_equals_the_existing_kernels(case):
    """the general-geometry entry points always run convgeom.hip: on the geometries of conv3x3_i8_raw (3x3 / pad 1, and 1x1 / 3x3
    stride 2 expressed through it) and of conv2d_bf16 they reproduce those kernels bit for bit"""
    from yolo355 import engine as E
    _, k, s, p, cin, cout, H, W = case
    g = E.conv_geom(k, s, 1, p)
    rng = np.random.default_rng(cin + cout)
    qi = rng.integers(-127, 128, size=(2, cin, H, W)).astype(np.int8)
    qw = rng.integers(-127, 128, size=(cout, cin, k, k)).astype(np.int8)
    qb = rng.integers(-127, 128, size=(cout,)).astype(np.int32)
    qw3 = qw if k == 3 else np.pad(qw, ((0, 0), (0, 0), (1, 1), (1, 1)))        # 1x1 = the centre tap of a 3x3
    for leaky, relu in ((True, False), (False, True), (False, False)):
        t, f = E.conv_geom_i8_raw(qi, qw, qb, 4, 9, 6, g, leaky=leaky, relu=relu)
        t3, f3 = E.conv3x3_i8_raw(qi, qw3, qb, 4, 9, 6, leaky=leaky, relu=relu)
        assert f == f3
        assert np.array_equal(t, t3[:, :, ::s, ::s]), (case[0], leaky, relu)
    x = rng.integers(-4, 5, size=(2, cin, H, W)).astype(np.float32)
    w = rng.integers(-2, 3, size=(cout, cin, k, k)).astype(np.float32)
    b = rng.integers(-8, 9, size=(cout,)).astype(np.float32)
    for slope, fp32 in ((1.0, True), (0.25, True), (0.5, False)):
        want = E.conv2d_bf16(x, w, b, stride=s, neg_slope=slope, out_fp32=fp32)
        assert np.array_equal(E.conv2d_geom_bf16(x, w, g, b, neg_slope=slope, out_fp32=fp32), want), (case[0], slope, fp32)


@pytest.mark.gpu
def test_one_operator_keeps_each_workspace_zeroed_for_its_own_geometry():
    """one bf16 operator object, 24 -> 40 channels, 3x3, stride 1: a map with a residual, a smaller map (another tile) without one,
    the smaller map with one -- the residual's workspace was last zeroed for the first map's layout.  Each output is bit-equal to
    conv2d_bf16, which runs a fresh operator, on the same data"""
    from yolo355 import engine as E
    from yolo355.synth import uniform_pm1
    cin, cout = 24, 40
    w = (uniform_pm1(41, (cout, cin, 3, 3)) * np.float32(1.0 / np.sqrt(cin * 9))).astype(np.float32)
    b = uniform_pm1(42, (cout,))
    op = E.ConvOp.bf16(w, b, neg_slope=0.1)
    try:
        for i, (shp, with_res) in enumerate((((2, cin, 14, 27), True), ((1, cin, 9, 11), False), ((1, cin, 9, 11), True))):
            x = uniform_pm1(50 + 2 * i, shp)
            res = uniform_pm1(51 + 2 * i, (shp[0], cout) + shp[2:]) if with_res else None
            rd = None if res is None else torch.from_numpy(res).cuda()
            got = op.forward(torch.from_numpy(x).cuda(), residual=rd).cpu().numpy()
            assert np.array_equal(got, E.conv2d_bf16(x, w, b, residual=res, neg_slope=0.1)), (i, shp, with_res)
    finally:
        op.close()


# ---- GPU: device-resident forms ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_resident_forms():
    from yolo355.utils.modules import Conv2d, Conv2d_fuse
    row = ("5x5_s2_d2", 5, 2, 2, 4, 96, 35, 3, 13, 17)
    # int8 route: CUDA in -> CUDA out on torch's current stream, equal to the host form and to the float64 conv
    m, x = _fused(Conv2d_fuse, row, True, 1)
    side = torch.cuda.Stream()
    xd = x.cuda()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(side):
            yd = m(xd)
        side.synchronize()
        yh = m(x)
    assert yd.is_cuda and yd.dtype == torch.float32 and not yh.is_cuda
    assert torch.equal(yd.cpu(), yh)
    assert np.array_equal(yh.numpy(), _ref(m.convs[0], x, 0.125))
    # an in-place weight update repacks (still dyadic: the exponent moves)
    with torch.no_grad():
        m.convs[0].weight.mul_(-0.5)
        yd2 = m(xd)
    assert not torch.equal(yd2, yd)
    assert np.array_equal(yd2.cpu().numpy(), _ref(m.convs[0], x, 0.125))
    # a non-dyadic input takes the bf16 route
    xn = x + 1e-3
    with torch.no_grad():
        yn = m(xn.cuda())
        yn_host = m(xn)
    assert yn.is_cuda and torch.equal(yn.cpu(), yn_host)
    assert not np.array_equal(yn_host.numpy(), _ref(m.convs[0], xn, 0.125))               # bf16, not the exact route
    _within_bf16(yn_host.numpy(), _ref(m.convs[0], xn, 0.125), "non-dyadic")
    # bf16 block: device == host form; an in-place BN update repacks
    mb, xb = _bf16_block(Conv2d, row, 5)
    with torch.no_grad():
        y1 = mb(xb.cuda())
        assert torch.equal(y1.cpu(), mb(xb))
        mb.convs[1].running_var.mul_(4.0)
        y2 = mb(xb.cuda())
    assert not torch.equal(y1, y2)
    _within_bf16(y2.cpu().numpy(), _ref_block(mb.convs, xb).float().numpy(), "bf16 after update")


# ---- GPU: composition ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_geometry_model_matches_torch():
    from yolo355.backbone.darknet import Conv_BN_LeakyReLU
    from yolo355.utils.modules import Conv2d
    torch.manual_seed(3)
    net = nn.Sequential(
        Conv2d(3, 32, 5, padding=2, stride=2, leakyReLU=True),        # 5x5 / s2 stem
        Conv2d(32, 48, 3, padding=2, dilation=2, leakyReLU=True),     # dilated 3x3
        Conv_BN_LeakyReLU(48, 64, 1, stride=2),                       # 1x1 / s2
        Conv2d(64, 40, 4, padding="same", leakyReLU=False),           # 'same' 4x4 (asymmetric)
    )
    for blk in net:
        conv, bn = blk.convs[0], blk.convs[1]
        K = conv.in_channels * conv.kernel_size[0] * conv.kernel_size[1]
        with torch.no_grad():
            conv.weight.uniform_(-1, 1).mul_((3.0 / K) ** 0.5)
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
    net.eval()
    x = torch.rand(2, 3, 37, 45) * 2 - 1
    with torch.no_grad():
        y = net(x.cuda())
    want = x.double()
    for blk in net:
        want = _ref_block(blk.convs, want)
    assert y.is_cuda and tuple(y.shape) == tuple(want.shape)
    _within_bf16(y.cpu().numpy(), want.float().numpy(), "mixed model")
