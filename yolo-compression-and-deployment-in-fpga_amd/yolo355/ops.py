"""The Python face of csrc/ops.hip: the operator-level C ABI (include/yolo355.h) -- ConvOp, whose weights live packed on the GPU,
the *_dev operators on CUDA tensors, the host-pointer operators on NumPy arrays, the fp32 detection head and the convolution
geometry helpers.  All compute is in libyolo355.so; there is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from ._handle import Handle, _require_gpu, split_dets


def _lib_on_gpu(device_id):
    """the library, for a host-pointer operator that is to run on GPU device_id"""
    lib = _ffi.lib()
    _require_gpu("cuda:%d" % int(device_id))
    return lib


def mfma_peak_i8(device_id=0, ms_target=50.0):
    """(Top/s, in-kernel clock in GHz) of back-to-back v_mfma_i32_16x16x64_i8 on this GPU (y355_mfma_peak_i8)."""
    t, c = C.c_float(), C.c_float()
    _ffi.check(_ffi.lib().y355_mfma_peak_i8(int(device_id), float(ms_target), C.byref(t), C.byref(c)))
    return float(t.value), float(c.value)


class ConvOp(Handle):
    """A convolution whose weights live packed on the GPU (y355_conv_op, include/yolo355.h): the device-resident form of
    conv2d_bf16 / conv3x3_i8_raw for callers whose tensors are CUDA tensors -- forward takes and returns CUDA tensors on
    torch's current stream, no tensor crosses to the host."""
    _destroy = "y355_conv_op_destroy"

    def __init__(self, handle, kind, cout, stride, device, geom=None):
        self.kind, self.cout, self.stride, self.device = kind, int(cout), int(stride), device
        self.geom = geom
        self._own(_ffi.lib(), handle)

    @classmethod
    def bf16(cls, w, bias, stride=1, neg_slope=1.0, device=None, geom=None):
        """geom (a y355_conv_geom, see conv_geom): any kernel / stride / dilation / padding on the general-geometry kernel; stride is
        then ignored"""
        dev = _require_gpu(device)
        wi = np.ascontiguousarray(w, dtype=np.float32)
        cout, cin, k, k2 = wi.shape
        bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        h = C.c_void_p()
        if geom is not None:
            g = _geom_for(geom, k, k2)
            _ffi.check(_ffi.lib().y355_conv_op_create_bf16_geom(dev.index, wi.ctypes.data, None if bi is None else bi.ctypes.data, cin, cout,
                                                                C.byref(g), float(neg_slope), C.byref(h)))
            return cls(h, "bf16", cout, g.stride_h, dev, g)
        if k != k2:
            raise ValueError("square kernels only")
        _ffi.check(_ffi.lib().y355_conv_op_create_bf16(dev.index, wi.ctypes.data, None if bi is None else bi.ctypes.data, cin, cout, k,
                                                       int(stride), float(neg_slope), C.byref(h)))
        return cls(h, "bf16", cout, stride, dev)

    @classmethod
    def int8(cls, q_w, q_b, e_w, e_b, leaky=True, relu=False, device=None, geom=None):
        """geom: as for bf16; without it the operator is 3x3 / stride 1 / pad 1"""
        dev = _require_gpu(device)
        qw = np.ascontiguousarray(q_w, dtype=np.int8)
        qb = np.ascontiguousarray(q_b, dtype=np.int32)
        h = C.c_void_p()
        if geom is not None:
            g = _geom_for(geom, qw.shape[2], qw.shape[3])
            _ffi.check(_ffi.lib().y355_conv_op_create_i8_geom(dev.index, qw.ctypes.data, qb.ctypes.data, qw.shape[1], qw.shape[0], C.byref(g),
                                                              int(e_w), int(e_b), _act_flag(leaky, relu), C.byref(h)))
            return cls(h, "int8", qw.shape[0], g.stride_h, dev, g)
        _ffi.check(_ffi.lib().y355_conv_op_create_i8(dev.index, qw.ctypes.data, qb.ctypes.data, qw.shape[1], qw.shape[0], int(e_w), int(e_b),
                                                     _act_flag(leaky, relu), C.byref(h)))
        return cls(h, "int8", qw.shape[0], 1, dev)

    def _out_hw(self, H, W):
        if self.geom is not None:
            return geom_out_size(self.geom, H, W)
        if self.kind == "bf16" and self.stride == 2:
            return (H + 1) // 2, (W + 1) // 2
        return H, W

    def forward(self, x, residual=None, out_fp32=False):
        """bf16 form: x CUDA float32 [B,cin,H,W] -> CUDA float32 [B,cout,Ho,Wo] (asynchronous, torch's current stream)."""
        x = x.detach().to(dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        Ho, Wo = self._out_hw(H, W)
        out = torch.empty((B, self.cout, Ho, Wo), dtype=torch.float32, device=x.device)
        r = None if residual is None else residual.detach().to(dtype=torch.float32).contiguous()
        if r is not None and tuple(r.shape) != tuple(out.shape):
            raise ValueError("residual shape %s, expected %s" % (tuple(r.shape), tuple(out.shape)))
        _ffi.check(self._lib.y355_conv_op_forward(self._h, x.data_ptr(), None if r is None else r.data_ptr(), B, H, W, 1 if out_fp32 else 0,
                                                  out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
        return out

    def forward_i8(self, x):
        """int8 form: Conv2d_fuse on a dyadic CUDA tensor, exact; returns None when x is not a dyadic int8 tensor."""
        x = x.detach().to(dtype=torch.float32).contiguous()
        B, _, H, W = x.shape
        Ho, Wo = self._out_hw(H, W)
        out = torch.empty((B, self.cout, Ho, Wo), dtype=torch.float32, device=x.device)
        sa, exact = C.c_int32(), C.c_int32()
        _ffi.check(self._lib.y355_conv_op_forward_i8(self._h, x.data_ptr(), B, H, W, out.data_ptr(),
                                                     torch.cuda.current_stream(x.device).cuda_stream, C.byref(sa), C.byref(exact)))
        return out if exact.value else None


# ---- element-wise operators: the *_dev forms on CUDA tensors, the host-pointer forms on NumPy arrays ------------------------
def _dev_unary(fn_name, x, out_shape, *args):
    """one of the y355_*_f32_dev operators on a CUDA tensor, on torch's current stream"""
    x = x.detach().to(dtype=torch.float32).contiguous()
    out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    B, Cc, H, W = x.shape
    _ffi.check(getattr(_ffi.lib(), fn_name)(x.data_ptr(), B, Cc, H, W, *args, out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
    return out


def _host_unary(fn_name, x, dtype, device_id, out_shape, *args):
    """the host-pointer form of the same: a NumPy NCHW array of dtype in, out_shape(B, C, H, W) of it out"""
    lib = _lib_on_gpu(device_id)
    xi = np.ascontiguousarray(x, dtype=dtype)
    B, Cc, H, W = xi.shape
    out = np.empty(out_shape(B, Cc, H, W), dtype)
    _ffi.check(getattr(lib, fn_name)(int(device_id), xi.ctypes.data, B, Cc, H, W, *args, out.ctypes.data))
    return out


def reorg_f32_dev(x, stride):
    B, Cc, H, W = x.shape
    s = int(stride)
    return _dev_unary("y355_reorg_f32_dev", x, (B, Cc * s * s, H // s, W // s), s)


def spp_f32_dev(x):
    B, Cc, H, W = x.shape
    return _dev_unary("y355_spp_f32_dev", x, (B, 4 * Cc, H, W))


def maxpool2x2_f32_dev(x):
    B, Cc, H, W = x.shape
    return _dev_unary("y355_maxpool2x2_f32_dev", x, (B, Cc, H // 2, W // 2))


def upsample2x_f32_dev(x):
    B, Cc, H, W = x.shape
    return _dev_unary("y355_upsample2x_f32_dev", x, (B, Cc, 2 * H, 2 * W))


def reorg_f32(x, stride, device_id=0):
    """utils.modules.reorg_layer.forward on fp32 NCHW (y355_reorg_f32); bit-exact data movement."""
    s = int(stride)
    return _host_unary("y355_reorg_f32", x, np.float32, device_id, lambda B, Cc, H, W: (B, Cc * s * s, H // max(s, 1), W // max(s, 1)), s)


def spp_f32(x, device_id=0):
    """utils.modules.SPP.forward on fp32 NCHW (y355_spp_f32); bit-exact."""
    return _host_unary("y355_spp_f32", x, np.float32, device_id, lambda B, Cc, H, W: (B, 4 * Cc, H, W))


def maxpool2x2_f32(x, device_id=0):
    """nn.MaxPool2d((2, 2), 2) on fp32 NCHW (y355_maxpool2x2_f32); bit-exact."""
    return _host_unary("y355_maxpool2x2_f32", x, np.float32, device_id, lambda B, Cc, H, W: (B, Cc, H // 2, W // 2))


def upsample2x_f32(x, device_id=0):
    """F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=True) on fp32 NCHW (y355_upsample2x_f32)."""
    return _host_unary("y355_upsample2x_f32", x, np.float32, device_id, lambda B, Cc, H, W: (B, Cc, 2 * H, 2 * W))


def maxpool2x2_i8(q, device_id=0):
    """Stand-alone 2x2 / stride 2 max-pool on int8 NCHW (y355_maxpool2x2_i8)."""
    return _host_unary("y355_maxpool2x2_i8", q, np.int8, device_id, lambda B, Cc, H, W: (B, Cc, H // 2, W // 2))


def quantize_input_f32_i8(x, sa, device_id=0):
    """Stand-alone input fake-quant (y355_quantize_input_f32_i8): (q int8 like x, clamped count)."""
    lib = _lib_on_gpu(device_id)
    xf = np.ascontiguousarray(x, dtype=np.float32)
    q = np.empty(xf.shape, np.int8)
    c = C.c_int64()
    _ffi.check(lib.y355_quantize_input_f32_i8(int(device_id), xf.ctypes.data, xf.size, int(sa), q.ctypes.data, C.byref(c)))
    return q, c.value


# ---- int8 convolutions on host pointers -------------------------------------------------------------------------------------
def _act_flag(leaky, relu):
    if leaky and relu:
        raise ValueError("LeakyReLU and ReLU are exclusive")
    return _ffi.OP_LEAKY if leaky else (_ffi.OP_RELU if relu else 0)


def conv3x3_i8_fused(q_in, q_w, q_b, sa_in, e_w, e_b, sa_out, leaky=True, pool=False, device_id=0, relu=False):
    """Operator-level fused layer (y355_conv3x3_i8_fused): numpy int8 NCHW in/out.  relu=True (with leaky=False):
    the ReLU epilogue of Conv2d_fuse(leakyReLU=False) (utils/modules.py:26)."""
    lib = _lib_on_gpu(device_id)
    qi = np.ascontiguousarray(q_in, dtype=np.int8)
    qw = np.ascontiguousarray(q_w, dtype=np.int8)
    qb = np.ascontiguousarray(q_b, dtype=np.int32)
    B, cin, H, W = qi.shape
    cout = qw.shape[0]
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    out = np.empty((B, cout, Ho, Wo), np.int8)
    st = _ffi.LayerStats()
    flags = _act_flag(leaky, relu) | (_ffi.OP_POOL if pool else 0)
    _ffi.check(lib.y355_conv3x3_i8_fused(int(device_id), qi.ctypes.data, qw.ctypes.data, qb.ctypes.data, B, cin, cout,
                                         H, W, int(sa_in), int(e_w), int(e_b), int(sa_out), flags,
                                         out.ctypes.data, C.byref(st)))
    return out, dict(absmax_t=st.absmax_t, frac_bits=st.frac_bits, saturated=st.saturated, guard=st.guard)


def _conv_i8_raw(q_in, q_w, q_b, sa_in, e_w, e_b, geom, leaky, relu, device_id):
    """y355_conv3x3_i8_raw (geom None) or y355_conv_geom_i8_raw: the two differ by the geometry argument and the output size"""
    lib = _lib_on_gpu(device_id)
    qi = np.ascontiguousarray(q_in, dtype=np.int8)
    qw = np.ascontiguousarray(q_w, dtype=np.int8)
    qb = np.ascontiguousarray(q_b, dtype=np.int32)
    B, cin, H, W = qi.shape
    cout = qw.shape[0]
    if geom is None:
        fn, mid, (Ho, Wo) = lib.y355_conv3x3_i8_raw, (), (H, W)
    else:
        g = _geom_for(geom, qw.shape[2], qw.shape[3])
        fn, mid, (Ho, Wo) = lib.y355_conv_geom_i8_raw, (C.byref(g),), geom_out_size(g, H, W)
    out = np.empty((B, cout, Ho, Wo), np.int64)
    fb = C.c_int32()
    _ffi.check(fn(int(device_id), qi.ctypes.data, qw.ctypes.data, qb.ctypes.data, B, cin, cout, H, W, *mid,
                  int(sa_in), int(e_w), int(e_b), _act_flag(leaky, relu), out.ctypes.data, C.byref(fb)))
    return out, fb.value


def conv3x3_i8_raw(q_in, q_w, q_b, sa_in, e_w, e_b, leaky=True, device_id=0, relu=False):
    """conv + bias + LeakyReLU(0.125) (or ReLU, or nothing) without requantisation (y355_conv3x3_i8_raw):
    returns (t' int64 [B,cout,H,W], F') with value = t' / 2^F'."""
    return _conv_i8_raw(q_in, q_w, q_b, sa_in, e_w, e_b, None, leaky, relu, device_id)


def conv_geom_i8_raw(q_in, q_w, q_b, sa_in, e_w, e_b, geom, leaky=True, device_id=0, relu=False):
    """conv3x3_i8_raw for any geometry (y355_conv_geom_i8_raw): (t' int64 [B,cout,Ho,Wo], F') with value = t' / 2^F', exact"""
    return _conv_i8_raw(q_in, q_w, q_b, sa_in, e_w, e_b, geom, leaky, relu, device_id)


# ---- bf16 convolutions on host pointers -------------------------------------------------------------------------------------
def _conv_bf16(x, w, bias, residual, neg_slope, out_fp32, device_id, geom=None, stride=1):
    """y355_conv2d_bf16 (geom None: square kernel, stride 1 or 2) or y355_conv2d_geom_bf16"""
    lib = _lib_on_gpu(device_id)
    xi = np.ascontiguousarray(x, dtype=np.float32)
    wi = np.ascontiguousarray(w, dtype=np.float32)
    B, Cin, H, W = xi.shape
    Cout, Cin2, kh, kw = wi.shape
    if Cin2 != Cin or (geom is None and kh != kw):
        raise ValueError("weight shape %s does not match the input's %d channels" % (wi.shape, Cin))
    if geom is None:
        s = int(stride)
        fn, mid, (Ho, Wo) = lib.y355_conv2d_bf16, (int(kh), s), ((H + 1) // 2, (W + 1) // 2) if s == 2 else (H, W)
    else:
        g = _geom_for(geom, kh, kw)
        fn, mid, (Ho, Wo) = lib.y355_conv2d_geom_bf16, (C.byref(g),), geom_out_size(g, H, W)
    bi = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
    ri = None if residual is None else np.ascontiguousarray(residual, dtype=np.float32)
    if ri is not None and ri.shape != (B, Cout, Ho, Wo):
        raise ValueError("residual shape %s, expected %s" % (ri.shape, (B, Cout, Ho, Wo)))
    out = np.empty((B, Cout, Ho, Wo), np.float32)
    _ffi.check(fn(int(device_id), xi.ctypes.data, wi.ctypes.data, None if bi is None else bi.ctypes.data,
                  None if ri is None else ri.ctypes.data, B, Cin, Cout, H, W, *mid, float(neg_slope), 1 if out_fp32 else 0,
                  out.ctypes.data))
    return out


def conv2d_bf16(x, w, bias=None, residual=None, stride=1, neg_slope=1.0, out_fp32=False, device_id=0):
    """conv (1x1, or 3x3 pad 1; stride 1, or 2 for 3x3) + bias + LeakyReLU(neg_slope) [+ residual] on the bf16 MFMA
    (y355_conv2d_bf16).  fp32 NCHW in and out; operands and result are rounded to bf16."""
    return _conv_bf16(x, w, bias, residual, neg_slope, out_fp32, device_id, stride=stride)


def conv2d_geom_bf16(x, w, geom, bias=None, residual=None, neg_slope=1.0, out_fp32=False, device_id=0):
    """conv2d_bf16's arithmetic for any geometry (y355_conv2d_geom_bf16): fp32 NCHW in and out, operands and result rounded to bf16"""
    return _conv_bf16(x, w, bias, residual, neg_slope, out_fp32, device_id, geom=geom)


def head_f32(preds, strides, anchors, num_classes, input_size, wh_mul, conf_thresh, nms_thresh, max_det=None, device_id=0,
             max_candidates=None, route=None, return_candidates=False):
    """Detection head on fp32 prediction maps (y355_head_f32_ex).  preds: list (1 to 3 levels) of [B, A*(5+C), Hs, Ws];
    anchors: [nlev][A][2].  Returns a list over the batch of (boxes [n,4] normalised, scores [n], classes int64 [n]).
    max_candidates (default 4096, up to min(anchors per image, 65536)): the most anchors of an image that may pass
    conf_thresh; route 1: every image through the NMS route for more than 4096 candidates.  return_candidates: also the
    decode of every anchor, (list, (boxes [B,N,4], scores [B,N], classes int32 [B,N]))."""
    lib = _lib_on_gpu(device_id)
    ps = [np.ascontiguousarray(p, dtype=np.float32) for p in preds]
    nlev = len(ps)
    B = ps[0].shape[0]
    an = np.ascontiguousarray(anchors, dtype=np.float32).reshape(nlev, -1, 2)
    A = an.shape[1]
    hs = (C.c_int * nlev)(*[p.shape[2] for p in ps])
    ws = (C.c_int * nlev)(*[p.shape[3] for p in ps])
    st = (C.c_float * nlev)(*[float(s) for s in strides])
    ptrs = (C.c_void_p * nlev)(*[p.ctypes.data for p in ps])
    cap = 4096 if max_candidates is None else int(max_candidates)
    na = sum(p.shape[2] * p.shape[3] * A for p in ps)
    N = min(na, cap)                                                 # the head keeps at most `cap` candidates per image
    md = N if max_det is None else min(int(max_det), N)
    boxes = np.zeros((B, md, 4), np.float32)
    scores = np.zeros((B, md), np.float32)
    cls = np.zeros((B, md), np.int32)
    count = np.zeros((B,), np.int32)
    cand = (np.zeros((B, na, 4), np.float32), np.zeros((B, na), np.float32), np.zeros((B, na), np.int32)) if return_candidates else None
    _ffi.check(lib.y355_head_f32_ex(int(device_id), nlev, ptrs, hs, ws, st, an.ctypes.data_as(C.POINTER(C.c_float)), A, int(num_classes),
                                    int(input_size[0]), int(input_size[1]), float(wh_mul), float(conf_thresh), float(nms_thresh), B, md,
                                    cap, 0 if route is None else int(route), boxes.ctypes.data, scores.ctypes.data, cls.ctypes.data,
                                    count.ctypes.data, *([c.ctypes.data for c in cand] if cand else [None, None, None])))
    out = split_dets(boxes, scores, cls, count, B)
    return (out, cand) if return_candidates else out


# ---- general convolution geometry (y355_conv_geom, convgeom.hip) ---------------------------------------------------------
def conv_geom(kernel_size, stride=1, dilation=1, padding=0):
    """y355_conv_geom from int-or-pair kernel_size / stride / dilation and padding given as an int, a pair (h, w) or four pads
    (top, bottom, left, right)"""
    def pair(v):
        return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))
    kh, kw = pair(kernel_size)
    sh, sw = pair(stride)
    dh, dw = pair(dilation)
    if np.isscalar(padding):
        pads = (int(padding),) * 4
    elif len(padding) == 2:
        pads = (int(padding[0]), int(padding[0]), int(padding[1]), int(padding[1]))
    else:
        pads = tuple(int(p) for p in padding)
    return _ffi.ConvGeom(kh, kw, sh, sw, dh, dw, *pads)


def _as_geom(geom):
    return geom if isinstance(geom, _ffi.ConvGeom) else _ffi.ConvGeom(*[int(v) for v in geom])


def _geom_for(geom, kh, kw):
    g = _as_geom(geom)
    if (g.kh, g.kw) != (kh, kw):
        raise ValueError("geometry %r does not match a %dx%d weight" % (g, kh, kw))
    return g


def geom_out_size(geom, height, width):
    """(Ho, Wo) of a geometry on a height x width map (y355_conv_geom_out_size; raises Y355Error outside the limits).  No GPU."""
    g = _as_geom(geom)
    ho, wo = C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().y355_conv_geom_out_size(C.byref(g), int(height), int(width), C.byref(ho), C.byref(wo)))
    return ho.value, wo.value
