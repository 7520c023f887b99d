"""A differentiable convolution of any geometry the operator API accepts, on the GPU: ctypes binding of
include/yolo355_convgrad.h (csrc/convgrad.hip, the companion library libyolo355_convgrad.so, loaded the first time it is asked
for), the handle ConvGrad, `conv2d`, a torch.autograd.Function over CUDA fp32 tensors with the activation fused, TrainableConv,
an nn.Module over a drop-in block's `.convs` that shares its parameters, and `trainable(model)`, which finds those blocks.
Forward, data gradient and weight gradient run on the bf16 MFMA from fp32 parameters that stay on the device; BatchNorm,
pooling, upsample, concat, reorg and the optimiser stay torch's, the loss is yolo355.grad.YoloCriterion.  The arithmetic
contract is DESIGN.md section 6p.  No CPU path: without a GPU every device entry point raises."""
import ctypes as C
import os
import types

import torch
import torch.nn as nn

from . import _ffi
from ._handle import Handle, _require_gpu

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_convgrad.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_convgrad.h"))

P = C.POINTER
_V, _I = C.c_void_p, C.c_int32
Geom = _ffi.ConvGeom                     # y355_convgrad_geom has y355_conv_geom's ten fields
_SIGS = {
    "y355_convgrad_last_error": (C.c_char_p, []),
    "y355_convgrad_out_size": (C.c_int, [P(Geom), _I, _I, P(_I), P(_I)]),
    "y355_convgrad_create": (C.c_int, [_I, _I, _I, P(Geom), C.c_float, P(_V)]),
    "y355_convgrad_destroy": (None, [_V]),
    "y355_convgrad_forward": (C.c_int, [_V, _V, _V, _V, _I, _I, _I, _V, _V]),
    "y355_convgrad_backward": (C.c_int, [_V, _V, _V, _V, _V, _I, _I, _I, _V, _V, _V, _V]),
    "y355_convgrad_wgrad_plan": (C.c_int, [_V, _I, _I, _I, P(_I)]),
}
_lib = None
# libyolo355_convgrad.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_convgrad_", "extensions first (make -C csrc)")

MAX_CHANNELS = 4096


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def geometry(kernel_size, stride=1, padding=0, dilation=1):
    """the ConvGeom of nn.Conv2d's arguments through utils.modules.conv_geometry: ints or pairs, padding also 'same' / 'valid'"""
    from .utils.modules import conv_geometry
    if isinstance(kernel_size, Geom):
        return kernel_size
    pad = padding if isinstance(padding, str) else _pair(padding)
    return conv_geometry(types.SimpleNamespace(groups=1, padding_mode="zeros", kernel_size=_pair(kernel_size), stride=_pair(stride),
                                               dilation=_pair(dilation), padding=pad))


def out_size(geom, height, width):
    """(Ho, Wo) of a geometry on a height x width map; no GPU needed"""
    ho, wo = _I(), _I()
    check(lib().y355_convgrad_out_size(C.byref(geom), int(height), int(width), C.byref(ho), C.byref(wo)))
    return ho.value, wo.value


def _stream(device):
    with torch.cuda.device(device):
        return torch.cuda.current_stream(device).cuda_stream


class ConvGrad(Handle):
    """One convolution (cin, cout, geometry, slope) of y355_convgrad: forward and backward on device tensors, on torch's
    current stream.  Stateless between calls; the workspaces inside are reused in stream order, so a handle serves one stream
    at a time.  last_request: (dx, dw, db) asked of the last backward."""
    _destroy = "y355_convgrad_destroy"

    def __init__(self, cin, cout, geom, neg_slope=1.0, device=None):
        l = lib()
        self.device = _require_gpu(device)
        self.cin, self.cout, self.geom, self.neg_slope = int(cin), int(cout), geom, float(neg_slope)
        self.last_request = None
        h = _V()
        check(l.y355_convgrad_create(self.device.index, self.cin, self.cout, C.byref(geom), self.neg_slope, C.byref(h)))
        self._own(l, h)

    def _t(self, t, shape, name):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != torch.float32:
            raise ValueError("%s: expected a float32 tensor on %s (yolo355 has no CPU path)" % (name, self.device))
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
        return t.detach().contiguous()

    def _operands(self, x, weight):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.cin:
            raise ValueError("x: expected [B,%d,H,W]" % self.cin)
        x = self._t(x, None, "x")
        w = self._t(weight, (self.cout, self.cin, self.geom.kh, self.geom.kw), "weight")
        B, _, H, W = (int(v) for v in x.shape)
        return x, w, B, H, W, out_size(self.geom, H, W)

    def forward(self, x, weight, bias=None):
        """y [B, cout, Ho, Wo] = act(conv(rb(x), rb(weight)) + bias)"""
        x, w, B, H, W, (ho, wo) = self._operands(x, weight)
        b = None if bias is None else self._t(bias, (self.cout,), "bias")
        y = torch.empty((B, self.cout, ho, wo), dtype=torch.float32, device=self.device)
        check(self._lib.y355_convgrad_forward(self._h, x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(), B, H, W, y.data_ptr(),
                                              _stream(self.device)))
        return y

    def backward(self, x, weight, y, dy, need_dx=True, need_dw=True, need_db=True):
        """(dx, dw, db) of the gradient dy arriving at y; an output that is not needed is None and is not computed.  y may be
        None when neg_slope is 1."""
        x, w, B, H, W, (ho, wo) = self._operands(x, weight)
        dy = self._t(dy, (B, self.cout, ho, wo), "dy")
        yy = None if y is None else self._t(y, (B, self.cout, ho, wo), "y")
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty_like(w) if need_dw else None
        db = torch.empty((self.cout,), dtype=torch.float32, device=self.device) if need_db else None
        self.last_request = (bool(need_dx), bool(need_dw), bool(need_db))
        ptr = lambda t: None if t is None else t.data_ptr()
        check(self._lib.y355_convgrad_backward(self._h, x.data_ptr(), w.data_ptr(), ptr(yy), dy.data_ptr(), B, H, W, ptr(dx), ptr(dw), ptr(db),
                                               _stream(self.device)))
        return dx, dw, db

    def wgrad_plan(self, batch, height, width):
        """{npix, runs, chunk, last} of the weight gradient at that shape, from the function the backward launches from"""
        out = (_I * 4)()
        check(self._lib.y355_convgrad_wgrad_plan(self._h, int(batch), int(height), int(width), out))
        return dict(npix=int(out[0]), runs=int(out[1]), chunk=int(out[2]), last=int(out[3]))


_handles = {}


def _handle_for(geom, cin, cout, neg_slope, device):
    """the cached handle of (geometry, channels, slope, device) -- and of torch's current stream, since a handle's workspaces
    serve one stream at a time"""
    key = (geom.astuple(), int(cin), int(cout), float(neg_slope), device.index, _stream(device))
    h = _handles.get(key)
    if h is None or h._h is None:
        h = _handles[key] = ConvGrad(cin, cout, geom, neg_slope, device)
    return h


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom, neg_slope):
        h = _handle_for(geom, weight.shape[1], weight.shape[0], neg_slope, x.device)
        y = h.forward(x, weight, bias)
        ctx.handle = h
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db = ctx.handle.backward(x, weight, y, dy.to(torch.float32), need[0], need[1], need[2])
        return dx, dw, db, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, neg_slope=1.0):
    """F.conv2d (groups 1, zero padding) followed by LeakyReLU(neg_slope) -- 1: no activation, 0: ReLU -- on CUDA float32
    tensors, with a graph: forward, data gradient and weight gradient on the bf16 MFMA, on torch's current stream.  padding:
    an int, a pair, 'same' or 'valid'.  Only the gradients autograd asks for are computed."""
    for t, name in ((x, "x"), (weight, "weight")) + (() if bias is None else ((bias, "bias"),)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError("%s: expected a CUDA float32 tensor (yolo355 has no CPU path)" % name)
    if weight.dim() != 4:
        raise ValueError("weight: expected [cout, cin, kh, kw]")
    geom = geometry((int(weight.shape[2]), int(weight.shape[3])), stride, padding, dilation)
    return _Conv2dFn.apply(x, weight, bias, geom, float(neg_slope))


def _split(convs):
    """(conv, BatchNorm2d or None, activation module or None, slope) of nn.Sequential(conv, [BatchNorm2d], [LeakyReLU | ReLU])
    or of a bare nn.Conv2d"""
    mods = list(convs) if isinstance(convs, nn.Sequential) else [convs]
    if not mods or not isinstance(mods[0], nn.Conv2d):
        raise TypeError("TrainableConv: expected nn.Sequential(nn.Conv2d, [BatchNorm2d], [LeakyReLU | ReLU]) or an nn.Conv2d")
    bn = act = None
    slope = 1.0
    for m in mods[1:]:
        if isinstance(m, nn.BatchNorm2d) and bn is None and act is None:
            bn = m
        elif isinstance(m, nn.LeakyReLU) and act is None:
            act, slope = m, float(m.negative_slope)
        elif isinstance(m, nn.ReLU) and act is None:
            act, slope = m, 0.0
        else:
            raise TypeError("TrainableConv: unexpected %s in the block" % type(m).__name__)
    return mods[0], bn, act, slope


class TrainableConv(nn.Module):
    """The training form of a drop-in block (utils.modules.Conv2d / Conv2d_fuse / Conv2d_fuse_nobias,
    backbone.darknet.Conv_BN_LeakyReLU) or of a bare nn.Conv2d: it holds the block's own `.convs`, so parameters, buffers and
    state_dict keys are the block's and an optimiser step on either is seen by both (the inference drop-in repacks when a
    parameter's version changes).  conv -> act runs as one fused call; conv -> BatchNorm2d -> act runs the convolution with no
    activation, then torch's batch_norm in the module's training or eval mode and torch's activation."""

    def __init__(self, convs):
        super().__init__()
        _split(convs)
        self.convs = convs

    def forward(self, x):
        conv, bn, act, slope = _split(self.convs)
        from .utils.modules import conv_geometry
        geom = conv_geometry(conv)
        if bn is None:
            return _Conv2dFn.apply(x, conv.weight, conv.bias, geom, slope)
        y = bn(_Conv2dFn.apply(x, conv.weight, conv.bias, geom, 1.0))
        return act(y) if act is not None else y


def trainable(model):
    """{qualified name: TrainableConv} of every block of `model` that has a `.convs` Sequential starting with an nn.Conv2d, and
    of every nn.Conv2d outside such a block (a bare `pred`), in module order.  The wrappers share the model's parameters:
    optimise model.parameters() and compose the forward from the wrappers."""
    out, inside = {}, []
    for name, m in model.named_modules():
        if any(p == "" or name == p or name.startswith(p + ".") for p in inside):
            continue
        convs = getattr(m, "convs", None)
        if isinstance(convs, nn.Sequential) and len(convs) and isinstance(convs[0], nn.Conv2d):
            out[name] = TrainableConv(convs)
            inside.append(name)
        elif isinstance(m, nn.Conv2d):
            out[name] = TrainableConv(m)
    return out
