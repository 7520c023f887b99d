"""The reference's training losses with their gradient with respect to the prediction maps, on the GPU: ctypes binding of
include/yolo355_grad.h (csrc/grad.hip, the companion library libyolo355_grad.so, loaded the first time it is asked for), the
handle YoloLossGrad, the autograd module YoloCriterion (`total_loss.backward()` on a torch model whose head output goes through
it) and `loss`, a drop-in with the signature of tools.loss (tools.py:392-435) whose four results carry a graph.  The value is
yolo355.loss's bit for bit.  The backward pass of the network itself and the optimiser are the caller's framework's.  No CPU
path: without a GPU every entry point raises."""
import ctypes as C
import os

import numpy as np
import torch

from . import _ffi
from ._handle import Handle, _require_gpu
from .loss import IGNORE_THRESH, MAX_ANCHORS, MAX_LEVELS, TARGET_FIELDS, LossConfig, _as_list, pack_labels

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_grad.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_grad.h"))

P = C.POINTER
_SIGS = {
    "y355_grad_last_error": (C.c_char_p, []),
    "y355_grad_create": (C.c_int, [P(LossConfig), P(C.c_void_p)]),
    "y355_grad_destroy": (None, [C.c_void_p]),
    "y355_grad_num_anchors_total": (C.c_int, [C.c_void_p]),
    "y355_grad_set_labels": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_double), C.c_int32]),
    "y355_grad_targets_dev": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_void_p)]),
    "y355_grad_forward_backward": (C.c_int, [C.c_void_p, P(C.c_void_p), C.c_void_p, C.c_int32, C.c_void_p, P(C.c_void_p), C.c_void_p,
                                             P(C.c_double), P(C.c_double)]),
    "y355_grad_backward": (C.c_int, [C.c_void_p, P(C.c_void_p), C.c_void_p, C.c_int32, C.c_void_p, P(C.c_void_p), C.c_void_p]),
    "y355_grad_flat": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                 C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_double), P(C.c_double)]),
}
_lib = None
# libyolo355_grad.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_grad_", "extensions first (make -C csrc)")


class _DeviceArray:
    """a device pointer as torch.as_tensor takes it (the CUDA array interface): no copy"""

    def __init__(self, ptr, shape, keep):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f4", data=(int(ptr), False), version=2, strides=None)
        self._keep = keep


def _stream(device):
    with torch.cuda.device(device):
        return torch.cuda.current_stream(device).cuda_stream


def _upstream(upstream, device):
    """None (= {0, 0, 0, 1}) or four values for conf, cls, txtytwth, total as fp32 on the device"""
    if upstream is None:
        return None
    u = torch.as_tensor(upstream).to(device=device, dtype=torch.float32).contiguous()
    if u.numel() != 4:
        raise ValueError("upstream: expected four values (conf, cls, txtytwth, total), got %s" % (tuple(u.shape),))
    return u


class YoloLossGrad(Handle):
    """Targets, losses and their gradient of one head geometry (y355_grad); the constructor arguments of loss.YoloLoss."""
    _destroy = "y355_grad_destroy"

    def __init__(self, input_size, strides, anchors, num_classes, multi=None, ignore_thresh=IGNORE_THRESH, obj_weight=5.0,
                 noobj_weight=1.0, max_batch=1, max_labels_per_image=64, device=None):
        l = lib()
        self.device = _require_gpu(device)
        self.multi = (not np.isscalar(strides)) if multi is None else bool(multi)
        self.strides = _as_list(strides)
        self.input_size = [int(input_size[0]), int(input_size[1])]
        anchors = np.asarray(anchors, np.float64).reshape(-1, 2)
        nlev = len(self.strides)
        if nlev < 1 or nlev > MAX_LEVELS or len(anchors) % nlev or not 1 <= len(anchors) // nlev <= MAX_ANCHORS:
            raise ValueError("expected 1..3 strides and 1..16 anchors per level, got %d strides and %d anchors" % (nlev, len(anchors)))
        self.anchors, self.num_anchors, self.num_classes = anchors, len(anchors) // nlev, int(num_classes)
        self.max_batch, self.max_labels_per_image = int(max_batch), int(max_labels_per_image)
        h, w = self.input_size
        self.grids = [(h // s, w // s) for s in self.strides] if self.multi else \
            [(int(round(h / self.strides[0])), int(round(w / self.strides[0])))]
        cfg = LossConfig()                                        # zeroed; the library has no default_config of its own
        cfg.device_id, cfg.num_levels, cfg.num_anchors, cfg.num_classes = self.device.index, nlev, self.num_anchors, self.num_classes
        for i, ((hs, ws), s) in enumerate(zip(self.grids, self.strides)):
            cfg.hs[i], cfg.ws[i], cfg.stride[i] = hs, ws, s
        for i, v in enumerate(anchors.reshape(-1)):
            cfg.anchors[i] = float(v)
        cfg.in_h, cfg.in_w = h, w
        cfg.anchors_in_grid_units = 0 if self.multi else 1
        cfg.wh_mul = 1.0 if self.multi else float(self.strides[0])
        cfg.ignore_thresh, cfg.obj_weight, cfg.noobj_weight = float(ignore_thresh), float(obj_weight), float(noobj_weight)
        cfg.max_batch, cfg.max_labels_per_image = self.max_batch, self.max_labels_per_image
        hd = C.c_void_p()
        check(l.y355_grad_create(C.byref(cfg), C.byref(hd)))
        self._own(l, hd)
        self.num_anchors_total = l.y355_grad_num_anchors_total(hd)
        self._batch = 0

    def set_labels(self, label_lists):
        """label_lists: per image a list of [xmin, ymin, xmax, ymax, cls] (coordinates in [0, 1]); builds the dense target
        tensor [B, N, 11] on the device, labels applied in list order"""
        offsets, labels = pack_labels(label_lists)
        self._batch = 0
        check(self._lib.y355_grad_set_labels(self._h, offsets.ctypes.data_as(P(C.c_int32)), labels.ctypes.data_as(P(C.c_double)),
                                             len(label_lists)))
        self._batch = len(label_lists)

    def targets(self):
        """float32 [B, N, 11] of the last set_labels as a torch view of the handle's device tensor (no copy): valid until
        the next set_labels or close()"""
        p = C.c_void_p()
        check(self._lib.y355_grad_targets_dev(self._h, max(self._batch, 1), C.byref(p)))
        return torch.as_tensor(_DeviceArray(p.value, (self._batch, self.num_anchors_total, TARGET_FIELDS), self), device=self.device)

    def _maps(self, pred_maps):
        if isinstance(pred_maps, (np.ndarray, torch.Tensor)):
            pred_maps = [pred_maps]
        if len(pred_maps) != len(self.strides):
            raise ValueError("expected %d prediction maps, got %d" % (len(self.strides), len(pred_maps)))
        maps = [torch.as_tensor(p).detach().to(device=self.device, dtype=torch.float32).contiguous() for p in pred_maps]
        B = int(maps[0].shape[0])
        ch = self.num_anchors * (5 + self.num_classes)
        for m, (hs, ws) in zip(maps, self.grids):
            if tuple(m.shape) != (B, ch, hs, ws):
                raise ValueError("expected a prediction map [%d,%d,%d,%d], got %s" % (B, ch, hs, ws, tuple(m.shape)))
        return maps, B

    def _target(self, target, B):
        if target is None:
            return None
        tgt = torch.as_tensor(target).detach().to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(tgt.shape) != (B, self.num_anchors_total, TARGET_FIELDS):
            raise ValueError("expected a target [%d,%d,11], got %s" % (B, self.num_anchors_total, tuple(tgt.shape)))
        return tgt

    @staticmethod
    def _ptrs(tensors):
        return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _grads(self, maps, grad_maps):
        """the maps a launch fills: fresh ones, or the caller's (fp32, contiguous, on this device, of the predictions' shapes)"""
        if grad_maps is None:
            return [torch.empty_like(m) for m in maps]
        for g, m in zip(grad_maps, maps):
            if not (isinstance(g, torch.Tensor) and g.device == m.device and g.dtype == torch.float32 and g.is_contiguous() and g.shape == m.shape):
                raise ValueError("grad_maps: expected contiguous float32 tensors on %s of the prediction maps' shapes" % (self.device,))
        if len(grad_maps) != len(maps):
            raise ValueError("expected %d gradient maps, got %d" % (len(maps), len(grad_maps)))
        return list(grad_maps)

    def forward_backward(self, pred_maps, target=None, upstream=None, with_grad=True, grad_maps=None):
        """pred_maps: one fp32 map [B, A(5+C), hs, ws] per level (torch on this device, or numpy).  target: dense [B, N, 11] or
        None = the targets of the last set_labels.  upstream: the gradients arriving at conf_loss, cls_loss, txtytwth_loss
        and total_loss (four values, torch or numpy) or None = (0, 0, 0, 1).  Returns (float64 [4], float64 [B, 5], [one
        gradient map per level, torch on this device]); with_grad=False: the value only and an empty list.  grad_maps: tensors
        to fill instead of fresh ones (every element is written, whatever they held)."""
        maps, B = self._maps(pred_maps)
        tgt, up = self._target(target, B), _upstream(upstream, self.device)
        grads = self._grads(maps, grad_maps) if with_grad else []
        out = (C.c_double * 4)()
        parts = np.empty((B, 5), np.float64)
        check(self._lib.y355_grad_forward_backward(self._h, self._ptrs(maps), None if tgt is None else tgt.data_ptr(), B,
                                                   None if up is None else up.data_ptr(), self._ptrs(grads) if with_grad else None,
                                                   _stream(self.device), out, parts.ctypes.data_as(P(C.c_double))))
        return np.array(list(out), np.float64), parts, grads

    def backward(self, pred_maps, target=None, upstream=None, grad_maps=None):
        """the gradient maps alone, asynchronous on the current stream: the bits forward_backward gives"""
        maps, B = self._maps(pred_maps)
        tgt, up = self._target(target, B), _upstream(upstream, self.device)
        grads = self._grads(maps, grad_maps)
        check(self._lib.y355_grad_backward(self._h, self._ptrs(maps), None if tgt is None else tgt.data_ptr(), B,
                                           None if up is None else up.data_ptr(), self._ptrs(grads), _stream(self.device)))
        return grads


def _loss_tensors(out, device):
    """the reference's return: four 0-dim float32 tensors"""
    return tuple(torch.tensor(float(v), dtype=torch.float32, device=device) for v in out)


class _MapLoss(torch.autograd.Function):
    """forward: the value (one pass over the maps, nothing saved but the inputs); backward: y355_grad_backward with the four
    arriving gradients as a device tensor -- no host synchronisation"""

    @staticmethod
    def forward(ctx, handle, target, *pred_maps):
        out, _, _ = handle.forward_backward(pred_maps, target=target, with_grad=False)
        ctx.handle, ctx.target = handle, target
        ctx.save_for_backward(*pred_maps)
        return _loss_tensors(out, handle.device)

    @staticmethod
    def backward(ctx, *g):
        h = ctx.handle
        up = torch.stack([v.to(device=h.device, dtype=torch.float32).reshape(()) for v in g])
        grads = h.backward(ctx.saved_tensors, target=ctx.target, upstream=up)
        return (None, None) + tuple(gr.to(p.dtype) for gr, p in zip(grads, ctx.saved_tensors))


class YoloCriterion(torch.nn.Module):
    """The reference's loss branch as a torch module with a graph: criterion(pred_maps, label_lists=None, target=None) ->
    (conf_loss, cls_loss, txtytwth_loss, total_loss), 0-dim float32 tensors whose backward() reaches the prediction maps.
    label_lists: per image [[xmin, ymin, xmax, ymax, cls], ...], assigned on the device (set_labels); or target: a dense
    [B, N, 11] tensor; or neither: the labels of the last call.  The handle's own target tensor serves the backward pass, so
    call backward() before the next batch's labels are set.  Constructor arguments: YoloLossGrad's."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.handle = YoloLossGrad(*args, **kwargs)

    def forward(self, pred_maps, label_lists=None, target=None):
        if label_lists is not None and target is not None:
            raise ValueError("give label_lists or target, not both")
        if isinstance(pred_maps, torch.Tensor):
            pred_maps = [pred_maps]
        if label_lists is not None:
            self.handle.set_labels(label_lists)
        return _MapLoss.apply(self.handle, target, *pred_maps)

    def close(self):
        self.handle.close()


def _cuda_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: expected a CUDA tensor (yolo355 has no CPU path)" % name)
    return t.detach().to(torch.float32).contiguous()


def _flat_args(pred_conf, pred_cls, pred_txtytwth, label, num_classes):
    conf, cls = _cuda_f32(pred_conf, "pred_conf"), _cuda_f32(pred_cls, "pred_cls")
    box, lab = _cuda_f32(pred_txtytwth, "pred_txtytwth"), _cuda_f32(label, "label")
    B, N = int(cls.shape[0]), int(cls.shape[1])
    if tuple(cls.shape) != (B, N, num_classes) or conf.numel() != B * N or tuple(box.shape) != (B, N, 4) or tuple(lab.shape) != (B, N, 8):
        raise ValueError("expected pred_conf [B,N,1], pred_cls [B,N,%d], pred_txtytwth [B,N,4] and label [B,N,8]" % num_classes)
    return conf, cls, box, lab, B, N


def flat_forward_backward(pred_conf, pred_cls, pred_txtytwth, label, num_classes, upstream=None, obj_weight=5.0, noobj_weight=1.0):
    """y355_grad_flat in one call: (float64 [4], float64 [B, 5], (g_conf, g_cls, g_txtytwth) of the inputs' shapes)"""
    conf, cls, box, lab, B, N = _flat_args(pred_conf, pred_cls, pred_txtytwth, label, num_classes)
    up = _upstream(upstream, cls.device)
    g = (torch.empty_like(conf), torch.empty_like(cls), torch.empty_like(box))
    out = (C.c_double * 4)()
    parts = np.empty((B, 5), np.float64)
    check(lib().y355_grad_flat(cls.device.index, conf.data_ptr(), cls.data_ptr(), box.data_ptr(), lab.data_ptr(), B, N, int(num_classes),
                               float(obj_weight), float(noobj_weight), None if up is None else up.data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                               g[2].data_ptr(), _stream(cls.device), out, parts.ctypes.data_as(P(C.c_double))))
    return np.array(list(out), np.float64), parts, g


class _FlatLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred_conf, pred_cls, pred_txtytwth, label, num_classes):
        conf, cls, box, lab, B, N = _flat_args(pred_conf, pred_cls, pred_txtytwth, label, num_classes)
        out = (C.c_double * 4)()
        check(lib().y355_grad_flat(cls.device.index, conf.data_ptr(), cls.data_ptr(), box.data_ptr(), lab.data_ptr(), B, N, int(num_classes),
                                   5.0, 1.0, None, None, None, None, _stream(cls.device), out, None))
        ctx.save_for_backward(pred_conf, pred_cls, pred_txtytwth, label)
        ctx.num_classes = int(num_classes)
        return _loss_tensors(out, cls.device)

    @staticmethod
    def backward(ctx, *g):
        pred_conf, pred_cls, pred_txtytwth, label = ctx.saved_tensors
        conf, cls, box, lab, B, N = _flat_args(pred_conf, pred_cls, pred_txtytwth, label, ctx.num_classes)
        up = torch.stack([v.to(device=cls.device, dtype=torch.float32).reshape(()) for v in g])
        gr = (torch.empty_like(conf), torch.empty_like(cls), torch.empty_like(box))
        check(lib().y355_grad_flat(cls.device.index, conf.data_ptr(), cls.data_ptr(), box.data_ptr(), lab.data_ptr(), B, N, ctx.num_classes,
                                   5.0, 1.0, up.data_ptr(), gr[0].data_ptr(), gr[1].data_ptr(), gr[2].data_ptr(), _stream(cls.device), None,
                                   None))
        return (gr[0].reshape(pred_conf.shape).to(pred_conf.dtype), gr[1].to(pred_cls.dtype), gr[2].to(pred_txtytwth.dtype), None, None)


def loss(pred_conf, pred_cls, pred_txtytwth, label, num_classes, obj_loss_f="mse"):
    """tools.loss (tools.py:392-435) on CUDA tensors: pred_conf [B,N,1], pred_cls [B,N,C], pred_txtytwth [B,N,4], label
    [B,N,8] = iou, obj, cls, tx, ty, tw, th, weight.  Returns (conf_loss, cls_loss, txtytwth_loss, total_loss) as 0-dim
    float32 tensors on the inputs' device, each with a grad_fn that reaches the three predictions (the label is a constant)."""
    if obj_loss_f != "mse":
        raise NotImplementedError("obj_loss_f=%r: only 'mse' is built (no model of the reference uses 'bce')" % (obj_loss_f,))
    return _FlatLoss.apply(pred_conf, pred_cls, pred_txtytwth, label, num_classes)
