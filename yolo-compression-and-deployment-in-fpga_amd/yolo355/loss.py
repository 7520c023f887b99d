"""The reference's training targets and the forward value of its losses on the GPU: ctypes binding of
include/yolo355_loss.h (csrc/loss.hip, the companion library libyolo355_loss.so, loaded the first time a loss is asked
for), the handle YoloLoss, and drop-ins with the signatures of tools.gt_creator / multi_gt_creator / iou_score / loss
(tools.py:202-435).  No backward pass and no CPU path: without a GPU every entry point raises."""
import ctypes as C
import os

import numpy as np
import torch

from . import _ffi
from ._handle import Handle, _require_gpu

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_loss.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_loss.h"))
MAX_LEVELS, MAX_ANCHORS, TARGET_FIELDS = 3, 16, 11
IGNORE_THRESH = 0.5              # data/config.py:33


class LossConfig(C.Structure):
    """y355_loss_config"""
    _fields_ = [("device_id", C.c_int32), ("num_levels", C.c_int32),
                ("hs", C.c_int32 * MAX_LEVELS), ("ws", C.c_int32 * MAX_LEVELS), ("stride", C.c_int32 * MAX_LEVELS),
                ("num_anchors", C.c_int32), ("anchors", C.c_double * (2 * MAX_LEVELS * MAX_ANCHORS)),
                ("num_classes", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32), ("wh_mul", C.c_float),
                ("anchors_in_grid_units", C.c_int32), ("ignore_thresh", C.c_double),
                ("obj_weight", C.c_double), ("noobj_weight", C.c_double),
                ("max_batch", C.c_int32), ("max_labels_per_image", C.c_int32)]


P = C.POINTER
_SIGS = {
    "y355_loss_last_error": (C.c_char_p, []),
    "y355_loss_default_config": (C.c_int, [P(LossConfig)]),
    "y355_loss_create": (C.c_int, [P(LossConfig), P(C.c_void_p)]),
    "y355_loss_destroy": (None, [C.c_void_p]),
    "y355_loss_num_anchors_total": (C.c_int, [C.c_void_p]),
    "y355_loss_set_labels": (C.c_int, [C.c_void_p, P(C.c_int32), P(C.c_double), C.c_int32]),
    "y355_loss_get_targets": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "y355_loss_compute": (C.c_int, [C.c_void_p, P(C.c_void_p), C.c_void_p, C.c_int32, C.c_void_p, P(C.c_double), P(C.c_double)]),
    "y355_loss_iou_score": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "y355_loss_flat": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_double, C.c_double, C.c_void_p, P(C.c_double), P(C.c_double)]),
}
_lib = None
# libyolo355_loss.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_loss_", "extensions first (make -C csrc)")


def _as_list(strides):
    return [int(strides)] if np.isscalar(strides) else [int(s) for s in strides]


def pack_labels(label_lists):
    """ragged [[xmin, ymin, xmax, ymax, cls], ...] per image -> (offsets int32 [B+1], labels float64 [n,5])"""
    offsets = np.zeros(len(label_lists) + 1, np.int32)
    rows = []
    for b, labels in enumerate(label_lists):
        labels = np.asarray(labels, np.float64).reshape(-1, 5) if len(labels) else np.zeros((0, 5), np.float64)
        rows.append(labels)
        offsets[b + 1] = offsets[b] + len(labels)
    return offsets, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 5), np.float64))


class YoloLoss(Handle):
    """Targets and losses of one head geometry (y355_loss).  strides: one int (gt_creator: anchors in grid units, grid
    round(h / s) x round(w / s), decode multiplies the anchors by the stride) or a list (multi_gt_creator: anchors in
    pixels, level 0 first, grids h // s x w // s).  `multi` overrides that reading of `strides`."""
    _destroy = "y355_loss_destroy"

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
        cfg = LossConfig()
        check(l.y355_loss_default_config(C.byref(cfg)))
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
        check(l.y355_loss_create(C.byref(cfg), C.byref(hd)))
        self._own(l, hd)
        self.num_anchors_total = l.y355_loss_num_anchors_total(hd)
        self._batch = 0

    def set_labels(self, label_lists):
        """label_lists: per image a list of [xmin, ymin, xmax, ymax, cls] (coordinates in [0, 1]); builds the dense target
        tensor [B, N, 11] on the device, labels applied in list order"""
        offsets, labels = pack_labels(label_lists)
        check(self._lib.y355_loss_set_labels(self._h, offsets.ctypes.data_as(P(C.c_int32)), labels.ctypes.data_as(P(C.c_double)),
                                             len(label_lists)))
        self._batch = len(label_lists)

    def targets(self):
        """float32 [B, N, 11] of the last set_labels: obj, cls, tx, ty, tw, th, weight, x1, y1, x2, y2"""
        out = np.empty((self._batch, self.num_anchors_total, TARGET_FIELDS), np.float32)
        check(self._lib.y355_loss_get_targets(self._h, self._batch, out.ctypes.data))
        return out

    def compute(self, pred_maps, target=None):
        """pred_maps: one fp32 map [B, A(5+C), hs, ws] per level (torch on this device, or numpy).  target: dense [B, N, 11]
        (torch or numpy) or None = the targets of the last set_labels.  Returns (float64 [4] = conf_loss, cls_loss,
        txtytwth_loss, total_loss; float64 [B, 5] = pos, neg, cls, txty, twth per image)."""
        if isinstance(pred_maps, (np.ndarray, torch.Tensor)):
            pred_maps = [pred_maps]
        if len(pred_maps) != len(self.strides):
            raise ValueError("expected %d prediction maps, got %d" % (len(self.strides), len(pred_maps)))
        maps = [torch.as_tensor(p).to(device=self.device, dtype=torch.float32).contiguous() for p in pred_maps]
        B = int(maps[0].shape[0])
        ch = self.num_anchors * (5 + self.num_classes)
        for m, (hs, ws) in zip(maps, self.grids):
            if tuple(m.shape) != (B, ch, hs, ws):
                raise ValueError("expected a prediction map [%d,%d,%d,%d], got %s" % (B, ch, hs, ws, tuple(m.shape)))
        tgt = None
        if target is not None:
            tgt = torch.as_tensor(target).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(tgt.shape) != (B, self.num_anchors_total, TARGET_FIELDS):
                raise ValueError("expected a target [%d,%d,11], got %s" % (B, self.num_anchors_total, tuple(tgt.shape)))
        ptrs = (C.c_void_p * len(maps))(*[m.data_ptr() for m in maps])
        out = (C.c_double * 4)()
        parts = np.empty((B, 5), np.float64)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.y355_loss_compute(self._h, ptrs, None if tgt is None else tgt.data_ptr(), B, stream, out,
                                          parts.ctypes.data_as(P(C.c_double))))
        return np.array(list(out), np.float64), parts


def _creator(input_size, strides, label_lists, anchor_size, multi):
    assert len(input_size) > 0 and len(label_lists) > 0
    ncls = 1 + max([int(l[-1]) for labels in label_lists for l in labels] + [0])
    h = YoloLoss(input_size, strides, anchor_size, ncls, multi=multi, max_batch=len(label_lists),
                 max_labels_per_image=max(1, max(len(labels) for labels in label_lists)))
    try:
        h.set_labels(label_lists)
        return h.targets().astype(np.float64)
    finally:
        h.close()


def gt_creator(input_size, stride, label_lists, anchor_size):
    """tools.gt_creator (tools.py:202-253) on the GPU: ndarray [B, hs * ws * A, 11], the float32 values of the reference's
    float64 tensor (what its callers keep after `.float()`)"""
    return _creator(input_size, int(stride), label_lists, anchor_size, False)


def multi_gt_creator(input_size, strides, label_lists, anchor_size):
    """tools.multi_gt_creator (tools.py:256-374) on the GPU: ndarray [B, N, 11], level 0 first"""
    return _creator(input_size, list(strides), label_lists, anchor_size, True)


def _cuda_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: expected a CUDA tensor (yolo355 has no CPU path)" % name)
    return t.detach().to(torch.float32).contiguous()


def iou_score(bboxes_a, bboxes_b):
    """tools.iou_score (tools.py:377-389) on CUDA tensors [n, 4] -> [n]"""
    a, b = _cuda_f32(bboxes_a, "bboxes_a"), _cuda_f32(bboxes_b, "bboxes_b")
    if a.dim() != 2 or a.shape[1] != 4 or a.shape != b.shape or a.device != b.device:
        raise ValueError("expected two [n,4] tensors on one device, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    check(lib().y355_loss_iou_score(a.device.index, a.data_ptr(), b.data_ptr(), a.shape[0], out.data_ptr(),
                                    torch.cuda.current_stream(a.device).cuda_stream))
    return out


def loss_parts(pred_conf, pred_cls, pred_txtytwth, label, num_classes, obj_loss_f="mse"):
    """tools.loss with the per-image parts: (float64 [4], float64 [B, 5])"""
    if obj_loss_f != "mse":
        raise NotImplementedError("obj_loss_f=%r: only 'mse' is built (no model of the reference uses 'bce')" % (obj_loss_f,))
    conf, cls = _cuda_f32(pred_conf, "pred_conf"), _cuda_f32(pred_cls, "pred_cls")
    box, lab = _cuda_f32(pred_txtytwth, "pred_txtytwth"), _cuda_f32(label, "label")
    B, N = int(cls.shape[0]), int(cls.shape[1])
    if tuple(cls.shape) != (B, N, num_classes) or conf.numel() != B * N or tuple(box.shape) != (B, N, 4) or tuple(lab.shape) != (B, N, 8):
        raise ValueError("expected pred_conf [B,N,1], pred_cls [B,N,%d], pred_txtytwth [B,N,4] and label [B,N,8]" % num_classes)
    out = (C.c_double * 4)()
    parts = np.empty((B, 5), np.float64)
    check(lib().y355_loss_flat(cls.device.index, conf.data_ptr(), cls.data_ptr(), box.data_ptr(), lab.data_ptr(), B, N, int(num_classes),
                               5.0, 1.0, torch.cuda.current_stream(cls.device).cuda_stream, out, parts.ctypes.data_as(P(C.c_double))))
    return np.array(list(out), np.float64), parts


def loss(pred_conf, pred_cls, pred_txtytwth, label, num_classes, obj_loss_f="mse"):
    """tools.loss (tools.py:392-435) on CUDA tensors: pred_conf [B,N,1], pred_cls [B,N,C], pred_txtytwth [B,N,4], label
    [B,N,8] = iou, obj, cls, tx, ty, tw, th, weight.  Returns (conf_loss, cls_loss, txtytwth_loss, total_loss) as 0-dim
    float32 tensors on the inputs' device; the value only, no graph."""
    out, _ = loss_parts(pred_conf, pred_cls, pred_txtytwth, label, num_classes, obj_loss_f)
    return as_loss_tensors(out, pred_cls.device)


def as_loss_tensors(out, device):
    """the reference's return: four 0-dim float32 tensors"""
    return tuple(torch.tensor(float(v), dtype=torch.float32, device=device) for v in out)
