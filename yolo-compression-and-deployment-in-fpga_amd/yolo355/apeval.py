"""VOC mAP on the GPU (y355_apeval, include/yolo355.h; csrc/apeval.hip): what the reference computes after its evaluator loop --
write_voc_results_file + voc_eval + voc_ap (utils/vocapi_evaluator_mask.py:140-336) -- from detections that stay on the device.

    ev = ApEval(20, ground_truth)                       # ground_truth[i] = rows (cls, xmin, ymin, xmax, ymax, difficult) of image i
    ev.add(first_image, boxes, scores, cls, count)      # the four CUDA tensors of Engine.forward_device / Pipeline.outputs
    aps, mean = ev.compute()                            # float64 [C], np.mean(aps)

The contract (text-file quantisation, rank order, matching, curve, both AP metrics) is DESIGN.md section 6c.  There is no host
fallback: without the library or a GPU the constructor raises."""
import ctypes as C

import numpy as np
import torch

from . import _ffi
from ._handle import Handle, _require_gpu


def _gt_arrays(ground_truth, num_classes):
    off = np.zeros(len(ground_truth) + 1, np.int32)
    rows = []
    for i, g in enumerate(ground_truth):
        g = np.asarray(g, np.float64).reshape(-1, 6)
        rows.append(g)
        off[i + 1] = off[i] + len(g)
    g = np.concatenate(rows) if rows else np.zeros((0, 6))
    cls = g[:, 0].astype(np.int32)
    if len(cls) and (cls.min() < 0 or cls.max() >= num_classes or np.any(cls != g[:, 0])):
        raise ValueError("ground-truth class outside 0 .. %d" % (num_classes - 1))
    return off, np.ascontiguousarray(g[:, 1:5], np.float32), cls, np.ascontiguousarray(g[:, 5] != 0, np.uint8)


class ApEval(Handle):
    _destroy = "y355_apeval_destroy"

    def __init__(self, num_classes, ground_truth, max_dets=None, device=0):
        lib = _ffi.lib()
        self.device = _require_gpu(device if isinstance(device, (str, torch.device)) else "cuda:%d" % int(device))
        self.num_classes, self.num_images = int(num_classes), len(ground_truth)
        # default capacity: 256 detections per image (VOC07 at conf_thresh 0.01 stays well below), at least 65536
        self.max_dets = int(max_dets) if max_dets is not None else min(1 << 27, max(1 << 16, 256 * self.num_images))
        off, boxes, cls, diff = _gt_arrays(ground_truth, self.num_classes)
        h = C.c_void_p()
        _ffi.check(lib.y355_apeval_create(self.device.index, self.num_classes, self.num_images, self.max_dets, C.byref(h)))
        self._own(lib, h)
        _ffi.check(lib.y355_apeval_set_gt(h, off.ctypes.data, boxes.ctypes.data, cls.ctypes.data, diff.ctypes.data))
        self.npos = self.ndet = self.mean_abi = None

    def add(self, first_image, boxes, scores, cls, count, after_stream=None, batch=None):
        """One batch of engine outputs, CUDA tensors: boxes float32 [B,max_det,4], scores float32 [B,max_det], cls int32
        [B,max_det], count int32 [B]; images first_image .. first_image + B - 1 (batch: only the first that many rows, for
        buffers sized for a larger batch).  Asynchronous.  after_stream: the torch stream (or raw handle) the tensors are produced
        on -- the append runs on it, behind its work; None: torch's current stream."""
        B = int(count.shape[0]) if batch is None else int(batch)
        md = int(scores.shape[1])
        for t, dt in ((boxes, torch.float32), (scores, torch.float32), (cls, torch.int32), (count, torch.int32)):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("ApEval.add takes contiguous CUDA tensors: float32 boxes / scores, int32 cls / count")
        if tuple(boxes.shape[1:]) != (md, 4) or tuple(cls.shape[1:]) != (md,) or min(boxes.shape[0], scores.shape[0], cls.shape[0], count.shape[0]) < B:
            raise ValueError("ApEval.add: shapes [B,max_det,4], [B,max_det], [B,max_det], [B] expected")
        if after_stream is None:
            after_stream = torch.cuda.current_stream(self.device)
        s = after_stream.cuda_stream if hasattr(after_stream, "cuda_stream") else int(after_stream)
        if s == 0:              # torch's default stream is HIP's null stream, handle 0 -- which the C ABI reads as "no producer"
            s = _ffi.AP_NULL_STREAM
        _ffi.check(self._lib.y355_apeval_add(self._h, int(first_image), B, md, boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(),
                                             count.data_ptr(), C.c_void_p(s)))

    def add_host(self, first_image, boxes, scores, cls, count):
        """the same from NumPy arrays (y355_apeval_add_host); synchronous"""
        scores = np.ascontiguousarray(scores, np.float32)
        B, md = scores.shape
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(B, md, 4)
        cls = np.ascontiguousarray(cls, np.int32).reshape(B, md)
        count = np.ascontiguousarray(count, np.int32).reshape(B)
        _ffi.check(self._lib.y355_apeval_add_host(self._h, int(first_image), B, md, boxes.ctypes.data, scores.ctypes.data, cls.ctypes.data,
                                                  count.ctypes.data))

    def add_detections(self, first_image, dets):
        """the [(bboxes [n,4], scores [n], cls_inds [n]), ...] list every forward_batch returns, one entry per image"""
        md = max([1] + [len(s) for _, s, _ in dets])
        B = len(dets)
        boxes, scores, cls = np.zeros((B, md, 4), np.float32), np.zeros((B, md), np.float32), np.zeros((B, md), np.int32)
        count = np.zeros(B, np.int32)
        for i, (b, s, c) in enumerate(dets):
            n = len(s)
            count[i] = n
            if n:
                boxes[i, :n], scores[i, :n], cls[i, :n] = np.asarray(b, np.float32).reshape(n, 4), s, c
        self.add_host(first_image, boxes, scores, cls, count)

    def reset(self):
        """drop the detections, keep the ground truth"""
        _ffi.check(self._lib.y355_apeval_reset(self._h))

    def compute(self, ovthresh=0.5, use_07_metric=True, quantize=True):
        """-> (aps float64 [C], np.mean(aps)); self.npos / self.ndet hold the per-class box and detection counts.  A class
        without detections has ap -1 and is part of the mean, as in the reference.  Raises Y355Error (ERANGE) when more than
        max_dets detections were added or a class index was out of range; reset() makes the handle usable again."""
        Cn = self.num_classes
        ap, npos, ndet, mean = np.zeros(Cn, np.float64), np.zeros(Cn, np.int32), np.zeros(Cn, np.int64), C.c_double()
        _ffi.check(self._lib.y355_apeval_compute(self._h, float(ovthresh), _ffi.AP_VOC07 if use_07_metric else _ffi.AP_AREA,
                                                 _ffi.AP_Q_VOCFILE if quantize else _ffi.AP_Q_NONE, ap.ctypes.data, npos.ctypes.data,
                                                 ndet.ctypes.data, C.byref(mean)))
        self.npos, self.ndet = npos, ndet
        self.mean_abi = mean.value                        # the C ABI's mean: the sum in class order / C (np.mean sums pairwise)
        return ap, float(np.mean(ap))

    def curve(self, cls):
        """(rec, prec, flag) of class cls of the last compute, in rank order; flag 1 TP, 2 FP, 0 neither (a difficult match)"""
        n = C.c_int64()
        _ffi.check(self._lib.y355_apeval_curve(self._h, int(cls), 0, None, None, None, C.byref(n)))
        rec, prec, flag = np.zeros(n.value), np.zeros(n.value), np.zeros(n.value, np.uint8)
        if n.value:
            _ffi.check(self._lib.y355_apeval_curve(self._h, int(cls), n.value, rec.ctypes.data, prec.ctypes.data, flag.ctypes.data, C.byref(n)))
        return rec, prec, flag
