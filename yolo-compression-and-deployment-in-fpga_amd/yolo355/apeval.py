"""VOC mAP and COCO AP on the GPU (y355_apeval, include/yolo355.h; csrc/apeval.hip, csrc/cocoeval.hip): what the reference computes
after its evaluator loops -- write_voc_results_file + voc_eval + voc_ap (utils/vocapi_evaluator_mask.py:140-336), and pycocotools'
COCOeval evaluate / accumulate / summarize (utils/cocoapi_evaluator.py:100-124) -- from detections that stay on the device.

    ev = ApEval(20, ground_truth)                       # ground_truth[i] = rows (cls, xmin, ymin, xmax, ymax, difficult) of image i
    ev.add(first_image, boxes, scores, cls, count)      # the four CUDA tensors of Engine.forward_device / Pipeline.outputs
    aps, mean = ev.compute()                            # float64 [C], np.mean(aps)

    ev = CocoEval(80, ground_truth, image_ids)          # ground_truth[i] = rows (cls, x, y, w, h, area, iscrowd) of image i
    ev.add(first_image, boxes, scores, cls, count)      # the same store (ApStore)
    stats = ev.compute()                                # float64 [12], what COCOeval.summarize() prints; ev.precision, ev.recall

The contracts (VOC: text-file quantisation, rank order, matching, curve, both AP metrics; COCO: groups, IoU, greedy matching per
area range and threshold, accumulation, the twelve numbers) are DESIGN.md section 6c.  There is no host
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


class ApStore(Handle):
    """The y355_apeval handle and its device store of detection records: what ApEval (VOC) and CocoEval share."""
    _destroy = "y355_apeval_destroy"

    def _create_store(self, num_classes, num_images, max_dets, device):
        lib = _ffi.lib()
        self.device = _require_gpu(device if isinstance(device, (str, torch.device)) else "cuda:%d" % int(device))
        self.num_classes, self.num_images = int(num_classes), int(num_images)
        # default capacity: 256 detections per image (VOC07 at conf_thresh 0.01 stays well below), at least 65536
        self.max_dets = int(max_dets) if max_dets is not None else min(1 << 27, max(1 << 16, 256 * self.num_images))
        h = C.c_void_p()
        _ffi.check(lib.y355_apeval_create(self.device.index, self.num_classes, self.num_images, self.max_dets, C.byref(h)))
        self._own(lib, h)
        return lib, h

    def add(self, first_image, boxes, scores, cls, count, after_stream=None, batch=None):
        """One batch of engine outputs, CUDA tensors: boxes float32 [B,max_det,4], scores float32 [B,max_det], cls int32
        [B,max_det], count int32 [B]; images first_image .. first_image + B - 1 (batch: only the first that many rows, for
        buffers sized for a larger batch).  Asynchronous.  after_stream: the torch stream (or raw handle) the tensors are produced
        on -- the append runs on it, behind its work; None: torch's current stream."""
        B = int(count.shape[0]) if batch is None else int(batch)
        md = int(scores.shape[1])
        for t, dt in ((boxes, torch.float32), (scores, torch.float32), (cls, torch.int32), (count, torch.int32)):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
                raise ValueError("%s.add takes contiguous CUDA tensors: float32 boxes / scores, int32 cls / count" % type(self).__name__)
        if tuple(boxes.shape[1:]) != (md, 4) or tuple(cls.shape[1:]) != (md,) or min(boxes.shape[0], scores.shape[0], cls.shape[0], count.shape[0]) < B:
            raise ValueError("%s.add: shapes [B,max_det,4], [B,max_det], [B,max_det], [B] expected" % type(self).__name__)
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


class ApEval(ApStore):
    def __init__(self, num_classes, ground_truth, max_dets=None, device=0):
        off, boxes, cls, diff = _gt_arrays(ground_truth, int(num_classes))
        lib, h = self._create_store(num_classes, len(ground_truth), max_dets, device)
        _ffi.check(lib.y355_apeval_set_gt(h, off.ctypes.data, boxes.ctypes.data, cls.ctypes.data, diff.ctypes.data))
        self.npos = self.ndet = self.mean_abi = None

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


# ---------------------------------------------------------------------------------------------------- COCO
# COCOeval's Params for iouType 'bbox'
COCO_IOU_THRS = np.linspace(.5, .95, 10)
COCO_REC_THRS = np.linspace(0, 1, 101)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNG = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))


def image_ranks(image_ids, num_images=None):
    """rank[i] = the place of image i when the images are taken in ascending id (COCOeval.evaluate: np.unique(imgIds)); None: the
    list order.  Duplicate ids are rejected."""
    if image_ids is None:
        return np.arange(int(num_images), dtype=np.int32)
    ids = np.asarray(image_ids)
    if ids.ndim != 1 or (num_images is not None and len(ids) != num_images):
        raise ValueError("image_ids: one id per image expected")
    order = np.argsort(ids, kind="stable")
    if len(ids) > 1 and np.any(ids[order][1:] == ids[order][:-1]):
        raise ValueError("duplicate image ids")
    rank = np.empty(len(ids), np.int32)
    rank[order] = np.arange(len(ids), dtype=np.int32)
    return rank


def coco_gt_arrays(ground_truth, num_classes):
    """rows (cls, x, y, w, h, area, iscrowd) per image -> (offsets i32, boxes f64 [n,4], area f64 [n], cls i32 [n], iscrowd u8 [n])"""
    off = np.zeros(len(ground_truth) + 1, np.int32)
    rows = []
    for i, g in enumerate(ground_truth):
        g = np.asarray(g, np.float64).reshape(-1, 7)
        rows.append(g)
        off[i + 1] = off[i] + len(g)
    g = np.concatenate(rows) if rows else np.zeros((0, 7))
    cls = g[:, 0].astype(np.int32)
    if len(cls) and (cls.min() < 0 or cls.max() >= num_classes or np.any(cls != g[:, 0])):
        raise ValueError("ground-truth class outside 0 .. %d" % (num_classes - 1))
    return off, np.ascontiguousarray(g[:, 1:5]), np.ascontiguousarray(g[:, 5]), cls, np.ascontiguousarray(g[:, 6] != 0, np.uint8)


def coco_summarize(precision, recall):
    """COCOeval.summarize() for the default parameters: the twelve stats from precision [10,101,K,4,3] and recall [10,K,4,3]"""
    def mean(s):
        s = s[s > -1]
        return -1.0 if len(s) == 0 else float(np.mean(s))
    M = precision.shape[4] - 1
    return np.array([mean(precision[:, :, :, 0, M]), mean(precision[0:1, :, :, 0, M]), mean(precision[5:6, :, :, 0, M])] +
                    [mean(precision[:, :, :, a, M]) for a in (1, 2, 3)] + [mean(recall[:, :, 0, m]) for m in (0, 1, 2)] +
                    [mean(recall[:, :, a, M]) for a in (1, 2, 3)], np.float64)


class CocoEval(ApStore):
    def __init__(self, num_classes, ground_truth, image_ids=None, max_dets=None, device=0):
        """ground_truth[i]: float64 rows (cls, x, y, w, h, area, iscrowd) of image i; image_ids: the images' COCO ids (they fix the
        order images are accumulated in; None: the list order)"""
        self._gt = coco_gt_arrays(ground_truth, int(num_classes))
        rank = image_ranks(image_ids, len(ground_truth))
        self._create_store(num_classes, len(ground_truth), max_dets, device)
        self._set_gt(rank)
        self.precision = self.recall = self.stats = self.stats_abi = None

    def _set_gt(self, rank):
        off, boxes, area, cls, crowd = self._gt
        _ffi.check(self._lib.y355_apeval_set_gt_coco(self._h, off.ctypes.data, boxes.ctypes.data, area.ctypes.data, cls.ctypes.data,
                                                     crowd.ctypes.data, rank.ctypes.data))

    def set_image_ids(self, image_ids):
        """the images' ids, for a caller that learns them while it adds (an evaluator's loop): only compute() reads the order, the
        detections already added stay"""
        self._set_gt(image_ranks(image_ids, self.num_images))

    def compute(self, iou_thrs=None, rec_thrs=None, area_rng=None, max_dets=None):
        """-> stats float64 [12] (what COCOeval.summarize() prints: np.mean over the device-produced arrays); self.precision
        [T,R,K,A,M], self.recall [T,K,A,M] as COCOeval.eval holds them, self.stats_abi the C ABI's own twelve (in-order sums).
        With other than the default parameter shape the stats are None.  Y355Error as ApEval.compute."""
        iou = np.ascontiguousarray(COCO_IOU_THRS if iou_thrs is None else iou_thrs, np.float64)
        rec = np.ascontiguousarray(COCO_REC_THRS if rec_thrs is None else rec_thrs, np.float64)
        rng = np.ascontiguousarray(COCO_AREA_RNG if area_rng is None else area_rng, np.float64).reshape(-1, 2)
        md = np.ascontiguousarray(COCO_MAX_DETS if max_dets is None else max_dets, np.int32)
        T, R, A, M, K = len(iou), len(rec), len(rng), len(md), self.num_classes
        default = (T, R, A, M) == (10, 101, 4, 3)
        precision, recall, stats = np.zeros((T, R, K, A, M)), np.zeros((T, K, A, M)), np.zeros(12)
        _ffi.check(self._lib.y355_apeval_compute_coco(self._h, iou.ctypes.data, T, rec.ctypes.data, R, rng.ctypes.data, A, md.ctypes.data, M,
                                                      precision.ctypes.data, recall.ctypes.data, stats.ctypes.data if default else None))
        self.precision, self.recall = precision, recall
        self.stats_abi = stats if default else None
        self.stats = coco_summarize(precision, recall) if default else None
        self._T = T
        return self.stats

    def matches(self, image, cls, area):
        """the parity tap of the last compute for the group (image index, cls) under area range `area`: dict(pos [D] positions in
        the image's list in score order, dtm [T,D] matched box (index among the group's boxes in annotation order) or -1,
        dt_ig [T,D], gt_marked [T,G])"""
        nd, ng = C.c_int64(), C.c_int64()
        _ffi.check(self._lib.y355_apeval_coco_matches(self._h, int(image), int(cls), int(area), 0, 0, C.byref(nd), C.byref(ng), None, None, None, None))
        D, G, T = nd.value, ng.value, self._T
        pos, dtm = np.zeros(D, np.int32), np.zeros((T, D), np.int32)
        ig, marked = np.zeros((T, D), np.uint8), np.zeros((T, G), np.uint8)
        if D or G:
            _ffi.check(self._lib.y355_apeval_coco_matches(self._h, int(image), int(cls), int(area), D, G, C.byref(nd), C.byref(ng),
                                                          pos.ctypes.data, dtm.ctypes.data, ig.ctypes.data, marked.ctypes.data))
        return dict(pos=pos, dtm=dtm, dt_ig=ig, gt_marked=marked)
