"""Anchor boxes fitted to a data set on the GPU: ctypes binding of include/yolo355_anchors.h (csrc/anchors.hip, the companion
library libyolo355_anchors.so, loaded the first time a fit is asked for), the handle AnchorFit, fit_anchors() with the
reference's random draws (generate_ab_kmeans.py: `np.random.seed(s)` there is `seed=s` here), and the host-side helpers that
turn annotations into boxes and the fitted anchors into the two conventions of data/config.py.  No CPU path for the fit: without
a GPU it raises."""
import ctypes as C
import os
import random

import numpy as np

from . import _ffi
from ._handle import Handle, _require_gpu

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libyolo355_anchors.so")
HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include", "yolo355_anchors.h"))
MAX_K, MAX_RESTARTS, CHUNK = 16, 64, 1024

P = C.POINTER
_SIGS = {
    "y355_anchors_last_error": (C.c_char_p, []),
    "y355_anchors_chunk": (C.c_int, []),
    "y355_anchors_create": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, P(C.c_void_p)]),
    "y355_anchors_destroy": (None, [C.c_void_p]),
    "y355_anchors_set_boxes": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int64]),
    "y355_anchors_set_boxes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "y355_anchors_num_boxes": (C.c_int64, [C.c_void_p]),
    "y355_anchors_fit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, P(C.c_int32), P(C.c_double), P(C.c_int32),
                                   C.c_void_p]),
    "y355_anchors_get_result": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_int32), P(C.c_int32), P(C.c_double), P(C.c_int32)]),
    "y355_anchors_assignments": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_int32)]),
    "y355_anchors_score": (C.c_int, [C.c_void_p, P(C.c_double), C.c_int32, P(C.c_double), P(C.c_int32), P(C.c_int32)]),
}
_lib = None
# libyolo355_anchors.so, built with libyolo355.so by `make -C csrc`
lib, check, declared_symbols = _ffi.loader(globals(), "y355_anchors_", "extensions first (make -C csrc)")


def _f64(a):
    return a.ctypes.data_as(P(C.c_double))


def _i32(a):
    return a.ctypes.data_as(P(C.c_int32))


def draws(n, k, seed, restarts=1):
    """The reference's random draws (init_centroids, generate_ab_kmeans.py:57,76): per restart r, from
    numpy.random.RandomState(seed + r), choice(n, 1) and then random_sample() k - 1 times.  -> (first int32 [R], u float64
    [R, k - 1])"""
    first, u = np.zeros(restarts, np.int32), np.zeros((restarts, max(k - 1, 0)), np.float64)
    for r in range(restarts):
        rs = np.random.RandomState(seed + r)
        first[r] = int(rs.choice(n, 1)[0])
        for j in range(k - 1):
            u[r, j] = rs.random_sample()
    return first, u


def sample_indices(n, k, seed, restarts=1):
    """plus=False of the reference (:133-136): random.sample(range(n), k) of random.Random(seed + r) -> int32 [R, k]"""
    return np.array([random.Random(seed + r).sample(range(n), k) for r in range(restarts)], np.int32).reshape(restarts, k)


class Restart:
    """One restart of a fit: anchors float64 [k, 2] in the reference's order, loss (a sum over the boxes), iterations (the
    number of do_kmeans steps), counts int32 [k], init float64 [k, 2]"""

    def __init__(self, anchors, loss, iterations, counts, init):
        self.anchors, self.loss, self.iterations, self.counts, self.init = anchors, float(loss), int(iterations), counts, init


class FitResult:
    """fit_anchors' return: the best restart's .anchors / .loss / .iterations / .counts / .init, .best (its index), .all (a
    Restart per restart), .mean_iou (the best restart's anchors scored on the boxes) and .groups (int32 [n], the best restart's
    groups of its last step)"""

    def __init__(self, all_, best, mean_iou, groups):
        self.all, self.best, self.mean_iou, self.groups = all_, int(best), float(mean_iou), groups
        b = all_[best]
        self.anchors, self.loss, self.iterations, self.counts, self.init = b.anchors, b.loss, b.iterations, b.counts, b.init


class AnchorFit(Handle):
    """y355_anchors: the boxes of a data set on the device and fits / scores on them."""
    _destroy = "y355_anchors_destroy"

    def __init__(self, max_boxes, max_restarts=1, max_k=MAX_K, device=None):
        l = lib()
        self.device = _require_gpu(device)
        self.max_boxes, self.max_restarts, self.max_k = int(max_boxes), int(max_restarts), int(max_k)
        self.n = self._k = self._r = 0
        hd = C.c_void_p()
        check(l.y355_anchors_create(self.device.index, self.max_boxes, self.max_restarts, self.max_k, C.byref(hd)))
        self._own(l, hd)

    def _cur_stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def set_boxes(self, boxes):
        """boxes [n, 2] = (w, h): a numpy array / list (host form) or a float64 CUDA tensor on this device (device form)"""
        import torch
        self.n = self._k = self._r = 0
        if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
            if boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 2 or boxes.device != self.device:
                raise ValueError("expected a float64 [n,2] tensor on %s" % (self.device,))
            b = boxes.contiguous()
            check(self._lib.y355_anchors_set_boxes_dev(self._h, b.data_ptr(), b.shape[0], self._cur_stream()))
            self.n = int(b.shape[0])
            return
        b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 2))
        check(self._lib.y355_anchors_set_boxes(self._h, _f64(b), len(b)))
        self.n = len(b)

    def fit(self, k, first=None, u=None, init_index=None, iters=1000, convergence=1e-6):
        """One fit with len(first) (or len(init_index)) restarts; first [R] with u [R, k - 1], or init_index [R, k]"""
        k = int(k)
        if init_index is not None:
            idx = np.ascontiguousarray(np.asarray(init_index, np.int32).reshape(-1, k))
            R, args = len(idx), (None, None, _i32(idx))
        else:
            f = np.ascontiguousarray(np.asarray(first, np.int32).reshape(-1))
            R = len(f)
            uu = np.ascontiguousarray(np.asarray(u if u is not None else np.zeros((R, 0)), np.float64).reshape(R, max(k - 1, 0)))
            args = (_i32(f), _f64(uu) if k > 1 else None, None)
        self._k = self._r = 0
        check(self._lib.y355_anchors_fit(self._h, k, R, int(iters), float(convergence), *args, self._cur_stream()))
        self._k, self._r = k, R

    def result(self):
        """(list of Restart, best)"""
        R, k = self._r, self._k
        cen, ini = np.zeros((R, k, 2), np.float64), np.zeros((R, k, 2), np.float64)
        loss, its, cnt, best = np.zeros(R, np.float64), np.zeros(R, np.int32), np.zeros((R, k), np.int32), C.c_int32(0)
        check(self._lib.y355_anchors_get_result(self._h, _f64(cen), _f64(loss), _i32(its), _i32(cnt), _f64(ini), C.byref(best)))
        return [Restart(cen[r], loss[r], its[r], cnt[r], ini[r]) for r in range(R)], int(best.value)

    def assignments(self, restart=0):
        out = np.zeros(self.n, np.int32)
        check(self._lib.y355_anchors_assignments(self._h, int(restart), _i32(out)))
        return out

    def score(self, anchors, with_index=False):
        """anchors [k, 2] in the boxes' units -> (mean best IoU, counts int32 [k]) or, with_index, (.., .., best index int32 [n])"""
        a = np.ascontiguousarray(np.asarray(anchors, np.float64).reshape(-1, 2))
        mean, cnt = C.c_double(0.0), np.zeros(len(a), np.int32)
        idx = np.zeros(self.n, np.int32) if with_index else None
        check(self._lib.y355_anchors_score(self._h, _f64(a), len(a), C.byref(mean), _i32(cnt), None if idx is None else _i32(idx)))
        return (mean.value, cnt, idx) if with_index else (mean.value, cnt)


def fit_anchors(boxes, k, seed=0, restarts=1, iters=1000, convergence=1e-6, plus=True, device=None, init_index=None):
    """Fit k anchors to boxes [n, 2] = (w, h) with `restarts` random starts side by side and keep the best (lowest loss, the
    lowest restart among equals).  Restart r draws from RandomState(seed + r), so restart 0 is the reference's run after
    np.random.seed(seed).  plus=False: the initial centroids are the boxes init_index [restarts, k], or, without it, the
    reference's random.sample of random.Random(seed + r)."""
    n = int(boxes.shape[0]) if hasattr(boxes, "shape") else len(boxes)
    h = AnchorFit(max(n, 1), restarts, max(int(k), 1), device=device)
    try:
        h.set_boxes(boxes)
        if plus:
            first, u = draws(n, k, seed, restarts)
            h.fit(k, first=first, u=u, iters=iters, convergence=convergence)
        else:
            h.fit(k, init_index=init_index if init_index is not None else sample_indices(n, k, seed, restarts), iters=iters,
                  convergence=convergence)
        all_, best = h.result()
        mean_iou, _ = h.score(all_[best].anchors)
        return FitResult(all_, best, mean_iou, h.assignments(best))
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ boxes of a data set (host)
def boxes_from_annotations(rows_px, sizes_wh, input_size):
    """generate_ab_kmeans.py:198-206 in float64: rows_px [m, 4] = xmin, ymin, xmax, ymax in pixels of their image, sizes_wh
    [m, 2] = that image's (w, h); bw = (xmax - xmin) / w * size, bh = (ymax - ymin) / h * size; a box with bw < 1 or bh < 1 is
    dropped.  -> float64 [n, 2]"""
    rows = np.asarray(rows_px, np.float64).reshape(-1, 4)
    wh = np.asarray(sizes_wh, np.float64).reshape(-1, 2)
    size = float(input_size)
    bw = (rows[:, 2] - rows[:, 0]) / wh[:, 0] * size
    bh = (rows[:, 3] - rows[:, 1]) / wh[:, 1] * size
    keep = ~((bw < 1.0) | (bh < 1.0))
    return np.stack([bw[keep], bh[keep]], axis=1)


def voc_boxes(annopath, image_ids, input_size):
    """Boxes of VOC annotation files: annopath % image_id (or a callable) is an XML file with <size> and <object><bndbox>;
    coordinates as data/voc0712.py reads them (int(text) - 1)."""
    import xml.etree.ElementTree as ET
    rows, sizes = [], []
    for i in image_ids:
        root = ET.parse(annopath(i) if callable(annopath) else annopath % i).getroot()
        size = root.find("size")
        w, h = float(size.find("width").text), float(size.find("height").text)
        for obj in root.iter("object"):
            bb = obj.find("bndbox")
            rows.append([int(float(bb.find(t).text)) - 1 for t in ("xmin", "ymin", "xmax", "ymax")])
            sizes.append([w, h])
    return boxes_from_annotations(rows, sizes, input_size)


def coco_boxes(annotations, input_size):
    """Boxes of a COCO annotation file (a path or the loaded dict): images[].width / height and annotations[].bbox = x, y, w,
    h; as pull_anno of data/cocodataset.py:83-104: xmin = max(0, x), xmax = xmin + w (the same in y), kept when its area (the
    annotation's `area`, or w * h without one) is > 0 and xmax >= xmin, ymax >= ymin.  Annotations in file order."""
    if not isinstance(annotations, dict):
        import json
        with open(annotations) as f:
            annotations = json.load(f)
    size_of = {im["id"]: (float(im["width"]), float(im["height"])) for im in annotations["images"]}
    rows, sizes = [], []
    for a in annotations["annotations"]:
        if "bbox" not in a or a["image_id"] not in size_of:
            continue
        x, y, w, h = [float(v) for v in a["bbox"]]
        xmin, ymin = max(0.0, x), max(0.0, y)
        xmax, ymax = xmin + w, ymin + h
        if not (float(a.get("area", w * h)) > 0 and xmax >= xmin and ymax >= ymin):
            continue
        rows.append([xmin, ymin, xmax, ymax])
        sizes.append(size_of[a["image_id"]])
    return boxes_from_annotations(rows, sizes, input_size)


# ------------------------------------------------------------------------------------------------ the conventions of data/config.py
def to_grid_units(anchors, stride):
    """pixels at the input size -> grid units (ANCHOR_SIZE of the one-level models)"""
    return np.asarray(anchors, np.float64).reshape(-1, 2) / float(stride)


def sort_by_area(anchors):
    """ascending w * h (stable), as MULTI_ANCHOR_SIZE lists them"""
    a = np.asarray(anchors, np.float64).reshape(-1, 2)
    return a[np.argsort(a[:, 0] * a[:, 1], kind="stable")]


def split_levels(anchors, levels):
    """pixels, sorted by area and grouped per level, finest level first: float64 [levels, k / levels, 2]"""
    a = sort_by_area(anchors)
    if levels < 1 or len(a) % levels:
        raise ValueError("%d anchors do not split into %d levels" % (len(a), levels))
    return a.reshape(levels, len(a) // levels, 2)
