#!/usr/bin/env python3
"""tests/golden/voc_ap.npz: the REFERENCE's own path from detections to AP -- write_voc_results_file + voc_eval (+ voc_ap) of
utils/vocapi_evaluator_mask.py:140-336 -- driven on a temporary devkit (the image-set file and annotations_cache/annots.pkl
holding the records, so no XML is parsed), on `object.__new__(VOCAPIEvaluator_mask)`.  Needs the reference (import recipe:
gen_golden.import_reference()); nothing of its source travels, only the seeded inputs and what it computed.

`write_voc_results_file` does not run on NumPy >= 2 (`if dets == []` on a non-empty array raises): the per-image arrays are
passed as a trivial ndarray subclass whose == with a list is False, empty entries as [] -- the reference itself is untouched.
Its rank order is np.argsort(-confidence), not stable: a case is only recorded after asserting, for every class file, that this
equals the stable order, the regime in which the reference's answer is defined.  With tied scores that is a property of the
input AND of NumPy's sort on the generating CPU (NumPy 2.2 with its SIMD sort reorders ties even among a dozen values), so the
tied case (c) walks seeds from 13 up to the first set on which the assertion holds for every class; the seed used is stored.

    python tests/golden/gen_golden_voc_ap.py        # rewrites tests/golden/voc_ap.npz
"""
import importlib
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402
import voc_ap_ref as R  # noqa: E402  (synth_set only: the inputs' generator)


class UndefinedOrder(AssertionError):
    pass


class _Dets(np.ndarray):
    def __eq__(self, other):
        if isinstance(other, list):
            return False
        return np.ndarray.__eq__(self, other)
    __hash__ = None


def distinct_scores(rng, cls, count, lo=1, hi=999):
    """scores whose 3-decimal roundings are distinct inside every class: k / 1000 plus less than half a thousandth"""
    scores = np.zeros(cls.shape, np.float32)
    live = np.arange(cls.shape[1])[None, :] < count[:, None]
    for c in np.unique(cls[live]):
        m = live & (cls == c)
        k = rng.permutation(np.arange(lo, hi + 1))[:m.sum()]
        assert len(k) == m.sum()
        scores[m] = (k / 1000.0 + rng.uniform(-0.0004, 0.0004, len(k))).astype(np.float32)
    return scores


def case_a(rng):
    gt, boxes, _, cls, count = R.synth_set(11, 12, 3, 8, 2.5, max_det=14)
    return 3, gt, boxes, distinct_scores(rng, cls, count), cls, count


def case_b(rng):
    gt, boxes, _, cls, count = R.synth_set(12, 120, 2, 10, 3, max_det=18, difficult=0.2)
    return 2, gt, boxes, distinct_scores(rng, cls, count), cls, count


def case_c(rng, seed=13):
    gt, boxes, scores, cls, count = R.synth_set(seed, 6, 3, 5, 2, max_det=8, score_decimals=1)
    for c in range(3):
        assert ((cls == c) & (np.arange(8)[None, :] < count[:, None])).sum() <= 16
    return 3, gt, boxes, scores, cls, count


def case_d(rng):
    """the edge set; detections are given as the file's coordinates minus one (the reference adds it back)"""
    gt = [
        # image 0: class 0 -- a box met at IoU exactly 0.5, a box matched twice, a difficult box matched first of all
        [(0, 0, 0, 10, 10, 0), (0, 100, 100, 140, 160, 0), (0, 200, 50, 260, 90, 1), (3, 300, 300, 340, 340, 0)],
        # image 1: a zero-area box of class 0 beside an ordinary one; class 2 has only difficult boxes
        [(0, 20, 20, 20, 20, 0), (0, 50, 50, 90, 90, 0), (2, 10, 200, 60, 260, 1)],
        [],                                                                    # image 2: no box at all
        [(2, 5, 5, 45, 65, 1), (3, 100, 20, 180, 90, 0)],                      # image 3
    ]
    dets = [
        [((-1, -1, 9, 4), 0.61, 0),            # inter 50, union 100: IoU exactly 0.5 -> FP
         ((99, 99, 139, 159), 0.93, 0),        # TP
         ((100, 101, 139, 158), 0.82, 0),      # the same box again -> FP
         ((199, 49, 259, 89), 0.99, 0),        # the difficult box, ranked first: neither (tp + fp = 0 at rank 0)
         ((10, 10, 60, 60), 0.47, 1)],         # class 1 has detections and no box anywhere
        [((19, 19, 19, 19), 0.77, 0),          # zero area on the zero-area box: 0 / 0 -> ovmax NaN -> FP
         ((49, 49, 89, 89), 0.71, 0),          # TP on the ordinary box
         ((9, 199, 59, 259), 0.66, 2),         # class 2: matches a difficult box
         ((300, 10, 350, 40), 0.31, 2)],       # class 2: FP
        [((30, 30, 80, 80), 0.52, 0),          # an image without boxes: FP
         ((40, 40, 70, 90), 0.25, 1)],
        [((4, 4, 44, 64), 0.58, 2)],
    ]
    md = 6
    n = len(gt)
    boxes, scores, cls = np.zeros((n, md, 4), np.float32), np.zeros((n, md), np.float32), np.zeros((n, md), np.int32)
    count = np.array([len(d) for d in dets], np.int32)
    for i, d in enumerate(dets):
        for k, (b, s, c) in enumerate(d):
            boxes[i, k], scores[i, k], cls[i, k] = b, s, c
    return 4, [np.asarray(g, np.float64).reshape(-1, 6) for g in gt], boxes, scores, cls, count


def run_reference(ev_mod, C, gt, boxes, scores, cls, count):
    """-> per class (rec, prec, ap07, ap_area) from the reference"""
    n = len(gt)
    names = ["%06d" % i for i in range(n)]
    labelmap = ["class%d" % c for c in range(C)]
    all_boxes = [[[] for _ in range(n)] for _ in range(C)]
    for i in range(n):
        for c in range(C):
            k = np.where(cls[i, :count[i]] == c)[0]
            if len(k):
                all_boxes[c][i] = np.hstack((boxes[i, k], scores[i, k][:, None])).astype(np.float32).view(_Dets)
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "annotations_cache"))
        with open(os.path.join(tmp, "test.txt"), "w") as f:
            f.write("".join(nm + "\n" for nm in names))
        recs = {nm: [dict(name=labelmap[int(r[0])], bbox=[int(v) for v in r[1:5]], difficult=int(r[5])) for r in g]
                for nm, g in zip(names, gt)}
        with open(os.path.join(tmp, "annotations_cache", "annots.pkl"), "wb") as f:
            pickle.dump(recs, f)
        ev = object.__new__(ev_mod.VOCAPIEvaluator_mask)
        ev.labelmap, ev.display, ev.set_type, ev.devkit_path = labelmap, False, "test", tmp
        ev.imgsetpath = os.path.join(tmp, "test.txt")
        ev.annopath = os.path.join(tmp, "%s.xml")
        ev.dataset = type("D", (), dict(ids=[(tmp, nm) for nm in names]))()
        ev.write_voc_results_file(all_boxes)
        for c, name in enumerate(labelmap):
            path = ev.get_voc_results_file_template(name)
            conf = np.array([float(line.split(" ")[1]) for line in open(path)])
            if not np.array_equal(np.argsort(-conf), np.argsort(-conf, kind="stable")):
                raise UndefinedOrder("the reference's rank order is undefined here: case not recorded")
            with np.errstate(invalid="ignore", divide="ignore"):
                rec, prec, ap07 = ev.voc_eval(path, name, os.path.join(tmp, "annotations_cache"), 0.5, True)
                rec2, prec2, apa = ev.voc_eval(path, name, os.path.join(tmp, "annotations_cache"), 0.5, False)
            assert np.array_equal(np.asarray(rec), np.asarray(rec2), equal_nan=True)
            assert np.array_equal(np.asarray(prec), np.asarray(prec2), equal_nan=True)
            res.append((np.atleast_1d(np.asarray(rec, np.float64)) if len(conf) else np.zeros(0),
                        np.atleast_1d(np.asarray(prec, np.float64)) if len(conf) else np.zeros(0), float(ap07), float(apa)))
    return res


def main():
    G.import_reference()
    ev_mod = importlib.import_module("utils.vocapi_evaluator_mask")
    rng = np.random.default_rng(2024)
    out = {}
    for name, make in (("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d)):
        if name == "c":
            for seed in range(13, 400):
                try:
                    C, gt, boxes, scores, cls, count = make(rng, seed)
                    if len(np.unique(scores[np.arange(scores.shape[1])[None, :] < count[:, None]])) > 9:
                        continue                          # want real tie groups
                    res = run_reference(ev_mod, C, gt, boxes, scores, cls, count)
                    break
                except AssertionError:
                    continue
            else:
                raise SystemExit("no tied set with a defined reference order found")
            out["c/seed"] = np.int32(seed)
        else:
            C, gt, boxes, scores, cls, count = make(rng)
            res = run_reference(ev_mod, C, gt, boxes, scores, cls, count)
        out[name + "/num_classes"] = np.int32(C)
        out[name + "/gt_off"] = np.cumsum([0] + [len(g) for g in gt]).astype(np.int32)
        out[name + "/gt"] = np.concatenate([np.asarray(g, np.float64).reshape(-1, 6) for g in gt]).astype(np.float32)
        out[name + "/boxes"], out[name + "/scores"], out[name + "/cls"], out[name + "/count"] = boxes, scores, cls, count
        for c, (rec, prec, ap07, apa) in enumerate(res):
            out["%s/rec/%d" % (name, c)], out["%s/prec/%d" % (name, c)] = rec, prec
        out[name + "/ap07"] = np.array([r[2] for r in res])
        out[name + "/ap_area"] = np.array([r[3] for r in res])
        print(name, "dets per class", [len(r[0]) for r in res], "ap07", out[name + "/ap07"], "area", out[name + "/ap_area"])
    path = os.path.join(HERE, "voc_ap.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
