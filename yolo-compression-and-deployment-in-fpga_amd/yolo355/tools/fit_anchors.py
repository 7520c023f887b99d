"""Fit anchor boxes to a data set on the GPU (yolo355.anchors), the counterpart of the reference's generate_ab_kmeans.py with
its arguments -d / -na / -size, without its hard-coded data set roots:

    python -m yolo355.tools.fit_anchors -d voc  --annopath 'VOC2007/Annotations/%s.xml' --ids VOC2007/ImageSets/Main/trainval.txt -na 5
    python -m yolo355.tools.fit_anchors -d coco --annotations annotations/instances_train2017.json -na 9 --restarts 16

--annopath / --ids may be repeated in pairs (VOC2007 and VOC2012).  Restart 0 of --seed S is the reference's run after
np.random.seed(S); the best of --restarts restarts is printed in both conventions of data/config.py: grid units of --stride
(ANCHOR_SIZE, the one-level models) and pixels sorted by area, grouped per level when -na splits into --levels
(MULTI_ANCHOR_SIZE, as yolo355.loss takes them), with the mean IoU and the boxes per anchor."""
import argparse
import json

import numpy as np


def load_boxes(a):
    from yolo355 import anchors as A
    if a.dataset == "voc":
        if not a.annopath or len(a.annopath) != len(a.ids or []):
            raise SystemExit("-d voc needs --annopath PATTERN --ids FILE (in pairs)")
        parts = []
        for pattern, ids in zip(a.annopath, a.ids):
            with open(ids) as f:
                names = [line.split()[0] for line in f if line.strip()]
            parts.append(A.voc_boxes(pattern, names, a.input_size))
        return np.concatenate(parts)
    if not a.annotations:
        raise SystemExit("-d coco needs --annotations FILE")
    return A.coco_boxes(a.annotations, a.input_size)


def fmt(anchors, digits=2):
    return "[" + ", ".join("[%.*f, %.*f]" % (digits, w, digits, h) for w, h in np.asarray(anchors).reshape(-1, 2)) + "]"


def main(argv=None):
    ap = argparse.ArgumentParser(description="k-means (1 - IoU) anchor boxes on the GPU")
    ap.add_argument("-d", "--dataset", default="coco", choices=["coco", "voc"])
    ap.add_argument("-na", "--num_anchorbox", default=9, type=int)
    ap.add_argument("-size", "--input_size", default=416, type=int)
    ap.add_argument("--restarts", default=8, type=int)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--iters", default=1000, type=int)
    ap.add_argument("--convergence", default=1e-6, type=float)
    ap.add_argument("--stride", default=32, type=int, help="grid units = pixels / stride")
    ap.add_argument("--levels", default=3, type=int, help="levels of the multi-level convention")
    ap.add_argument("--annopath", action="append", help="voc: pattern of an annotation file, %%s = image id")
    ap.add_argument("--ids", action="append", help="voc: file with one image id per line")
    ap.add_argument("--annotations", help="coco: the instances_*.json file")
    ap.add_argument("--json", action="store_true", help="print one JSON line instead of text")
    a = ap.parse_args(argv)
    from yolo355 import anchors as A
    boxes = load_boxes(a)
    if len(boxes) < 1:
        raise SystemExit("no boxes of at least one pixel at the input size")
    res = A.fit_anchors(boxes, a.num_anchorbox, seed=a.seed, restarts=a.restarts, iters=a.iters, convergence=a.convergence)
    by_area = A.sort_by_area(res.anchors)
    out = dict(boxes=len(boxes), k=a.num_anchorbox, input_size=a.input_size, restarts=a.restarts, seed=a.seed, best_restart=res.best,
               loss=res.loss, mean_loss=res.loss / len(boxes), iterations=res.iterations, mean_iou=res.mean_iou,
               losses=[r.loss for r in res.all], anchors_px=res.anchors.tolist(), counts=res.counts.tolist(),
               anchors_grid_units=A.to_grid_units(res.anchors, a.stride).tolist(), anchors_px_by_area=by_area.tolist())
    if a.json:
        print(json.dumps(out))
        return out
    print("boxes %d, k %d, input size %d: best of %d restarts is restart %d (%d steps), loss %.6f (%.6f per box), mean IoU %.4f"
          % (len(boxes), a.num_anchorbox, a.input_size, a.restarts, res.best, res.iterations, res.loss, res.loss / len(boxes), res.mean_iou))
    print("loss of every restart:", " ".join("%.4f" % r.loss for r in res.all))
    print("anchors (pixels, the reference's order):", fmt(res.anchors))
    print("boxes per anchor:", res.counts.tolist())
    print("grid units of stride %d (ANCHOR_SIZE):" % a.stride, fmt(A.to_grid_units(res.anchors, a.stride)))
    if a.num_anchorbox % a.levels == 0 and a.levels > 1:
        for l, lv in enumerate(A.split_levels(res.anchors, a.levels)):
            print("pixels by area, level %d (MULTI_ANCHOR_SIZE):" % l, fmt(lv))
    else:
        print("pixels by area:", fmt(by_area))
    return out


if __name__ == "__main__":
    main()
