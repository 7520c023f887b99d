"""Times VOC mAP on the GPU (yolo355.apeval.ApEval) on a synthetic VOC07-sized set, and the NumPy restatement of the same contract
(tests/voc_ap_ref.py, the host yardstick) on the same data:

    python -m yolo355.tools.apeval_bench [--images 4952 --classes 20 --dets 100 --boxes 3 --reps 15 --batch 64]

After a warm-up: the median over --reps repetitions of compute() (synchronous, wall clock) and of appending the whole set in
batches of --batch images from device tensors (wall clock around a synchronised loop).  Prints one JSON line.  The restatement
lives with the tests, so this tool runs from a source checkout.  For the per-kernel split run it under a kernel trace with --reps 3.

    python -m yolo355.tools.apeval_bench --coco [--images 5000 --classes 80 --dets 100 --boxes 14 --reps 15 --batch 64]

the same for COCO AP (yolo355.apeval.CocoEval) on a synthetic set of COCO val2017 size from tests/coco_ap_ref.py::synth_set: 0 to
--boxes boxes per image (val2017 has 7.4 on average), 15 % of them crowd, sizes drawn evenly from ten shapes across the three area
ranges; the host yardstick is the literal restatement tests/coco_ap_ref.py::evaluate, a checker written for clarity, not speed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--coco", action="store_true", help="COCO AP (CocoEval) on a val2017-sized set instead of VOC mAP")
    ap.add_argument("--images", type=int, default=None, help="default 4952 (VOC07 test), with --coco 5000 (val2017)")
    ap.add_argument("--classes", type=int, default=None, help="default 20, with --coco 80")
    ap.add_argument("--dets", type=float, default=100.0)
    ap.add_argument("--boxes", type=float, default=None, help="boxes per image: the mean (default 3), with --coco the maximum (default 14)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (it takes a while)")
    a = ap.parse_args(argv)
    a.images = a.images if a.images is not None else 5000 if a.coco else 4952
    a.classes = a.classes if a.classes is not None else 80 if a.coco else 20
    a.boxes = a.boxes if a.boxes is not None else 14 if a.coco else 3.0
    tests = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "tests")
    sys.path.insert(0, os.path.normpath(tests))
    from yolo355.apeval import ApEval, CocoEval
    if a.coco:
        import coco_ap_ref as R
        gt, boxes, scores, cls, count, ids = R.synth_set(7, a.images, a.classes, a.dets, int(a.boxes))
    else:
        import voc_ap_ref as R
        gt, boxes, scores, cls, count = R.synth_set(7, a.images, a.classes, a.dets, a.boxes)
    n = int(count.sum())
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (boxes, scores, cls, count)]
    ev = CocoEval(a.classes, gt, image_ids=ids, max_dets=n) if a.coco else ApEval(a.classes, gt, max_dets=n)

    def append():
        for i0 in range(0, a.images, a.batch):
            i1 = min(a.images, i0 + a.batch)
            ev.add(i0, *[t[i0:i1] for t in dev])
        torch.cuda.synchronize()
    t_add, t_cmp = [], []
    res = None
    for rep in range(a.reps + 2):                        # two warm-up rounds
        ev.reset()
        t0 = time.perf_counter()
        append()
        t1 = time.perf_counter()
        res = ev.compute()
        t2 = time.perf_counter()
        if rep >= 2:
            t_add.append(t1 - t0)
            t_cmp.append(t2 - t1)
    out = dict(images=a.images, classes=a.classes, detections=n, boxes=int(sum(len(g) for g in gt)), reps=a.reps,
               gpu_compute_ms=1e3 * statistics.median(t_cmp), gpu_append_ms=1e3 * statistics.median(t_add))
    if a.coco:
        out["gpu_stats"] = [float(v) for v in res]
        out["crowd_share"] = float(np.concatenate(gt)[:, 6].mean())
        if not a.no_host:
            t0 = time.perf_counter()
            ref = R.evaluate(a.classes, gt, boxes, scores, cls, count, ids)
            out["host_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
            out["host_stats"] = [float(v) for v in ref["stats"]]
            out["equal"] = bool(np.array_equal(ev.precision, ref["precision"]) and np.array_equal(ev.recall, ref["recall"])
                                and np.array_equal(res, ref["stats"]))
        ev.close()
        print(json.dumps(out))
        return out
    out["gpu_mean_ap"] = res[1]
    if not a.no_host:
        t0 = time.perf_counter()
        ref = R.evaluate(a.classes, gt, boxes, scores, cls, count)
        out["host_restatement_ms"] = 1e3 * (time.perf_counter() - t0)
        out["host_mean_ap"] = ref["mean"]
        out["equal"] = bool(np.array_equal(res[0], ref["ap"]))
    ev.close()
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
