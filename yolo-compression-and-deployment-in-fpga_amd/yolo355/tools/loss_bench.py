"""Times the training targets and losses on the GPU (yolo355.loss.YoloLoss) at a VOC-like batch, and the host restatement of
the same contract (tests/loss_ref.py, the yardstick) on the same data:

    python -m yolo355.tools.loss_bench [--arch slim_yolo_v2|tiny_yolo_v3|yolo_v3 --batch 64 --size 416 --classes 20 --labels 2.4 --reps 30]

After a warm-up: the median over --reps repetitions (wall clock, both calls are synchronous) of set_labels (host check, upload,
target assignment) and of compute (terms, sums, four numbers back) on prediction maps that are already on the device, as
the models' loss branch has them after its upload.  Prints one JSON line.  The restatement lives with the tests, so this
tool runs from a source checkout."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

GEOM = {"slim_yolo_v2": (16, "ANCHOR_SIZE"), "tiny_yolo_v3": ([16, 32], "TINY_MULTI_ANCHOR_SIZE"), "yolo_v3": ([8, 16, 32], "MULTI_ANCHOR_SIZE")}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="slim_yolo_v2", choices=sorted(GEOM))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--labels", type=float, default=2.4, help="mean labels per image (VOC07+12 trainval: about 2.4)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement")
    a = ap.parse_args(argv)
    tests = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "tests")
    sys.path.insert(0, os.path.normpath(tests))
    from yolo355 import synth
    from yolo355.loss import YoloLoss
    strides, an = GEOM[a.arch]
    anchors = getattr(synth, an)
    size = [a.size, a.size]
    u = (synth.uniform_pm1(11, (a.batch,)).astype(np.float64) + 1.0) / 2.0
    counts = np.floor(u * 2.0 * a.labels + 0.5).astype(int)                 # 0 .. 2 * mean labels, the mean as asked
    labels = []
    for b, n in enumerate(counts):
        v = (synth.uniform_pm1(100 + b, (max(int(n), 1), 5)).astype(np.float64) + 1.0) / 2.0
        rows = []
        for cx, cy, sw, sh, c in v[:n]:
            w, h = 0.05 + 0.55 * sw, 0.05 + 0.55 * sh
            rows.append([max(cx - w / 2, 0.0), max(cy - h / 2, 0.0), min(cx + w / 2, 1.0), min(cy + h / 2, 1.0), int(c * a.classes) % a.classes])
        labels.append(rows)
    h = YoloLoss(size, strides, anchors, a.classes, max_batch=a.batch, max_labels_per_image=max(1, int(counts.max())))
    maps = [synth.uniform_pm1(500 + l, (a.batch, h.num_anchors * (5 + a.classes), hs, ws)) * np.float32(2.0) for l, (hs, ws) in enumerate(h.grids)]
    dev = [torch.from_numpy(m).to(h.device) for m in maps]
    t_set, t_cmp = [], []
    out = None
    for rep in range(a.reps + 2):                                           # two warm-up rounds
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.set_labels(labels)
        t1 = time.perf_counter()
        out, parts = h.compute(dev)
        t2 = time.perf_counter()
        if rep >= 2:
            t_set.append(t1 - t0)
            t_cmp.append(t2 - t1)
    res = dict(arch=a.arch, batch=a.batch, size=a.size, classes=a.classes, anchors_per_image=h.num_anchors_total, labels=int(counts.sum()),
               reps=a.reps, gpu_set_labels_ms=1e3 * statistics.median(t_set), gpu_compute_ms=1e3 * statistics.median(t_cmp),
               gpu_losses=[float(v) for v in out])
    if not a.no_host:
        import loss_ref as R
        multi = not np.isscalar(strides)
        t0 = time.perf_counter()
        target = R.make_targets(size, strides, labels, anchors, multi)
        t1 = time.perf_counter()
        want, _ = R.loss(maps, target, strides, anchors, a.classes, size, 1.0 if multi else float(strides))
        t2 = time.perf_counter()
        res.update(host_targets_ms=1e3 * (t1 - t0), host_loss_ms=1e3 * (t2 - t1), host_losses=[float(v) for v in want],
                   max_rel_diff=float(np.max(np.abs(out - want) / np.abs(want))))
    h.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
