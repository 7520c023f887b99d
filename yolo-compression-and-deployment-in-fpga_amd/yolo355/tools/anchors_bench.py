"""Times the anchor fit on the GPU (yolo355.anchors.AnchorFit) on a seeded synthetic box set of COCO's size, and one
iteration of the same contract as a vectorised NumPy statement on the host:

    python -m yolo355.tools.anchors_bench [--boxes 860000 -k 9 --restarts 8 --reps 15 --seed 0]

Prints one JSON line:
  fit_ms, fit_steps        a whole fit with the reference's settings (k-means++, convergence 1e-6, at most 1000 iterations), all
                           restarts side by side: wall clock of the synchronous call (median of --reps), the steps of each restart
  iteration_ms             one iteration of all restarts (one assign and one update launch): the difference of two fits that
                           cannot converge (convergence 0) capped at 104 and at 8 iterations, over the 96 steps between them
                           (medians of --reps; the fastest and the slowest repetition of both are in the line too)
  start_ms                 what is left of the 8-iteration fit: k-means++ (2 (k - 1) launches), uploads, the reads of `done`
  host_numpy_iteration_ms  the same iteration of all restarts as NumPy statements over the (box, centroid) pairs
  first_assignments_equal  the assignments of the first iteration of every restart, all boxes, equal that statement exactly
"""
import argparse
import json
import statistics
import time

import numpy as np


def synthetic_boxes(seed, n, size=416.0):
    """(w, h) around a dozen modes between 8 pixels and the input size, log-normal spread: continuous, so no ties"""
    rs = np.random.RandomState(seed)
    modes = np.exp(rs.uniform(np.log(8.0), np.log(0.9 * size), size=(12, 2)))
    wh = modes[rs.randint(0, len(modes), size=n)] * np.exp(rs.normal(0.0, 0.45, size=(n, 2)))
    return np.ascontiguousarray(np.clip(wh, 1.0, size), dtype=np.float64)


def numpy_iteration(boxes, cents):
    """one do_kmeans step (generate_ab_kmeans.py:87-115) of one restart: distances of all (box, centroid) pairs, the first
    minimum per box (what the strict `<` keeps), the loss and the new centroids"""
    w1, h1 = boxes[:, 0:1], boxes[:, 1:2]
    w2, h2 = cents[None, :, 0], cents[None, :, 1]
    inter = (np.minimum(w1 / 2, w2 / 2) - np.maximum(-w1 / 2, -w2 / 2)) * (np.minimum(h1 / 2, h2 / 2) - np.maximum(-h1 / 2, -h2 / 2))
    d = 1.0 - inter / (w1 * h1 + w2 * h2 - inter)
    g = np.argmin(d, axis=1)
    k = len(cents)
    cnt = np.maximum(np.bincount(g, minlength=k), 1)
    new = np.stack([np.bincount(g, weights=boxes[:, 0], minlength=k) / cnt, np.bincount(g, weights=boxes[:, 1], minlength=k) / cnt], axis=1)
    return g.astype(np.int32), float(d[np.arange(len(boxes)), g].sum()), new


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=860000)
    ap.add_argument("-k", type=int, default=9)
    ap.add_argument("--restarts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy statement")
    a = ap.parse_args(argv)
    import torch
    from yolo355 import anchors as A
    boxes = synthetic_boxes(a.seed, a.boxes)
    first, u = A.draws(a.boxes, a.k, a.seed, a.restarts)
    h = A.AnchorFit(a.boxes, a.restarts, a.k)
    h.set_boxes(boxes)

    def timed(**kw):
        ts = []
        for rep in range(a.reps + 1):                                       # one warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.fit(a.k, first=first, u=u, **kw)
            ts.append(time.perf_counter() - t0)
        return 1e3 * statistics.median(ts[1:]), [1e3 * min(ts[1:]), 1e3 * max(ts[1:])]

    (t104, r104), (t8, r8) = timed(iters=104, convergence=0.0), timed(iters=8, convergence=0.0)
    it_ms = (t104 - t8) / 96.0
    fit_ms, fit_range = timed()
    runs, best = h.result()
    res = dict(boxes=a.boxes, k=a.k, restarts=a.restarts, reps=a.reps, chunk=A.CHUNK, fit_ms=fit_ms, fit_ms_min_max=fit_range,
               fit_steps=[r.iterations for r in runs],
               best_restart=best, best_loss_per_box=runs[best].loss / a.boxes, iteration_ms=it_ms, start_ms=t8 - 9 * it_ms,
               fit_of_8_iterations_ms=t8, fit_of_8_iterations_ms_min_max=r8, fit_of_104_iterations_ms=t104,
               fit_of_104_iterations_ms_min_max=r104)
    res["mean_iou"] = h.score(runs[best].anchors)[0]
    if not a.no_host:
        equal, t_host = True, 0.0
        for r in range(a.restarts):
            t0 = time.perf_counter()
            g, _, _ = numpy_iteration(boxes, runs[r].init)
            t_host += time.perf_counter() - t0
            equal = equal and bool(np.array_equal(g, h.score(runs[r].init, with_index=True)[2]))
        res.update(host_numpy_iteration_ms=1e3 * t_host, first_assignments_equal=equal)
    h.close()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
