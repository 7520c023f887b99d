#!/usr/bin/env python3
"""Golden vectors of the anchor fit, from the REFERENCE itself (generate_ab_kmeans.py) -> tests/golden/anchors.npz.

Runs only where the reference is checked out (import recipe of gen_golden.py: its directory on sys.path, the names it pulls
from `data` stubbed); nothing of its source travels.  Inputs come from tests/anchors_cases.py (seeded), so only the reference's
outputs are stored, per case <tag>:

  <tag>/init         the initial centroids [k, 2] (init_centroids' list, or the boxes of the given indices); the reference's list
                     is shorter when k-means++ finds nothing to append: the unfilled slots are (0, 0), <tag>/nfound is its length
  <tag>/first, /u    the draws the reference made after np.random.seed(seed): choice(n, 1)[0], then random() k - 1 times
  <tag>/losses       the loss of every do_kmeans step
  <tag>/anchors      the centroids anchor_box_kmeans returns [k, 2]
  <tag>/groups       the group of every box in the last step (uint8 [n])
  <tag>/iterations   the number of do_kmeans steps
  <tag>/margins      [3]: the smallest gap between a box's best and second-best distance over all steps; the smallest
                     | |old_loss - loss| - convergence |; the smallest clearance of a k-means++ pick relative to sum D

Asserted for every case, so that the reference alone decides every discrete outcome and another order of the sums cannot
change it: assignment gaps > 1e-9 (centroids that are bit for bit the winner do not compete: the lowest index wins on any
implementation), convergence margins > 4 * 14 n^2 2^-53, pick clearances > 1e-9 * sum D on both sides (a pick that finds
nothing needs sum D == 0 exactly).

    python tests/golden/gen_golden_anchors.py
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (REF, sys.dont_write_bytecode)

import anchors_cases as AC  # noqa: E402
import anchors_ref as R  # noqa: E402


def import_script():
    data = types.ModuleType("data")
    for name in ("BaseTransform", "VOC_ROOT", "VOCDetection", "coco_root", "COCODataset"):
        setattr(data, name, None)
    saved = sys.modules.get("data")
    sys.modules["data"] = data
    sys.path.insert(0, G.REF)
    try:
        return importlib.import_module("generate_ab_kmeans")
    finally:
        sys.path.remove(G.REF)
        if saved is not None:
            sys.modules["data"] = saved
        else:
            del sys.modules["data"]


def run_case(ref, tag):
    c = AC.case(tag)
    wh, n, k = c["wh"], c["n"], c["k"]
    boxes = [ref.Box(0, 0, float(w), float(h)) for w, h in wh]
    index_of = {id(b): i for i, b in enumerate(boxes)}
    rec = dict(steps=[], first=-1, u=[], init=None, assign_margin=np.inf, pick_margin=np.inf)

    orig_do, orig_choice, orig_random, orig_sample = ref.do_kmeans, np.random.choice, np.random.random, ref.random.sample

    def do_kmeans(n_anchors, bxs, centroids):
        if rec["init"] is None:
            rec["init"] = [(b.w, b.h) for b in centroids]
        for box in bxs:                                            # margins, with the reference's own iou()
            d = [1 - ref.iou(box, cen) for cen in centroids]
            best = min(range(len(d)), key=lambda i: (d[i], i))
            others = [d[i] for i, cen in enumerate(centroids) if i != best and (cen.w, cen.h) != (centroids[best].w, centroids[best].h)]
            others.append(1)                                       # the start value of min_distance
            if d[best] < 1:
                rec["assign_margin"] = min(rec["assign_margin"], min(others) - d[best])
            else:
                assert all(v == 1 for v in d), (tag, d)            # nobody beats the start: exactly 1 everywhere
        new, groups, loss = orig_do(n_anchors, bxs, centroids)
        g = np.full(n, 255, np.uint8)
        for gi, grp in enumerate(groups):
            for b in grp:
                g[index_of[id(b)]] = gi
        assert (g < n_anchors).all()
        rec["steps"].append(dict(loss=float(loss), groups=g, new=[(b.w, b.h) for b in new]))
        return new, groups, loss

    def choice(a, size):
        r = orig_choice(a, size)
        rec["first"] = int(r[0])
        return r

    def random():
        v = orig_random()
        rec["u"].append(float(v))
        return v

    ref.do_kmeans = do_kmeans
    np.random.choice, np.random.random = choice, random
    if c["init_index"] is not None:
        ref.random.sample = lambda population, kk: list(c["init_index"])
    try:
        if c["seed"] is not None:
            np.random.seed(c["seed"])
        with contextlib.redirect_stdout(io.StringIO()):
            cents = ref.anchor_box_kmeans(boxes, k, AC.CONVERGENCE, c["iters"], plus=c["init_index"] is None)
    finally:
        ref.do_kmeans, np.random.choice, np.random.random, ref.random.sample = orig_do, orig_choice, orig_random, orig_sample

    losses = np.array([s["loss"] for s in rec["steps"]], np.float64)
    iterations = len(rec["steps"])
    init = np.zeros((k, 2), np.float64)
    init[:len(rec["init"])] = np.array(rec["init"], np.float64).reshape(-1, 2)
    anchors = np.array([(b.w, b.h) for b in cents], np.float64)
    assert np.array_equal(anchors, np.array(rec["steps"][-1]["new"], np.float64))

    # the stop rule's margins: every test the loop made
    conv_margin, old = np.inf, losses[0]
    for s in range(1, iterations):
        conv_margin = min(conv_margin, abs(abs(old - losses[s]) - AC.CONVERGENCE))
        old = losses[s]
    assert conv_margin > 4 * AC.loss_bound(n), (tag, conv_margin)
    assert rec["assign_margin"] > 1e-9, (tag, rec["assign_margin"])

    # the k-means++ picks again, with the reference's iou() and its sequential sums: clearances on both sides
    if c["init_index"] is None:
        chosen = [boxes[rec["first"]]]
        assert len(rec["u"]) == k - 1
        for j in range(k - 1):
            D = []
            for box in boxes:
                md = 1
                for cen in chosen:
                    d = 1 - ref.iou(box, cen)
                    if d < md:
                        md = d
                D.append(md)
            prefix = np.cumsum(np.array(D, np.float64))
            total = float(prefix[-1])
            thresh = total * rec["u"][j]
            above = np.nonzero(prefix > thresh)[0]
            if len(above):
                i = int(above[0])
                lo = thresh - (prefix[i - 1] if i else 0.0)
                hi = prefix[i] - thresh
                assert lo > 1e-9 * total and hi > 1e-9 * total, (tag, j, lo, hi, total)
                rec["pick_margin"] = min(rec["pick_margin"], lo / total, hi / total)
                chosen.append(boxes[i])
            else:
                assert total == 0.0, (tag, j, total)
        assert [(b.w, b.h) for b in chosen] == rec["init"], tag
        first, u = rec["first"], np.array(rec["u"], np.float64)
    else:
        first, u = -1, np.zeros(0, np.float64)

    # the restatement must say the same, bit for bit
    mine = R.fit(wh, k, first=first, u=u, init_index=c["init_index"], iters=c["iters"], convergence=AC.CONVERGENCE)
    same = (np.array_equal(mine["init"], init) and np.array_equal(mine["losses"], losses) and np.array_equal(mine["anchors"], anchors)
            and np.array_equal(mine["groups"], rec["steps"][-1]["groups"]) and mine["iterations"] == iterations)
    print("%-18s n %5d k %2d steps %3d loss %.9g found %d margins: assign %.3g conv %.3g pick %.3g restatement %s"
          % (tag, n, k, iterations, losses[-1], len(rec["init"]), rec["assign_margin"], conv_margin, rec["pick_margin"], "equal" if same else "DIFFERS"))
    assert same, tag
    return {"init": init, "nfound": np.array([len(rec["init"])], np.int32), "first": np.array([first], np.int64), "u": u, "losses": losses,
            "anchors": anchors, "groups": rec["steps"][-1]["groups"], "iterations": np.array([iterations], np.int32),
            "margins": np.array([rec["assign_margin"], conv_margin, rec["pick_margin"]], np.float64)}


def main():
    ref = import_script()
    out = {}
    for tag in AC.TAGS:
        for key, v in run_case(ref, tag).items():
            out["%s/%s" % (tag, key)] = v
    path = os.path.join(HERE, "anchors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
