"""Seeded box sets and the case table of the anchor fit (tests/test_anchors_ref.py, tests/test_anchors.py and
tests/golden/gen_golden_anchors.py share them): the smallest shapes at which the fit can still go wrong.  Only the reference's
outputs are stored in tests/golden/anchors.npz; the inputs are made here."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1024                     # Y355_ANCHORS_CHUNK: 4097 boxes are four chunks and one box
EPS = 2.0 ** -53
CONVERGENCE, ITERS = 1e-6, 1000  # generate_ab_kmeans.py:166-167


def random_boxes(seed, n, size=416.0):
    """n boxes around a handful of (w, h) modes, as a data set's boxes at an input size of `size`: continuous draws, so no two
    boxes and no two distances are equal"""
    rs = np.random.RandomState(seed)
    modes = np.exp(rs.uniform(np.log(12.0), np.log(0.8 * size), size=(7, 2)))
    which = rs.randint(0, len(modes), size=n)
    wh = modes[which] * np.exp(rs.normal(0.0, 0.35, size=(n, 2)))
    return np.ascontiguousarray(np.clip(wh, 1.5, size), dtype=np.float64)


# 4 distinct sizes whose sums are exact in any order (few mantissa bits), 16 boxes of each, interleaved
FOUR_SIZES = np.array([[24.0, 40.0], [96.5, 64.0], [200.0, 180.25], [48.0, 300.0]], np.float64)


def boxes(name):
    if name == "one":
        return np.array([[37.25, 81.5]], np.float64)
    if name == "b300":
        return random_boxes(300, 300)
    if name == "b257":
        return random_boxes(257, 257)
    if name == "b1500":
        return random_boxes(1500, 1500)
    if name == "b4097":
        return random_boxes(4097, 4097)
    if name == "four":
        return np.ascontiguousarray(FOUR_SIZES[np.arange(64) % 4])
    if name == "same8":
        return np.ascontiguousarray(np.tile(np.array([[50.5, 120.25]], np.float64), (8, 1)))
    raise KeyError(name)


# tag -> dict(boxes, k, seed, iters, init_index): seed is the reference's np.random.seed; init_index (plus=False) replaces it
CASES = {
    "n1_k1": dict(boxes="one", k=1, seed=0),
    "n300_k1": dict(boxes="b300", k=1, seed=1),
    "n257_k3": dict(boxes="b257", k=3, seed=2),
    "n1500_k5": dict(boxes="b1500", k=5, seed=3),
    "n4097_k9": dict(boxes="b4097", k=9, seed=4),
    "n300_k16": dict(boxes="b300", k=16, seed=5),
    "n1500_k5_iters3": dict(boxes="b1500", k=5, seed=3, iters=3),
    # boxes 0 and 4 have one size, index 1 twice, index 0 again: groups 1, 3 and 5 are empty from the first step and become
    # (0, 0), the size nobody starts at joins its nearest; the lowest index wins every tie
    "four_dup_k6": dict(boxes="four", k=6, init_index=[0, 4, 1, 1, 2, 0]),
    "same8_k3": dict(boxes="same8", k=3, seed=6),
}
TAGS = list(CASES)


def case(tag):
    c = dict(iters=ITERS, seed=None, init_index=None)
    c.update(CASES[tag])
    c["wh"] = boxes(c["boxes"])
    c["n"] = len(c["wh"])
    return c


def centroid_bound(n):
    """relative: two orders of a float64 sum of n non-negative terms differ by at most 2 (n - 1) 2^-53 relative, and with equal
    groups a centroid carries the error of one iteration only"""
    return 2.0 * n * EPS


def loss_bound(n):
    """absolute: a relative centroid error e moves an IoU by at most 6 e; each of the n distance terms is charged 12 n 2^-53,
    plus the order term of the loss sum itself (2 n 2^-53 relative of a sum <= n)"""
    return 14.0 * n * n * EPS


def load_golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "anchors.npz")) as z:
        return {k: z[k] for k in z.files}


# ANCHOR_SIZE-style constants (data/config.py:10, grid units of stride 32) in pixels, and a set with a (0, 0) anchor
CONFIG_ANCHORS_PX = np.array([[1.19, 1.98], [2.79, 4.59], [4.53, 8.92], [8.06, 5.29], [10.32, 10.65]], np.float64) * 32.0
