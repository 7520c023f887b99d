"""Inputs of the augmentation tests, from a build-owned seeded generator: tests/golden/augment.npz stores only sample ids
(frame shape, seed, output size) and the reference's results for them (tests/golden/gen_golden_augment.py)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
MEAN, STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
# (height, width, number of boxes) of the frames; the output sizes [H, W] (non-square: an H / W swap shows)
SHAPES = [(37, 53, 3), (64, 48, 1), (5, 7, 2), (1, 1, 1)]
SIZES = [(32, 64), (64, 32)]
SEEDS = range(64)


def frame(shape, seed):
    """uint8 [h,w,3] BGR: noise, with flat red, magenta-red (hue just below 360), grey (s == 0) and black pixels sprinkled in, so
    that a hue delta wraps past 360 and below 0 and the s == 0 branch of HSV -> BGR runs"""
    h, w, _ = SHAPES[shape]
    rs = np.random.RandomState(100000 + 1000 * shape + seed)
    f = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    flat = f.reshape(-1, 3)
    flat[0::7] = (0, 0, 255)
    flat[3::7] = (20, 0, 255)
    flat[5::11] = (128, 128, 128)
    flat[6::13] = 0
    return f


def target(shape, seed):
    """float64 [n,5] = (xmin, ymin, xmax, ymax, cls), boxes in [0,1]"""
    n = SHAPES[shape][2]
    rs = np.random.RandomState(200000 + 1000 * shape + seed)
    c = rs.uniform(0.15, 0.85, (n, 2))
    half = rs.uniform(0.05, 0.4, (n, 2))
    t = np.zeros((n, 5), np.float64)
    t[:, :2] = np.clip(c - half, 0.0, 1.0)
    t[:, 2:4] = np.clip(c + half, 0.0, 1.0)
    t[:, 4] = rs.randint(0, 20, n)
    return t


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def samples(gold):
    """[(tag, shape, seed, size index)] of the stored samples"""
    return [("s%d" % i, int(a), int(b), int(c)) for i, (a, b, c) in enumerate(gold["ids"])]
