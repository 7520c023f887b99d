#!/usr/bin/env python3
"""Golden vectors of the training augmentation, from the REFERENCE itself -> tests/golden/augment.npz.

Runs only where the reference is checked out; nothing of its source travels.  utils/augmentations.py is loaded as a file (its
package's __init__ pulls in the evaluators) under stand-ins:

  * `torchvision` / `torchvision.transforms`: empty stubs; `torch` is the real one.
  * `cv2`: tests/augment_ref.py's resize and cvtColor (float32, three channels) -- NumPy restatements of OpenCV 4.x's
    published algorithm, UNPINNED for the reason given there.  Everything around the two calls is the reference's own code.
  * `augmentations.random` (the module's `from numpy import random`) is replaced by a proxy that forwards randint / uniform
    to numpy.random and whose choice(seq) is seq[numpy.random.randint(len(seq))]: `random.choice(self.sample_options)` raises
    ValueError (inhomogeneous array) under NumPy 2, and under the NumPy of the reference's time it drew exactly one
    randint(0, 6) -- choice(6) and randint(6) give the same stream for the same seed (asserted below).

Inputs come from tests/augment_cases.py (seeded), so per stored sample only ids and the reference's outputs are kept:
ids [n,3] = (frame shape, seed, output size); per sample sK/image float32 [H,W,3] BGR, sK/target float64 [m,5], sK/shape (the
image's shape on entry to cv2.resize), sK/next (numpy.random.randint(2 ** 30) right after the sample: the stream's position).
The whole sweep (every shape x seed x size) is run and checked against yolo355.augment.draw + augment_ref.pixels; stored is the
smallest subset found (greedy set cover) that still covers every item of COVER.

    python tests/golden/gen_golden_augment.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"))
sys.path.insert(0, os.path.dirname(HERE))

import augment_cases as AC  # noqa: E402
import augment_ref as R  # noqa: E402
from yolo355 import augment as A  # noqa: E402

COVER = (["brightness", "no_brightness", "contrast_first", "contrast_last", "contrast", "no_contrast", "saturation", "no_saturation", "hue",
          "no_hue", "hue_above_360", "hue_below_0", "expand", "no_expand", "aspect", "centre", "dropped", "kept", "mirror", "no_mirror",
          "neg_origin", "fill_in_window"] + ["mode%d" % m for m in range(6)] + ["shape%d" % s for s in range(len(AC.SHAPES))] +
         ["size%d" % s for s in range(len(AC.SIZES))])


class RandomProxy:
    randint = staticmethod(lambda *a, **k: np.random.randint(*a, **k))
    uniform = staticmethod(lambda *a, **k: np.random.uniform(*a, **k))

    @staticmethod
    def choice(seq):
        return seq[np.random.randint(len(seq))]


def load_reference():
    shapes = []

    def resize(img, dsize):
        shapes.append(img.shape)
        return R.resize(img, dsize)
    cv2 = types.ModuleType("cv2")
    cv2.resize, cv2.cvtColor, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = resize, R.cvtColor, R.COLOR_BGR2HSV, R.COLOR_HSV2BGR
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    spec = importlib.util.spec_from_file_location("ref_augmentations", os.path.join(REF, "utils", "augmentations.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.random = RandomProxy
    return mod, shapes


def tags_of(shape, size, frame, p, trace):
    t = set(trace) - {"exhausted"}
    t |= {"brightness" if p.brightness_on else "no_brightness", "contrast_first" if p.contrast_first else "contrast_last",
          "contrast" if p.contrast_on else "no_contrast", "saturation" if p.saturation_on else "no_saturation",
          "hue" if p.hue_on else "no_hue", "mirror" if p.mirror else "no_mirror", "shape%d" % shape, "size%d" % size}
    if "expand" not in t:
        t.add("no_expand")
    if p.hue_on:                                                   # the hue plane as RandomHue sees it
        im = frame.astype(np.float32)
        if p.brightness_on:
            im += np.float32(p.brightness)
        if p.contrast_on and p.contrast_first:
            im *= np.float32(p.contrast)
        h = R.bgr2hsv(im)[:, :, 0] + np.float32(p.hue)
        if (h > 360.0).any():
            t.add("hue_above_360")
        if (h < 0.0).any():
            t.add("hue_below_0")
    cropped = any(x in t for x in ("kept", "dropped"))
    if cropped and p.oy < 0 and p.ox < 0:
        t.add("neg_origin")
    if cropped and "expand" in t and (p.oy > 0 or p.ox > 0 or p.oy + frame.shape[0] < p.vh or p.ox + frame.shape[1] < p.vw):
        t.add("fill_in_window")
    return t


def main():
    for s in range(8):                                             # the proxy's claim
        np.random.seed(s)
        a = [int(np.random.choice(6)) for _ in range(32)]
        np.random.seed(s)
        assert a == [int(np.random.randint(6)) for _ in range(32)]
    mod, shapes = load_reference()
    runs = []
    for si, size in enumerate(AC.SIZES):
        aug = mod.SSDAugmentation(list(size))
        assert tuple(aug.mean) == AC.MEAN and tuple(aug.std) == AC.STD
        for shape in range(len(AC.SHAPES)):
            for seed in AC.SEEDS:
                frame, tgt = AC.frame(shape, seed), AC.target(shape, seed)
                np.random.seed(seed)
                del shapes[:]
                img, boxes, labels = aug(frame.copy(), tgt[:, :4].copy(), tgt[:, 4].copy())
                nxt = int(np.random.randint(1 << 30))
                assert img.dtype == np.float32 and img.shape == (size[0], size[1], 3) and len(shapes) == 1
                out = np.hstack((boxes, labels[:, None]))
                # our side on the same seed: the draws, the boxes, the pixels
                np.random.seed(seed)
                trace = []
                p, b2, l2 = A.draw(frame.shape[0], frame.shape[1], tgt[:, :4], tgt[:, 4], trace=trace)
                assert int(np.random.randint(1 << 30)) == nxt, (shape, seed, "draws consumed")
                assert (p.vh, p.vw, 3) == tuple(shapes[0]), (shape, seed, p, shapes[0])
                assert b2.tobytes() == boxes.astype(np.float64).tobytes() and np.array_equal(l2, labels), (shape, seed)
                mine = R.pixels(frame, p, size, AC.MEAN, AC.STD)
                assert mine.tobytes() == img.tobytes(), (shape, seed, "pixels", np.abs(mine - img).max())
                assert "exhausted" not in trace
                runs.append(dict(id=(shape, seed, si), image=img, target=out, shape=np.array(shapes[0][:2], np.int32), next=nxt,
                                 tags=tags_of(shape, si, frame, p, trace)))
    count = {c: sum(c in r["tags"] for r in runs) for c in COVER}
    print("sweep of %d samples; occurrences:" % len(runs), count)
    missing = [c for c in COVER if not count[c]]
    assert not missing, "not covered by the sweep: %s" % missing
    # greedy set cover, ties to the smaller image and then the earlier sample
    need, chosen = set(COVER), []
    while need:
        best = max(runs, key=lambda r: (len(r["tags"] & need), -runs.index(r)))
        assert best["tags"] & need
        chosen.append(best)
        need -= best["tags"]
    chosen.sort(key=lambda r: r["id"][::-1])
    covered = set().union(*[r["tags"] for r in chosen])
    assert set(COVER) <= covered
    out = {"ids": np.array([r["id"] for r in chosen], np.int32), "cover": np.array(COVER)}
    for i, r in enumerate(chosen):
        out["s%d/image" % i] = r["image"]
        out["s%d/target" % i] = r["target"]
        out["s%d/shape" % i] = r["shape"]
        out["s%d/next" % i] = np.array([r["next"]], np.int64)
        out["s%d/tags" % i] = np.array(sorted(r["tags"]))
        print("s%d" % i, r["id"], sorted(r["tags"]))
    path = os.path.join(HERE, "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(chosen), "samples")


if __name__ == "__main__":
    main()
