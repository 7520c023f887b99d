"""Inputs of the target / loss tests (tests/test_loss_ref.py, tests/test_loss.py) and of their golden generator
(tests/golden/gen_golden_loss.py): label lists and synthetic prediction maps, all from yolo355.synth's seeded streams."""
import numpy as np

from yolo355 import synth

# head geometries: tag -> (input size [h, w], strides (int: gt_creator; list: multi_gt_creator), anchors)
GEOM = {
    "t64": ([64, 64], 16, synth.ANCHOR_SIZE_MASK),
    "t96x64": ([96, 64], 16, synth.ANCHOR_SIZE_MASK),
    "m2": ([64, 64], [16, 32], synth.TINY_MULTI_ANCHOR_SIZE),
    "m3": ([64, 64], [8, 16, 32], synth.MULTI_ANCHOR_SIZE),
    "m3_416": ([416, 416], [8, 16, 32], synth.MULTI_ANCHOR_SIZE),
}


def is_multi(tag):
    return not np.isscalar(GEOM[tag][1])


def wh_mul(tag):
    return 1.0 if is_multi(tag) else float(GEOM[tag][1])


def num_anchors(tag):
    size, strides, anchors = GEOM[tag]
    return len(anchors) // (len(strides) if is_multi(tag) else 1)


def _box(cx, cy, w_px, h_px, cls, size):
    """a label whose box is w_px x h_px pixels around (cx, cy) (fractions of the image)"""
    w, h = w_px / size[1], h_px / size[0]
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, cls]


def random_labels(seed, n, num_classes, lo=0.05, hi=0.6):
    """n labels: centres uniform in the image, sides uniform in [lo, hi] of it, clipped to [0, 1]"""
    u = (synth.uniform_pm1(seed, (max(n, 1), 5)).astype(np.float64) + 1.0) / 2.0
    out = []
    for cx, cy, sw, sh, c in u[:n]:
        w, h = lo + (hi - lo) * sw, lo + (hi - lo) * sh
        out.append([max(cx - w / 2, 0.0), max(cy - h / 2, 0.0), min(cx + w / 2, 1.0), min(cy + h / 2, 1.0), int(c * num_classes) % num_classes])
    return out


def crafted_labels(tag):
    """Image 0 of the target cases: in list order, all centred in one cell of the finest level --
      0  a box with IoU > ignore_thresh against two anchors (one positive slot P, one ignore slot I)
      1  a box whose only write is a positive on slot I          (positive over an earlier ignore)
      2  a box whose positive lands on slot I again and whose ignore lands on slot P
                                                                (later positive wins; ignore over an earlier positive)
      3  a box narrower than one pixel                           (skipped)
      4  a small box somewhere else
    The pixel geometry is the same in every case of a kind, so the properties carry over; the tests assert them on the
    restatement.  With the tiny-v3 anchors no box inside 64 x 64 passes 0.5 against two anchors: "m2" has the overwrite only."""
    size = GEOM[tag][0]
    cx, cy = 28.8 / size[1], 31.0 / size[0]         # pixels (28.8, 31): the crafted boxes live in the top-left 64 x 64 pixels, off every cell edge
    if tag in ("t64", "t96x64"):
        dims = [(40.0, 60.8), (28.8, 44.8), (39.2, 60.0)]
    elif tag == "m2":
        dims = [(34.0, 60.0), (36.0, 62.0), (33.0, 58.0)]
    else:
        dims = [(45.0, 62.0), (52.0, 62.0), (48.0, 62.0)]
    out = [_box(cx, cy, dims[0][0], dims[0][1], 0, size), _box(cx, cy, dims[1][0], dims[1][1], 1, size),
           _box(cx, cy, dims[2][0], dims[2][1], 1, size)]
    out.append([0.5, 0.2 * 64 / size[0], 0.5 + 0.5 / size[1], 0.6 * 64 / size[0], 1])
    out.append(_box(0.8 * 64 / size[1], 0.2 * 64 / size[0], 12.8, 19.2, 0, size))
    return out


def target_labels(tag):
    """B = 3: the crafted image, an image without labels, an image with 70 labels (more than a wave is wide)"""
    return [crafted_labels(tag), [], random_labels(1000 + len(tag), 70, 2)]


TARGET_CASES = ["t64", "t96x64", "m2", "m3"]

# loss cases: (tag, geometry, classes, batch)
LOSS_CASES = [("%s_c%d_b%d" % (g, c, b), g, c, b) for g in TARGET_CASES for c in (2, 20) for b in (1, 5)] + [("m3_416_c20_b2", "m3_416", 20, 2)]


def loss_labels(tag):
    _, g, C, B = next(c for c in LOSS_CASES if c[0] == tag)
    seed = 2000 + 17 * [c[0] for c in LOSS_CASES].index(tag)
    counts = [3, 0, 5, 1, 4]
    lo, hi = (0.05, 0.6) if g != "m3_416" else (0.03, 0.5)
    labels = [random_labels(seed + b, counts[b] if g != "m3_416" else 6 + b, C, lo, hi) for b in range(B)]
    if g != "m3_416":
        labels[0] = crafted_labels(g)[:3] + labels[0]                   # ignore slots and overwrites take part in the loss
        for l in labels[0][:3]:
            l[4] = l[4] % C
    return labels


def loss_pred_maps(tag, gain=2.0):
    """one fp32 map [B, A(5+C), hs, ws] per level, uniform in [-gain, gain)"""
    _, g, C, B = next(c for c in LOSS_CASES if c[0] == tag)
    size, strides, anchors = GEOM[g]
    seed = 3000 + 31 * [c[0] for c in LOSS_CASES].index(tag)
    A = num_anchors(g)
    if is_multi(g):
        grids = [(size[0] // s, size[1] // s) for s in strides]
    else:
        grids = [(int(round(size[0] / strides)), int(round(size[1] / strides)))]
    return [synth.uniform_pm1(seed + l, (B, A * (5 + C), hs, ws)) * np.float32(gain) for l, (hs, ws) in enumerate(grids)]


def nan_case():
    """t64, C = 2, B = 1: tw = 127, th = -127 at anchor 0 of cell 0, an unassigned slot: the decoded area is inf * 0"""
    labels = [random_labels(4242, 3, 2)]
    pred = synth.uniform_pm1(4243, (1, 5 * 7, 4, 4)) * np.float32(2.0)
    pred[0, 5 * 3 + 2, 0, 0] = 127.0
    pred[0, 5 * 3 + 3, 0, 0] = -127.0
    return labels, [pred]


# the q_bf model case: 64 x 64, B = 2, two batches (the first calibrates, the second takes the EMA branch)
QBF = dict(size=[64, 64], classes=2, weights=dict(seed=2, pred_gain=400.0, obj_bias=-4.0), image_seeds=[51, 52], batch=2)


def qbf_labels(it):
    return [random_labels(5000 + 10 * it + b, 3 - b, 2) for b in range(2)]


def golden_bound(out, gap):
    """How far a float64-accumulating result may be from a golden loss: twice the recorded gap between the reference's fp32
    number and the restatement, and never looser than 1e-5 relative (terms are non-negative and carry a few fp32 ulps each)."""
    out, gap = np.asarray(out, np.float64), np.asarray(gap, np.float64)
    return np.minimum(2.0 * gap, 1e-5 * np.abs(out))


def assert_losses(got, out, gap, what):
    """got float64 [4] against a golden: same NaN pattern, finite entries within golden_bound"""
    got, out = np.asarray(got, np.float64), np.asarray(out, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(out)), (what, got, out)
    ok = ~np.isnan(out)
    err, bound = np.abs(got - out)[ok], golden_bound(out, gap)[ok]
    print(what, "err", err, "bound", bound)
    assert (err <= bound).all(), (what, got, out, err, bound)


def _ref():
    import loss_ref
    return loss_ref


def targets_match(got32, want64):
    """every field equal after .float(); tw / th within one fp32 ulp"""
    want = want64.astype(np.float32)
    exact = [0, 1, 2, 3, 6, 7, 8, 9, 10]
    assert np.array_equal(np.asarray(got32, np.float32)[..., exact], want[..., exact])
    d = np.abs(np.asarray(got32, np.float32)[..., 4:6].astype(np.float64) - want[..., 4:6].astype(np.float64))
    assert (d <= np.spacing(np.abs(want[..., 4:6])).astype(np.float64)).all(), d.max()


def restated_targets(tag, trace=None):
    size, strides, anchors = GEOM[tag]
    return _ref().make_targets(size, strides, target_labels(tag), anchors, is_multi(tag), trace=trace)


def check_case_properties(tag):
    """the label lists really exercise what they are meant to (asserted on the restatement)"""
    size, strides, anchors = GEOM[tag]
    labels = target_labels(tag)
    trace = []
    t = restated_targets(tag, trace)
    assert len(labels) == 3 and len(labels[1]) == 0 and len(labels[2]) == 70 and not t[1].any()
    st = [strides] if np.isscalar(strides) else list(strides)
    per_label = [_ref().label_writes(l, size, st, anchors, is_multi(tag)) for l in labels[0]]
    assert per_label[3] == [] and (labels[0][3][2] - labels[0][3][0]) * size[1] < 1          # narrower than one pixel
    kinds = {}
    for b, slot, kind in trace:
        if b == 0:
            kinds.setdefault(slot, []).append(kind)
    assert any(k[-2:] == [1, 1] for k in kinds.values() if len(k) > 1)                        # two boxes on one (cell, anchor)
    if tag != "m2":                 # (no box inside 64 x 64 passes 0.5 against two of the tiny-v3 anchors)
        assert sorted(f is None for *_, f in per_label[0]) == [False, True]                   # one positive, one ignore slot
        assert any(k[:2] == [0, 1] for k in kinds.values())                                   # positive over an earlier ignore
        assert any(k[-1] == 0 and 1 in k for k in kinds.values())                             # ignore over an earlier positive
        slot = next(s for s, k in kinds.items() if k[-1] == 0 and 1 in k)
        assert t[0, slot, 0] == -1 and t[0, slot, 6] == -1 and t[0, slot, 7:].any()           # keeps the positive's other fields
    later = next(s for s, k in kinds.items() if len(k) > 1 and k[-1] == 1)
    assert t[0, later, 1] == 1                                                              # the later box (class 1) won
