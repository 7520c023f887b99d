"""VOC mAP on the GPU (yolo355.apeval.ApEval, csrc/apeval.hip) against the reference's own output (tests/golden/voc_ap.npz) and,
for everything larger, against the NumPy restatement that tests/test_voc_ap_ref.py pins to it bit for bit.

Comparison rule of every test: VOC07 ap, npos, ndet and curve() (flags, rec, prec) exactly equal; AREA ap within ndet * 2^-52 --
the worst-case float64 error of a sum of ndet terms <= 1 taken in another association (a bound, not a measurement)."""
import os

import numpy as np
import pytest

import voc_ap_ref as R
from test_voc_ap_ref import load_case, same, CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _add_device(ev, first, boxes, scores, cls, count):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes.astype(np.float32), scores.astype(np.float32),
                                                                    cls.astype(np.int32), count.astype(np.int32))]
    ev.add(first, *t)
    return t                                              # kept alive by the caller until compute()


def _compare(ev, C, gt, boxes, scores, cls, count, quantize=True, classes=None):
    """both metrics of ev (detections already added) against the restatement; -> the VOC07 result"""
    first = None
    for use07 in (True, False):
        aps, mean = ev.compute(0.5, use07, quantize)
        ref = R.evaluate(C, gt, boxes, scores, cls, count, 0.5, use07, quantize)
        assert np.array_equal(ev.npos, ref["npos"]) and np.array_equal(ev.ndet, ref["ndet"])
        if use07:
            assert same(aps, ref["ap"]), (aps, ref["ap"])
            assert mean == ref["mean"] or (np.isnan(mean) and np.isnan(ref["mean"]))
            first = (aps, mean)
        else:
            assert np.array_equal(np.isnan(aps), np.isnan(ref["ap"]))
            ok = ~np.isnan(aps)
            err = np.abs(aps[ok] - ref["ap"][ok])
            assert np.all(err <= ref["ndet"][ok] * 2.0 ** -52), (err.max(), aps, ref["ap"])
            assert np.array_equal(aps[ref["ndet"] == 0], np.full((ref["ndet"] == 0).sum(), -1.0))
        for c in (range(C) if classes is None else classes):
            rec, prec, flag = ev.curve(c)
            assert np.array_equal(flag, ref["flag"][c]), (c, np.flatnonzero(flag != ref["flag"][c])[:8])
            assert same(rec, ref["rec"][c]) and same(prec, ref["prec"][c]), c
    return first


def _run(C, gt, boxes, scores, cls, count, quantize=True, classes=None, max_dets=None):
    from yolo355.apeval import ApEval
    ev = ApEval(C, gt, max_dets=max_dets if max_dets is not None else max(1, int(count.sum())))
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        res = _compare(ev, C, gt, boxes, scores, cls, count, quantize, classes)
        del keep
        return res
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 1. the reference's own output
@pytest.mark.parametrize("name", CASES)
def test_golden_cases_through_apeval(name):
    from yolo355.apeval import ApEval
    with np.load(os.path.join(ROOT, "tests", "golden", "voc_ap.npz")) as z:
        g = {k: z[k] for k in z.files}
    C, gt, boxes, scores, cls, count = load_case(g, name)
    ev = ApEval(C, gt, max_dets=int(count.sum()))
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        aps, mean = ev.compute(0.5, True, True)
        assert same(aps, g[name + "/ap07"]), (aps, g[name + "/ap07"])
        assert mean == float(np.mean(g[name + "/ap07"]))
        for c in range(C):
            rec, prec, flag = ev.curve(c)
            assert same(rec, g["%s/rec/%d" % (name, c)]) and same(prec, g["%s/prec/%d" % (name, c)]), c
            assert len(flag) == ev.ndet[c]
        aps, _ = ev.compute(0.5, False, True)
        want = g[name + "/ap_area"]
        assert np.array_equal(np.isnan(aps), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.all(np.abs(aps[ok] - want[ok]) <= ev.ndet[ok] * 2.0 ** -52), (aps, want)
        del keep
        _compare(ev, C, gt, boxes, scores, cls, count)    # flags, npos, ndet: the restatement's
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 2. the kernels' own boundaries
def test_sort_over_several_tiles():
    """(i) 150 images, 2 classes, about 5000 detections: the 1024-key tiles of the radix sort -- at least 3 full ones and a partial one"""
    gt, boxes, scores, cls, count = R.synth_set(21, 150, 2, 34, 3)
    n = int(count.sum())
    assert n > 3 * 1024 and n % 1024 != 0 and n < 6000, n
    aps, mean = _run(2, gt, boxes, scores, cls, count)
    assert np.all(aps > 0.05)


def test_one_image_with_more_boxes_than_two_wavefronts():
    """(ii) one image, one class, 130 boxes, 200 detections"""
    rng = np.random.default_rng(22)
    nb, nd = 130, 200
    x1, y1 = rng.integers(0, 400, nb), rng.integers(0, 300, nb)
    g = np.stack([np.zeros(nb), x1, y1, x1 + rng.integers(8, 60, nb), y1 + rng.integers(8, 60, nb), rng.random(nb) < 0.2], 1).astype(np.float64)
    j = rng.integers(0, nb, nd)
    boxes = (g[j, 1:5] + rng.normal(0, 1.5, (nd, 4))).astype(np.float32)[None]
    scores = rng.random((1, nd)).astype(np.float32)
    aps, _ = _run(1, [g], boxes, scores, np.zeros((1, nd), np.int32), np.array([nd], np.int32))
    assert aps[0] > 0.2


def test_tie_groups_across_images_and_workgroups():
    """(iii) scores with 2 decimals: at most 101 values for about 2500 detections per class -- the tie rule (image, then position)"""
    gt, boxes, scores, cls, count = R.synth_set(23, 150, 2, 34, 3, score_decimals=2)
    img, pos, dcls, dsc, _ = R.flatten(boxes, scores, cls, count)
    assert len(np.unique(dsc)) <= 101 and len(dsc) > 4096
    _run(2, gt, boxes, scores, cls, count)


def test_raw_float32_values():
    """(iv) quantize=False: no rounding, no + 1"""
    gt, boxes, scores, cls, count = R.synth_set(24, 40, 3, 30, 3)
    got = _run(3, gt, boxes, scores, cls, count, quantize=False)
    ref_q = R.evaluate(3, gt, boxes, scores, cls, count, 0.5, True, True)
    assert not np.array_equal(got[0], ref_q["ap"])        # the two modes are different numbers on this set


def test_256_classes_most_of_them_empty():
    """(v)"""
    gt, boxes, scores, cls, count = R.synth_set(25, 30, 256, 25, 3, used_classes=6)
    lut = np.array([0, 7, 100, 200, 254, 255])
    cls = lut[cls].astype(np.int32)
    for g in gt:
        g[:, 0] = lut[g[:, 0].astype(np.int64)]
    aps, mean = _run(256, gt, boxes, scores, cls, count, classes=[0, 1, 7, 100, 199, 200, 254, 255])
    assert (aps == -1.0).sum() == 250 and np.all(aps[lut] >= 0)


# ---------------------------------------------------------------------------------------------------- 3. batches
def test_batches_in_any_order_and_from_the_host_give_the_same_result():
    from yolo355.apeval import ApEval
    gt, boxes, scores, cls, count = R.synth_set(31, 61, 3, 20, 3, score_decimals=2)
    N, md = scores.shape
    # what lies behind count[b] must not matter: NaN, huge values, classes out of range
    dead = np.arange(md)[None, :] >= count[:, None]
    assert dead.any()
    boxes, scores, cls = boxes.copy(), scores.copy(), cls.copy()
    boxes[dead] = np.nan
    scores[dead] = np.where(np.arange(dead.sum()) % 2, np.float32(3e38), np.float32(np.nan))
    cls[dead] = np.where(np.arange(dead.sum()) % 2, 1000, -5)
    total = int(count.sum())
    results = []
    for how in ("one", "ragged", "host"):
        ev = ApEval(3, gt, max_dets=total)
        keep = []
        try:
            if how == "one":
                keep.append(_add_device(ev, 0, boxes, scores, cls, count))
            elif how == "host":
                ev.add_host(0, boxes, scores, cls, count)
            else:
                cuts = [0, 1, 12, 13, 30, 41, 56, N]      # 7 ragged batches, each with its own max_det, in shuffled order
                for k in np.random.default_rng(3).permutation(7):
                    a, b = cuts[k], cuts[k + 1]
                    m = min(md, int(count[a:b].max()) + int(k))
                    keep.append(_add_device(ev, a, boxes[a:b, :max(m, 1)], scores[a:b, :max(m, 1)], cls[a:b, :max(m, 1)], count[a:b]))
            r = {}
            for use07 in (True, False):
                aps, mean = ev.compute(0.5, use07, True)
                r[use07] = (aps, mean, [ev.curve(c) for c in range(3)], ev.ndet.copy())
            if how == "one":
                _compare(ev, 3, gt, boxes, scores, cls, count)
            results.append(r)
        finally:
            ev.close()
    for r in results[1:]:
        for use07 in (True, False):
            a, b = results[0][use07], r[use07]
            assert same(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[3], b[3])
            for (r0, p0, f0), (r1, p1, f1) in zip(a[2], b[2]):
                assert same(r0, r1) and same(p0, p1) and np.array_equal(f0, f1)


# ---------------------------------------------------------------------------------------------------- 4. capacity
def test_capacity_and_class_range_are_reported_by_compute():
    from yolo355 import _ffi
    from yolo355.apeval import ApEval
    gt, boxes, scores, cls, count = R.synth_set(41, 20, 2, 12, 3)
    total = int(count.sum())
    ev = ApEval(2, gt, max_dets=total - 7)
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        with pytest.raises(_ffi.Y355Error) as ei:
            ev.compute()
        assert ei.value.code == _ffi.ERANGE and str(total) in str(ei.value) and str(total - 7) in str(ei.value)
        with pytest.raises(_ffi.Y355Error):               # still so until reset
            ev.compute()
        ev.reset()
        keep2 = _add_device(ev, 0, boxes[:15], scores[:15], cls[:15], count[:15])
        assert int(count[:15].sum()) <= total - 7
        c15 = np.concatenate([count[:15], np.zeros(5, np.int32)])
        _compare(ev, 2, gt, boxes, scores, cls, c15)
        # a class index outside 0 .. C - 1 inside count
        ev.reset()
        bad = cls.copy()
        bad[3, 0] = 2
        assert count[3] > 0
        keep3 = _add_device(ev, 0, boxes[:15], scores[:15], bad[:15], count[:15])
        with pytest.raises(_ffi.Y355Error) as ei:
            ev.compute()
        assert ei.value.code == _ffi.ERANGE and "class" in str(ei.value)
        ev.reset()
        keep4 = _add_device(ev, 0, boxes[:15], scores[:15], cls[:15], count[:15])
        _compare(ev, 2, gt, boxes, scores, cls, c15)
        del keep, keep2, keep3, keep4
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 5. routes
EVAL = dict(weights=dict(seed=2, pred_gain=400.0, obj_bias=-4.0), size=[240, 320], classes=20, seeds=[51, 52, 53, 54, 59],
            sizes=[(640, 480), (500, 375), (333, 500), (1280, 720), (320, 240)], conf=0.1)      # mirrors gen_golden_r2.py


class _VocSet:
    def __init__(self, x, sizes):
        self.x, self.sizes = x, sizes

    def __len__(self):
        return len(self.x)

    def pull_item(self, i):
        import torch
        return torch.from_numpy(self.x[i]), None, self.sizes[i][1], self.sizes[i][0]


def _gt_from(all_boxes, seed):
    """ground truth made from a subset of the detections, jittered, some of it difficult"""
    rng = np.random.default_rng(seed)
    C, n = len(all_boxes), len(all_boxes[0])
    gt = []
    for i in range(n):
        rows = []
        for j in range(C):
            for d in np.asarray(all_boxes[j][i], np.float32).reshape(-1, 5):
                if rng.random() < 0.5:
                    rows.append([j] + list(np.rint(d[:4] + rng.normal(0, 2.0, 4))) + [rng.random() < 0.2])
        gt.append(np.asarray(rows, np.float64).reshape(-1, 6))
    return gt


def _routes(net, x, sizes, C, monkeypatch, device_route, **kw):
    from yolo355 import apeval
    from yolo355.utils.evaluator_batch import voc_all_boxes, voc_map, voc_map_from_all_boxes
    ds = _VocSet(x, sizes)
    all_boxes = voc_all_boxes(net, ds, C, batch_size=2, **kw)            # also calibrates a fresh q_bf model on image 0
    ndet = sum(len(a) for row in all_boxes for a in row)
    assert ndet >= 10, ndet
    gt = _gt_from(all_boxes, 7)
    calls = dict(add=0, add_detections=0)
    for name in calls:
        orig = getattr(apeval.ApEval, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(apeval.ApEval, name, spy)
    got = voc_map(net, ds, C, gt, batch_size=2, **kw)
    if device_route:
        assert calls == dict(add=3, add_detections=0), calls
    else:
        assert calls["add"] == 0 and calls["add_detections"] == 3, calls
    via = voc_map_from_all_boxes(all_boxes, gt)
    ref = R.evaluate(C, gt, *R.all_boxes_to_padded(all_boxes), 0.5, True, True)
    print("routes: detections", ndet, "mean", got[1], via[1], ref["mean"])
    assert same(got[0], via[0]) and got[1] == via[1]
    assert same(got[0], ref["ap"]) and got[1] == ref["mean"]
    assert (ref["ap"] > 0).any()
    got_a = voc_map(net, ds, C, gt, batch_size=2, use_07_metric=False, **kw)
    via_a = voc_map_from_all_boxes(all_boxes, gt, use_07_metric=False)
    assert same(got_a[0], via_a[0])


def _qbf_model():
    from yolo355 import synth
    from test_dropin import _model
    cfg = EVAL
    x = np.concatenate([synth.make_images(s, 1, cfg["size"][0], cfg["size"][1], "blocks") for s in cfg["seeds"]])
    net = _model(synth.make_weights(**cfg["weights"], num_classes=cfg["classes"]), cfg["classes"], synth.ANCHOR_SIZE, cfg["size"],
                 cfg["conf"], "cuda:0")
    return net, x


def test_voc_map_device_route_of_a_calibrated_q_bf_model(monkeypatch):
    net, x = _qbf_model()
    _routes(net, x, EVAL["sizes"], EVAL["classes"], monkeypatch, True, quantization=True)


def test_voc_map_host_route_without_quantization(monkeypatch):
    net, x = _qbf_model()
    _routes(net, x, EVAL["sizes"], EVAL["classes"], monkeypatch, False, quantization=False)


def test_voc_map_host_route_of_a_y355_net_family(monkeypatch):
    from yolo355 import synth
    from yolo355.models.tiny_yolo_v3 import YOLOv3tiny
    from cases import synth_state_dict
    size = [224, 320]
    m = YOLOv3tiny("cuda:0", input_size=size, num_classes=20, trainable=False, conf_thresh=0.02, nms_thresh=0.5,
                   anchor_size=synth.TINY_MULTI_ANCHOR_SIZE)
    m.load_state_dict(synth_state_dict(m.state_dict(), 5, weight_gain=2.0))
    m.eval()
    x = np.concatenate([synth.make_images(s, 1, size[0], size[1], "blocks") for s in EVAL["seeds"]])
    _routes(m, x, EVAL["sizes"], 20, monkeypatch, False)
