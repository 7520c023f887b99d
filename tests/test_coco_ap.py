"""COCO bbox AP on the GPU (yolo355.apeval.CocoEval, csrc/cocoeval.hip) against the literal restatement of the contract
(tests/coco_ap_ref.py, pinned by tests/test_coco_ap_ref.py).

Comparison rule of every test: the match tap, precision, recall (with their -1 entries) and CocoEval.compute()'s stats exactly
equal -- the same float64 operations in the same order, np.mean on both sides; the C ABI's own stats within N * 2^-52, N the number
of averaged entries -- the worst-case float64 error of a sum of N terms <= 1 taken in another association (a bound, not a
measurement)."""
import os
import subprocess

import numpy as np
import pytest

import coco_ap_ref as R
import voc_ap_ref as V
from test_coco_ap_ref import check_known, known

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _add_device(ev, first, boxes, scores, cls, count, stream=None):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes.astype(np.float32), scores.astype(np.float32),
                                                                    cls.astype(np.int32), count.astype(np.int32))]
    if stream is None:
        ev.add(first, *t)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ev.add(first, *t)
    return t                                              # kept alive by the caller until compute()


def _stats_bound(ev, ref):
    """the ABI's stats: in-order sums against np.mean, within N * 2^-52"""
    p, r = ref["precision"], ref["recall"]
    sel = [p[:, :, :, 0, 2], p[0:1, :, :, 0, 2], p[5:6, :, :, 0, 2], p[:, :, :, 1, 2], p[:, :, :, 2, 2], p[:, :, :, 3, 2],
           r[:, :, 0, 0], r[:, :, 0, 1], r[:, :, 0, 2], r[:, :, 1, 2], r[:, :, 2, 2], r[:, :, 3, 2]]
    for j, s in enumerate(sel):
        N = int((s > -1).sum())
        assert abs(ev.stats_abi[j] - ref["stats"][j]) <= N * 2.0 ** -52, (j, ev.stats_abi[j], ref["stats"][j], N)
        if N == 0:
            assert ev.stats_abi[j] == -1


def _compare(ev, ref, groups=None):
    """ev (computed) against the restatement's result; groups: the (image, k, a) keys to check through the tap (None: all; an int: every
    that many-th)"""
    assert np.array_equal(ev.precision, ref["precision"]), np.argwhere(ev.precision != ref["precision"])[:6]
    assert np.array_equal(ev.recall, ref["recall"]), np.argwhere(ev.recall != ref["recall"])[:6]
    assert np.array_equal(ev.stats, ref["stats"]), (ev.stats, ref["stats"])
    _stats_bound(ev, ref)
    keys = sorted(ref["matches"])
    for key in (keys if groups is None else keys[::groups] if isinstance(groups, int) else groups):
        want, got = ref["matches"][key], ev.matches(*key)
        for name in ("pos", "dtm", "dt_ig", "gt_marked"):
            assert np.array_equal(got[name], want[name]), (key, name, got[name], want[name])


def _run(C, gt, boxes, scores, cls, count, ids=None, groups=None):
    from yolo355.apeval import CocoEval
    ref = R.evaluate(C, gt, boxes, scores, cls, count, ids)
    ev = CocoEval(C, gt, image_ids=ids, max_dets=max(1, int(count.sum())))
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        ev.compute()
        _compare(ev, ref, groups)
        del keep
        return ev.stats, ref
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 1. known answers
@pytest.mark.parametrize("name", ("K1", "K2", "K3", "K4"))
def test_known_answers_through_cocoeval(name):
    from yolo355.apeval import CocoEval
    C, gt, boxes, scores, cls, count = known(name)
    ev = CocoEval(C, gt, max_dets=8)
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        stats = ev.compute()
        check_known(name, ev.precision, ev.recall, stats)
        _compare(ev, R.evaluate(C, gt, boxes, scores, cls, count))
        del keep
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 2. mixed set
def test_mixed_set_every_group_through_the_tap():
    """40 images, 3 categories (one unused), about 30 detections and 0 to 6 boxes per image; images without boxes, without
    detections, without both; 15 % crowd; areas in all ranges and on both borders; scores with 2 decimals; shuffled ids"""
    gt, boxes, scores, cls, count, ids = R.synth_set(11, 40, 3, 30, 6, used_classes=2)
    allg = np.concatenate(gt)
    assert len(gt[1]) == 0 and count[2] == 0 and len(gt[3]) == 0 and count[3] == 0 and count[1] > 0 and len(gt[2]) > 0
    assert (allg[:, 5] == 1024).any() and (allg[:, 5] == 9216).any() and 0.05 < allg[:, 6].mean() < 0.3
    assert all(((allg[:, 5] >= lo) & (allg[:, 5] <= hi)).any() for lo, hi in R.AREA_RNG[1:])
    assert not np.array_equal(np.argsort(ids), np.arange(40)) and len(np.unique(scores)) <= 101
    stats, ref = _run(3, gt, boxes, scores, cls, count, ids)
    assert stats[0] > 0.05 and np.all(ref["precision"][:, :, 2] == -1) and len(ref["matches"]) > 200
    assert any((m["dt_ig"] == 1).any() for m in ref["matches"].values())


# ---------------------------------------------------------------------------------------------------- 3. truncation, large groups
def test_truncation_and_groups_larger_than_two_wavefronts():
    """image 0: 130 detections and 150 boxes of one category, 20 % crowd (D > 100, G beyond two wavefronts and any LDS matrix);
    image 1: 100 detections exactly"""
    rng = np.random.default_rng(22)
    gts, dets = [], []
    for nb, nd in ((150, 130), (12, 100)):
        x, y = rng.integers(0, 560, nb), rng.integers(0, 400, nb)
        wh = np.array([R.SIZES[i] for i in rng.integers(0, len(R.SIZES), nb)])
        g = np.stack([np.zeros(nb), x, y, wh[:, 0], wh[:, 1], wh[:, 0] * wh[:, 1], rng.random(nb) < 0.2], 1).astype(np.float64)
        j = rng.integers(0, nb, nd)
        b = np.stack([g[j, 1], g[j, 2], g[j, 1] + g[j, 3], g[j, 2] + g[j, 4]], 1) + rng.normal(0, 1.5, (nd, 4)) * (rng.random((nd, 1)) < 0.7)
        gts.append(g)
        dets.append((b.astype(np.float32), np.round(rng.random(nd), 2).astype(np.float32), np.zeros(nd, np.int32)))
    boxes, scores, cls, count = R.pad(dets)
    assert count.tolist() == [130, 100] and gts[0][:, 6].sum() > 15
    stats, ref = _run(1, gts, boxes, scores, cls, count, ids=[9, 4])
    assert ref["matches"][0, 0, 0]["dtm"].shape == (10, 100) and ref["matches"][1, 0, 0]["dtm"].shape == (10, 100)
    assert stats[0] > 0.05


# ---------------------------------------------------------------------------------------------------- 4. sort across tiles
def test_sort_and_scans_over_several_tiles():
    """150 images, 2 categories, over 3 * 1024 detections and no multiple of 1024: the carry of the scans, the cross-tile order"""
    gt, boxes, scores, cls, count, ids = R.synth_set(21, 150, 2, 24, 4)
    n = int(count.sum())
    assert n > 3 * 1024 and n % 1024 != 0 and n < 5000, n
    stats, ref = _run(2, gt, boxes, scores, cls, count, ids, groups=37)
    assert stats[0] > 0.05 and len(ref["matches"]) > 37


# ---------------------------------------------------------------------------------------------------- 5. appending
def test_appending_in_any_order_reset_overflow_and_voc_on_the_same_handle():
    import torch
    from yolo355 import _ffi, apeval
    from yolo355.apeval import CocoEval
    gt, boxes, scores, cls, count, ids = R.synth_set(31, 30, 2, 14, 4)
    ref = R.evaluate(2, gt, boxes, scores, cls, count, ids)
    total = int(count.sum())
    ev = CocoEval(2, gt, image_ids=ids, max_dets=total)
    try:
        keep = [_add_device(ev, 0, boxes, scores, cls, count)]
        ev.compute()
        _compare(ev, ref, groups=11)
        # batches in reverse order, from two streams
        ev.reset()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        cuts = [0, 7, 8, 19, 30]
        for k in (3, 2, 1, 0):
            a, b = cuts[k], cuts[k + 1]
            keep.append(_add_device(ev, a, boxes[a:b], scores[a:b], cls[a:b], count[a:b], stream=streams[k % 2]))
        ev.compute()
        _compare(ev, ref, groups=11)
        # reset, then the same again from the host
        ev.reset()
        with pytest.raises(_ffi.Y355Error) as ei:
            ev.matches(0, 0, 0)
        assert ei.value.code == _ffi.ENOTREADY
        ev.add_host(0, boxes, scores, cls, count)
        ev.compute()
        _compare(ev, ref, groups=[])
        # VOC on the same handle, both ground truths set
        vgt = [np.concatenate([g[:, 0:1], g[:, 1:3], g[:, 1:3] + g[:, 3:5], g[:, 6:7]], 1) for g in gt]
        off, vb, vc, vd = apeval._gt_arrays(vgt, 2)
        _ffi.check(ev._lib.y355_apeval_set_gt(ev._h, off.ctypes.data, vb.ctypes.data, vc.ctypes.data, vd.ctypes.data))
        import ctypes as C
        ap, npos, ndet, mean = np.zeros(2), np.zeros(2, np.int32), np.zeros(2, np.int64), C.c_double()
        _ffi.check(ev._lib.y355_apeval_compute(ev._h, 0.5, _ffi.AP_VOC07, _ffi.AP_Q_VOCFILE, ap.ctypes.data, npos.ctypes.data, ndet.ctypes.data,
                                               C.byref(mean)))
        vref = V.evaluate(2, vgt, boxes, scores, cls, count, 0.5, True, True)
        assert np.array_equal(ap, vref["ap"]) and np.array_equal(npos, vref["npos"]) and np.array_equal(ndet, vref["ndet"])
        ev.compute()                                      # and COCO after VOC, still the same
        _compare(ev, ref, groups=11)
        ev.set_image_ids(None)                            # other ranks, the same store: the list order ...
        ev.compute()
        _compare(ev, R.evaluate(2, gt, boxes, scores, cls, count, None), groups=11)
        ev.set_image_ids(ids)                             # ... and back
        ev.compute()
        _compare(ev, ref, groups=[])
        del keep
    finally:
        ev.close()
    # overflow of max_dets: ERANGE, and a reset recovers
    ev = CocoEval(2, gt, image_ids=ids, max_dets=total - 5)
    try:
        keep = _add_device(ev, 0, boxes, scores, cls, count)
        with pytest.raises(_ffi.Y355Error) as ei:
            ev.compute()
        assert ei.value.code == _ffi.ERANGE and str(total) in str(ei.value) and str(total - 5) in str(ei.value)
        ev.reset()
        c20 = np.concatenate([count[:20], np.zeros(10, np.int32)])
        assert int(c20.sum()) <= total - 5
        keep2 = _add_device(ev, 0, boxes[:20], scores[:20], cls[:20], count[:20])
        ev.compute()
        _compare(ev, R.evaluate(2, gt, boxes, scores, cls, c20, ids), groups=[])
        del keep, keep2
    finally:
        ev.close()


# ---------------------------------------------------------------------------------------------------- 6. end to end
SIZES_HW = [(375, 500), (480, 640), (333, 500), (224, 320), (97, 131)]


class _RawSet:
    """pull_image(i) -> (img uint8 HWC BGR, id) like data/cocodataset.py:70-81"""

    def __init__(self, num_classes):
        from yolo355 import synth
        self.class_ids = [1 + 2 * k for k in range(num_classes)]
        self.imgs = [synth.make_frames_u8(300 + i, 1, h, w, "blocks")[0] for i, (h, w) in enumerate(SIZES_HW)]
        self.ids = [1000, 400, 700, 100, 1300]

    def __len__(self):
        return len(self.imgs)

    def pull_image(self, i):
        return self.imgs[i], self.ids[i]


def _instances(ds, data_dict, seed):
    """a COCO-style annotation dict made from a subset of the detections, jittered, some of it crowd"""
    rng = np.random.default_rng(seed)
    anns = []
    for d in data_dict:
        if rng.random() < 0.5:
            x, y, w, h = (float(np.rint(v)) for v in np.asarray(d["bbox"]) + rng.normal(0, 2.0, 4))
            w, h = max(w, 2.0), max(h, 2.0)
            anns.append(dict(id=len(anns) + 1, image_id=d["image_id"], category_id=d["category_id"], bbox=[x, y, w, h],
                             area=w * h * (1.0 if len(anns) % 2 else 0.75), iscrowd=int(rng.random() < 0.15)))
    return dict(images=[dict(id=i) for i in ds.ids], categories=[dict(id=c) for c in ds.class_ids], annotations=anns)


def _routes(net, C, monkeypatch, device_route, **kw):
    from yolo355 import apeval
    from yolo355.utils.evaluator_batch import coco_data_dict_frames, coco_ground_truth, coco_map, coco_stats_from_data_dict
    ds = _RawSet(C)
    ids, dd = coco_data_dict_frames(net, ds, batch_size=2, **kw)
    assert ids == ds.ids and len(dd) >= 10, len(dd)
    gt = coco_ground_truth(_instances(ds, dd, 7), ids, ds.class_ids)
    assert sum(len(g) for g in gt) >= 4
    calls = dict(add=0, add_detections=0)
    for name in calls:
        orig = getattr(apeval.ApStore, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            calls[_name] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(apeval.ApStore, name, spy)
    got = coco_map(net, ds, gt, batch_size=2, **kw)
    assert calls == (dict(add=3, add_detections=0) if device_route else dict(add=0, add_detections=3)), calls
    via = coco_stats_from_data_dict(ids, dd, gt, ds.class_ids)
    print("routes: detections", len(dd), "stats", got.stats[:3], via.stats[:3])
    assert tuple(got) == tuple(via) == (got.stats[0], got.stats[1]) and np.array_equal(got.stats, via.stats)
    assert np.array_equal(got.precision, via.precision) and np.array_equal(got.recall, via.recall)
    # and the restatement on the same data
    per = {i: ([], [], []) for i in ids}
    index = {c: k for k, c in enumerate(ds.class_ids)}
    for d in dd:
        x, y, w, h = d["bbox"]
        b, s, c = per[d["image_id"]]
        b.append([x, y, np.float32(x + w), np.float32(y + h)]), s.append(d["score"]), c.append(index[d["category_id"]])
    ref = R.evaluate(C, gt, *R.pad([(np.asarray(per[i][0], np.float32).reshape(-1, 4), np.asarray(per[i][1], np.float32),
                                     np.asarray(per[i][2], np.int32)) for i in ids]), ids)
    assert np.array_equal(got.precision, ref["precision"]) and np.array_equal(got.stats, ref["stats"])
    assert got.stats[0] > 0


def test_coco_map_device_route_of_a_calibrated_q_bf_model(monkeypatch):
    import torch
    from yolo355 import synth
    from test_dropin import _model
    C, size = 20, [416, 416]
    net = _model(synth.make_weights(seed=2, pred_gain=400.0, obj_bias=-4.0, num_classes=C), C, synth.ANCHOR_SIZE, size, 0.1, "cuda:0")
    net.forward_batch(torch.from_numpy(synth.make_images(51, 1, size[0], size[1], "blocks")), quantization=True)     # calibrates
    _routes(net, C, monkeypatch, True, quantization=True)


def test_coco_map_host_route_of_a_y355_net_family(monkeypatch):
    from test_net_frames import _model
    _routes(_model("tiny_yolo_v3", "cuda:0"), 3, monkeypatch, False)


# ---------------------------------------------------------------------------------------------------- 7. C client
def test_cocoeval_client_known_answers_from_c(tmp_path):
    from yolo355 import _ffi
    exe = str(tmp_path / "cocoeval_client")
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_client", "cocoeval_client.c"), "-o", exe, "-L", libdir, "-l:libyolo355.so",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == "ok cocoeval"
