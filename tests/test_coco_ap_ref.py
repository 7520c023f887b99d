"""COCO AP without a GPU: the literal restatement of the contract (tests/coco_ap_ref.py, the oracle of tests/test_coco_ap.py)
against known answers worked out by hand, its properties, pycocotools itself wherever that package exists, the annotation reader,
and the argument checks of the COCO part of the y355_apeval_* C ABI from a plain C program."""
import json
import os
import subprocess

import numpy as np
import pytest

import coco_ap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
assert P == 0.9999999999999998


def known(name):
    """-> (num_classes, ground_truth, boxes, scores, cls, count) of the known-answer cases K1 .. K4: one image, one category"""
    box = [0, 10, 10, 50, 50, 2500, 0]
    d1 = ([10, 10, 60, 60], .9)
    gt, dt = {
        "K1": ([box], [d1]),
        "K2": ([box, [0, 200, 200, 50, 50, 2500, 0]], [d1, ([300, 10, 340, 50], .8)]),
        "K3": ([box, [0, 100, 100, 200, 200, 40000, 1]], [d1, ([120, 120, 160, 160], .95), ([150, 150, 190, 190], .5)]),
        "K4": ([[0, 0, 0, 10, 20, 200, 0]], [([0, 0, 10, 10], .9)]),
    }[name]
    dets = [(np.array([d[0] for d in dt], np.float32), np.array([d[1] for d in dt], np.float32), np.zeros(len(dt), np.int32))]
    return (1, [np.asarray(gt, np.float64)]) + R.pad(dets)


def check_known(name, precision, recall, stats):
    """the expected values of the issue's table, for any producer of the three arrays"""
    mean = lambda n: float(np.mean(np.full(n, P)))        # noqa: E731  np.mean of an array of p
    if name in ("K1", "K3"):
        for a in (0, 2):
            assert np.all(precision[:, :, 0, a, 2] == P) and np.all(precision[:, :, 0, a, 1] == P)
        assert np.all(precision[:, :, 0, (1, 3), :] == -1) and np.all(recall[:, 0, (1, 3), :] == -1)
        ar1 = 1.0 if name == "K1" else 0.0                # K3: the top detection is the ignored one
        assert np.all(recall[:, 0, (0, 2), 1:] == 1) and np.all(recall[:, 0, (0, 2), 0] == ar1)
        assert np.all(precision[:, :, 0, 0, 0] == (P if name == "K1" else 0.0))
        want = [mean(1010), mean(101), mean(101), -1, mean(1010), -1, ar1, 1, 1, -1, 1, -1]
        assert stats.tolist() == want, (stats.tolist(), want)
    elif name == "K2":
        assert np.all(precision[:, :51, 0, 0, 2] == P) and np.all(precision[:, 51:, 0, 0, 2] == 0)
        ap = float(np.mean(np.concatenate([np.full(51, P), np.zeros(50)])))
        assert abs(ap - 51 * P / 101) <= 101 * 2.0 ** -52 and abs(ap - 0.5049504950495048) < 1e-15
        assert stats[1] == ap and stats[2] == ap and abs(stats[0] - ap) <= 1010 * 2.0 ** -52
        assert stats[6:9].tolist() == [0.5, 0.5, 0.5] and np.all(recall[:, 0, 0, :] == 0.5)
    else:
        assert recall[:, 0, 0, 2].tolist() == [1] + [0] * 9 and recall[:, 0, 1, 2].tolist() == [1] + [0] * 9
        assert np.all(recall[:, 0, 2:, :] == -1)          # area 200: the small range only
        assert np.all(precision[0, :, 0, 0, 2] == P) and np.all(precision[1:, :, 0, 0, 2] == 0)
        assert stats[1] == float(np.mean(np.full(101, P))) and stats[2] == 0.0 and abs(stats[0] - 0.1) < 1e-15
        assert stats[3] == stats[0] and stats[4] == -1 and stats[5] == -1


@pytest.mark.parametrize("name", ("K1", "K2", "K3", "K4"))
def test_known_answers(name):
    ref = R.evaluate(*known(name))
    check_known(name, ref["precision"], ref["recall"], ref["stats"])
    if name == "K3":
        m = ref["matches"][0, 0, 0]
        assert m["pos"].tolist() == [1, 0, 2]             # score order
        assert np.all(m["dtm"] == [1, 0, 1]) and np.all(m["dt_ig"] == [1, 0, 1]) and np.all(m["gt_marked"] == 1)
    if name == "K4":
        assert ref["matches"][0, 0, 0]["dtm"][:, 0].tolist() == [0] + [-1] * 9


def _same(a, b):
    for k in ("precision", "recall", "stats", "npig"):
        assert np.array_equal(a[k], b[k]), k


def test_order_of_the_image_list_does_not_matter_given_the_ids():
    gt, boxes, scores, cls, count, ids = R.synth_set(3, 12, 2, 8, 3)
    ref = R.evaluate(2, gt, boxes, scores, cls, count, ids)
    p = np.random.default_rng(1).permutation(12)
    got = R.evaluate(2, [gt[i] for i in p], boxes[p], scores[p], cls[p], count[p], ids[p])
    _same(ref, got)
    other = R.evaluate(2, gt, boxes, scores, cls, count, None)      # other ranks: ties across images fall the other way
    assert other["precision"].shape == ref["precision"].shape


def test_area_exactly_1024_is_small_and_medium():
    gt = [np.array([[0, 10, 10, 32, 32, 1024, 0]], np.float64)]
    dets = R.pad([(np.array([[10, 10, 42, 42]], np.float32), np.array([.9], np.float32), np.zeros(1, np.int32))])
    ref = R.evaluate(1, gt, *dets)
    assert np.all(ref["recall"][:, 0, (0, 1, 2), 2] == 1) and np.all(ref["recall"][:, 0, 3, :] == -1)
    assert ref["npig"].tolist() == [[1, 1, 1, 0]]
    gt[0][0, 5] = 9216                                    # and 96 * 96 is medium and large
    assert R.evaluate(1, gt, *dets)["npig"].tolist() == [[1, 0, 1, 1]]


def test_the_101st_detection_of_a_group_cannot_matter():
    rng = np.random.default_rng(8)
    g = np.array([[0, 20 * j, 15 * j, 40, 40, 1600, 0] for j in range(20)], np.float64)
    j = rng.integers(0, 20, 130)
    b = np.stack([g[j, 1], g[j, 2], g[j, 1] + 40, g[j, 2] + 40], 1) + rng.normal(0, 2, (130, 4))
    s = rng.permutation(130).astype(np.float32) / 200 + 0.1          # distinct scores
    a = R.evaluate(1, [g], *R.pad([(b, s, np.zeros(130, np.int32))]))
    assert a["matches"][0, 0, 0]["dtm"].shape == (10, 100)
    top = np.argsort(-s, kind="mergesort")
    b2, s2 = b.copy(), s.copy()
    b2[top[100:]] = (0, 0, 40, 40)                        # perfect matches of box 0, all behind the cut
    keep = np.sort(top[:100])
    _same(a, R.evaluate(1, [g], *R.pad([(b2, s2, np.zeros(130, np.int32))])))
    _same(a, R.evaluate(1, [g], *R.pad([(b[keep], s[keep], np.zeros(100, np.int32))])))


def test_equal_iou_against_two_boxes_picks_the_later_one():
    gt = [np.array([[0, 10, 10, 40, 40, 1600, 0], [0, 10, 10, 40, 40, 1600, 0], [0, 10, 10, 40, 40, 1600, 0]], np.float64)]
    dets = R.pad([(np.array([[10, 10, 50, 50], [10, 10, 50, 50]], np.float32), np.array([.9, .8], np.float32), np.zeros(2, np.int32))])
    m = R.evaluate(1, gt, *dets)["matches"][0, 0, 0]
    assert np.all(m["dtm"][:, 0] == 2) and np.all(m["dtm"][:, 1] == 1) and np.all(m["gt_marked"] == [0, 1, 1])


def coco_dicts(num_classes, gt, boxes, scores, cls, count, ids):
    """the synthetic set as an instances_*.json dict (category ids 1 + 2 k) and the reference's data_dict"""
    class_ids = [1 + 2 * k for k in range(num_classes)]
    anns, data = [], []
    for i, g in enumerate(gt):
        for r in g:
            anns.append(dict(id=len(anns) + 1, image_id=int(ids[i]), category_id=class_ids[int(r[0])], bbox=[float(v) for v in r[1:5]],
                             area=float(r[5]), iscrowd=int(r[6])))
        for p in range(int(count[i])):
            x1, y1, x2, y2 = (float(v) for v in boxes[i, p])
            data.append({"image_id": int(ids[i]), "category_id": class_ids[int(cls[i, p])], "bbox": [x1, y1, x2 - x1, y2 - y1],
                         "score": float(scores[i, p])})
    inst = dict(images=[dict(id=int(v)) for v in ids], categories=[dict(id=c) for c in class_ids], annotations=anns)
    return inst, data, class_ids


def test_restatement_equals_pycocotools():
    pytest.importorskip("pycocotools")
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    for seed, n, C in ((11, 40, 3), (12, 25, 2)):
        gt, boxes, scores, cls, count, ids = R.synth_set(seed, n, C, 30, 6, used_classes=max(1, C - 1))
        inst, data, class_ids = coco_dicts(C, gt, boxes, scores, cls, count, ids)
        g = COCO()
        g.dataset = inst
        g.createIndex()
        E = COCOeval(g, g.loadRes(data), "bbox")
        E.params.imgIds = [int(v) for v in ids]
        E.evaluate()
        E.accumulate()
        E.summarize()
        ref = R.evaluate(C, gt, boxes, scores, cls, count, ids)
        assert np.array_equal(E.eval["precision"], ref["precision"]) and np.array_equal(E.eval["recall"], ref["recall"])
        assert np.array_equal(E.stats, ref["stats"])


def test_coco_ground_truth_reads_an_instances_file(tmp_path):
    from yolo355.utils.evaluator_batch import coco_ground_truth
    gt, boxes, scores, cls, count, ids = R.synth_set(5, 6, 3, 4, 4)
    inst, _, class_ids = coco_dicts(3, gt, boxes, scores, cls, count, ids)
    inst["annotations"].append(dict(id=10 ** 6, image_id=int(ids[0]), category_id=2, bbox=[1, 2, 3, 4], area=12.0, iscrowd=0))   # no such class
    path = tmp_path / "instances.json"
    path.write_text(json.dumps(inst))
    for src in (str(path), inst):
        got = coco_ground_truth(src, [int(v) for v in ids], class_ids)
        assert len(got) == 6
        for a, b in zip(got, gt):
            assert a.dtype == np.float64 and np.array_equal(a, b.reshape(-1, 7))


def test_coco_eval_and_its_prototypes_exist():
    from yolo355 import _ffi, apeval
    names = ["y355_apeval_" + n for n in ("set_gt_coco", "compute_coco", "coco_matches")]
    declared = _ffi.declared_symbols()
    lib = _ffi.lib()
    for n in names:
        assert n in declared and n in _ffi._SIGS and hasattr(lib, n), n
    assert issubclass(apeval.CocoEval, apeval.ApStore) and issubclass(apeval.ApEval, apeval.ApStore)
    for name in ("add", "add_host", "add_detections", "reset"):    # one copy, on the base
        assert name in vars(apeval.ApStore) and name not in vars(apeval.CocoEval) and name not in vars(apeval.ApEval)
    assert apeval.CocoEval._destroy == "y355_apeval_destroy"
    assert np.array_equal(apeval.COCO_IOU_THRS, R.IOU_THRS) and np.array_equal(apeval.COCO_REC_THRS, R.REC_THRS)
    assert list(apeval.COCO_MAX_DETS) == R.MAX_DETS and np.array_equal(np.asarray(apeval.COCO_AREA_RNG, np.float64), np.asarray(R.AREA_RNG, np.float64))


def test_coco_eval_rejects_duplicate_image_ids_and_bad_rows():
    from yolo355.apeval import coco_gt_arrays, image_ranks
    assert image_ranks([30, 10, 20]).tolist() == [2, 0, 1] and image_ranks(None, 3).tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match="duplicate"):
        image_ranks([3, 1, 3])
    with pytest.raises(ValueError, match="class"):
        coco_gt_arrays([np.array([[2, 0, 0, 1, 1, 1, 0]], np.float64)], 2)
    off, box, area, cls, crowd = coco_gt_arrays([np.zeros((0, 7)), np.array([[1, 1, 2, 3, 4, 11.5, 1]], np.float64)], 2)
    assert off.tolist() == [0, 0, 1] and box.tolist() == [[1, 2, 3, 4]] and area.tolist() == [11.5] and cls.tolist() == [1] and crowd.tolist() == [1]
    assert box.dtype == np.float64 and area.dtype == np.float64 and cls.dtype == np.int32 and crowd.dtype == np.uint8


def test_cocoeval_argument_checks_from_a_c_program(tmp_path):
    """tests/c_client/cocoeval_client.c: the COCO entry points linked from C99, every argument check answered before any HIP call
    (so it passes without a GPU; with one, the known answers K1 .. K3 run too)"""
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
    assert r.stdout.startswith("ok cocoeval")
