"""The host restatement of the anchor fit (tests/anchors_ref.py) against the reference's own results
(tests/golden/anchors.npz, tests/golden/gen_golden_anchors.py), and the surface of the companion library: header, exports and
ctypes signatures agree, the header is C99, libyolo355.so and include/yolo355.h know nothing of it, arguments are refused
before any HIP call, and the host-side helpers of yolo355/anchors.py.  No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import anchors_cases as AC
import anchors_ref as R
from yolo355 import _ffi, anchors as A

ROOT = AC.ROOT


@pytest.fixture(scope="module")
def gold():
    return AC.load_golden()


@pytest.mark.parametrize("tag", AC.TAGS)
def test_restatement_equals_the_reference(gold, tag):
    c = AC.case(tag)
    g = {k: gold["%s/%s" % (tag, k)] for k in ("init", "nfound", "first", "u", "losses", "anchors", "groups", "iterations", "margins")}
    got = R.fit(c["wh"], c["k"], first=int(g["first"][0]), u=g["u"], init_index=c["init_index"], iters=c["iters"], convergence=AC.CONVERGENCE)
    assert np.array_equal(got["init"], g["init"])
    assert got["iterations"] == int(g["iterations"][0])
    assert np.array_equal(got["losses"], g["losses"]) and got["loss"] == g["losses"][-1]
    assert np.array_equal(got["anchors"], g["anchors"])
    assert np.array_equal(got["groups"], g["groups"])
    assert np.array_equal(got["counts"], np.bincount(g["groups"], minlength=c["k"]))
    # the margins with which the reference decided every discrete outcome
    assert g["margins"][0] > 1e-9 and g["margins"][1] > 4 * AC.loss_bound(c["n"]) and g["margins"][2] > 1e-9


def test_cases_are_the_shapes_they_claim(gold):
    assert A.CHUNK == AC.CHUNK and AC.case("n4097_k9")["n"] == 4 * AC.CHUNK + 1
    it = {t: int(gold[t + "/iterations"][0]) for t in AC.TAGS}
    assert it["n1500_k5_iters3"] == 4 < it["n1500_k5"]                       # the cap is hit before convergence
    assert it["n4097_k9"] > 16                                               # several groups of queued iterations
    four = gold["four_dup_k6/anchors"]
    assert (four[[1, 3, 5]] == 0).all() and (four[[0, 2, 4]] > 0).all()      # empty groups became (0, 0)
    assert set(np.unique(gold["four_dup_k6/groups"])) == {0, 2, 4}           # the lowest index won every tie
    assert int(gold["same8_k3/nfound"][0]) == 1 and (gold["same8_k3/init"][1:] == 0).all()
    assert np.array_equal(gold["same8_k3/anchors"][0], AC.boxes("same8")[0]) and (gold["same8_k3/anchors"][1:] == 0).all()


@pytest.mark.parametrize("tag", [t for t in AC.TAGS if AC.CASES[t].get("seed") is not None])
def test_same_seed_draws_equal_the_reference(gold, tag):
    c = AC.case(tag)
    first, u = A.draws(c["n"], c["k"], c["seed"], restarts=2)
    assert first.dtype == np.int32 and u.shape == (2, c["k"] - 1)
    assert first[0] == gold[tag + "/first"][0] and np.array_equal(u[0], gold[tag + "/u"])
    f1, u1 = A.draws(c["n"], c["k"], c["seed"] + 1)                          # restart r draws from seed + r
    assert first[1] == f1[0] and np.array_equal(u[1], u1[0])


def test_sample_indices_are_the_reference_sampling():
    import random
    random.seed(11)
    want = random.sample(range(300), 5)
    got = A.sample_indices(300, 5, 11, restarts=2)
    assert got.shape == (2, 5) and got[0].tolist() == want and got[1].tolist() == random.Random(12).sample(range(300), 5)


# ------------------------------------------------------------------------------------------------ the library's surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("y355"))


def test_header_library_and_signatures_agree():
    names = A.declared_symbols()
    assert set(names) == set(A._SIGS) and "y355_anchors_fit" in names and "y355_anchors_score" in names
    assert _exports(A.LIB_PATH) == names
    lib = A.lib()
    for n in names:
        assert hasattr(lib, n)
    text = open(A.HEADER_PATH).read()
    import re
    consts = {n: int(eval(re.search(r"#define Y355_ANCHORS_%s (\S+)" % n, text).group(1).strip("()"))) for n in ("MAX_K", "MAX_RESTARTS", "CHUNK")}
    assert (A.MAX_K, A.MAX_RESTARTS, A.CHUNK) == (consts["MAX_K"], consts["MAX_RESTARTS"], consts["CHUNK"])
    assert lib.y355_anchors_chunk() == A.CHUNK


def test_header_is_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "yolo355_anchors.h"\nint main(void) {\n  y355_anchors *h = 0;\n  (void)h;\n'
                   "  return Y355_ANCHORS_CHUNK == 1024 && Y355_ANCHORS_MAX_K == 16 ? 0 : 1;\n}\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-c",
                        str(src), "-o", str(tmp_path / "use_cc.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_main_library_knows_nothing_of_it():
    assert not [n for n in _exports(_ffi.LIB_PATH) if n.startswith("y355_anchors")]
    assert not [n for n in _ffi._SIGS if n.startswith("y355_anchors")] and not [n for n in _ffi.declared_symbols() if n.startswith("y355_anchors")]
    text = open(_ffi.HEADER_PATH).read().lower()
    assert "y355_anchors" not in text and "yolo355_anchors" not in text and "kmeans" not in text
    from yolo355 import loss
    assert not [n for n in _exports(loss.LIB_PATH) if n.startswith("y355_anchors")]


@pytest.mark.parametrize("args,text", [((-1, 10, 1, 4), "device_id"), ((0, 0, 1, 4), "max_boxes"), ((0, (1 << 28) + 1, 1, 4), "max_boxes"),
                                       ((0, 10, 0, 4), "max_restarts"), ((0, 10, 65, 4), "max_restarts"), ((0, 10, 1, 0), "max_k"),
                                       ((0, 10, 1, 17), "max_k")])
def test_create_refuses_bad_arguments_before_any_hip_call(args, text):
    lib = A.lib()
    h = ctypes.c_void_p()
    assert lib.y355_anchors_create(*args, ctypes.byref(h)) == -1 and not h.value
    assert text in lib.y355_anchors_last_error().decode()


def test_null_arguments_are_refused():
    lib = A.lib()
    one = (ctypes.c_double * 2)(1.0, 1.0)
    i32 = (ctypes.c_int32 * 1)(0)
    m = ctypes.c_double(0.0)
    for call, text in ((lambda: lib.y355_anchors_create(0, 10, 1, 4, None), "null out"),
                       (lambda: lib.y355_anchors_set_boxes(None, one, 1), "set_boxes: null"),
                       (lambda: lib.y355_anchors_set_boxes_dev(None, None, 1, None), "set_boxes_dev: null"),
                       (lambda: lib.y355_anchors_fit(None, 1, 1, 10, 1e-6, i32, None, None, None), "fit: null handle"),
                       (lambda: lib.y355_anchors_get_result(None, None, None, None, None, None, None), "get_result: null handle"),
                       (lambda: lib.y355_anchors_assignments(None, 0, i32), "assignments: null"),
                       (lambda: lib.y355_anchors_score(None, one, 1, ctypes.byref(m), i32, None), "score: null")):
        assert call() == -1 and text in lib.y355_anchors_last_error().decode(), text
    assert lib.y355_anchors_num_boxes(None) == -1
    lib.y355_anchors_destroy(None)


# ------------------------------------------------------------------------------------------------ the host-side helpers
def test_boxes_from_annotations_is_the_reference_statement():
    rows = [[10, 20, 110, 220], [0, 0, 3, 400], [5, 5, 5.5, 100], [100, 50, 300, 375]]
    sizes = [[500, 375], [500, 375], [640, 480], [353, 500]]
    got = A.boxes_from_annotations(rows, sizes, 416)
    want = []
    for (xmin, ymin, xmax, ymax), (w, h) in zip(rows, sizes):
        bw = (xmax - xmin) / w * 416
        bh = (ymax - ymin) / h * 416
        if bw < 1.0 or bh < 1.0:
            continue
        want.append([bw, bh])
    assert len(want) == 3 and got.dtype == np.float64 and np.array_equal(got, np.array(want))     # 0.5 / 640 * 416 < 1: dropped
    assert A.boxes_from_annotations(np.zeros((0, 4)), np.zeros((0, 2)), 416).shape == (0, 2)


def test_unit_conversions():
    px = np.array([[330.24, 340.8], [38.08, 63.36], [257.92, 169.28], [89.28, 146.88], [144.96, 285.44], [20.0, 400.0]])
    assert np.array_equal(A.to_grid_units(px, 32), px / 32.0)
    s = A.sort_by_area(px)
    assert np.array_equal(s, px[[1, 5, 3, 4, 2, 0]]) and (np.diff(s[:, 0] * s[:, 1]) >= 0).all()
    lv = A.split_levels(px, 3)
    assert lv.shape == (3, 2, 2) and np.array_equal(lv.reshape(-1, 2), s) and np.array_equal(A.split_levels(px, 2)[1], s[3:])
    with pytest.raises(ValueError):
        A.split_levels(px, 4)
    tie = np.array([[4.0, 2.0], [2.0, 4.0], [1.0, 1.0]])
    assert np.array_equal(A.sort_by_area(tie), tie[[2, 0, 1]])                                     # equal areas keep their order


def test_voc_and_coco_boxes(tmp_path):
    xml = ("<annotation><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>a</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
           "<object><name>b</name><bndbox><xmin>7</xmin><ymin>9</ymin><xmax>8</xmax><ymax>200</ymax></bndbox></object></annotation>")
    (tmp_path / "a.xml").write_text(xml % (500, 375, 49, 100, 250, 300))
    (tmp_path / "b.xml").write_text(xml % (320, 480, 1, 1, 320, 480))
    got = A.voc_boxes(str(tmp_path / "%s.xml"), ["a", "b"], 416)
    want = A.boxes_from_annotations([[48, 99, 249, 299], [6, 8, 7, 199], [0, 0, 319, 479], [6, 8, 7, 199]],
                                    [[500, 375], [500, 375], [320, 480], [320, 480]], 416)
    assert np.array_equal(got, want) and len(got) == 3                        # 1 / 500 * 416 < 1 dropped, 1 / 320 * 416 >= 1 kept
    coco = {"images": [{"id": 7, "width": 640, "height": 480}, {"id": 9, "width": 100, "height": 200}],
            "annotations": [{"image_id": 7, "bbox": [10.5, 20.0, 100.0, 50.5], "area": 5000.0},
                            {"image_id": 9, "bbox": [-4.0, 3.0, 50.0, 60.0], "area": 10.0},
                            {"image_id": 9, "bbox": [1.0, 1.0, 30.0, 30.0], "area": 0.0},
                            {"image_id": 7, "bbox": [0.0, 0.0, 1.0, 300.0], "area": 300.0}]}
    want = A.boxes_from_annotations([[10.5, 20.0, 110.5, 70.5], [0.0, 3.0, 50.0, 63.0], [0.0, 0.0, 1.0, 300.0]], [[640, 480], [100, 200], [640, 480]], 416)
    assert np.array_equal(A.coco_boxes(coco, 416), want) and len(want) == 2
    p = tmp_path / "instances.json"
    p.write_text(json.dumps(coco))
    assert np.array_equal(A.coco_boxes(str(p), 416), want)


def test_python_side_without_a_gpu(tmp_path):
    import argparse
    import torch
    from yolo355.tools import fit_anchors as cli
    coco = {"images": [{"id": 1, "width": 416, "height": 208}], "annotations": [{"image_id": 1, "bbox": [1.0, 2.0, 30.0, 40.0], "area": 1200.0}]}
    (tmp_path / "c.json").write_text(json.dumps(coco))
    got = cli.load_boxes(argparse.Namespace(dataset="coco", annotations=str(tmp_path / "c.json"), input_size=416))
    assert np.array_equal(got, [[30.0 / 416 * 416, 40.0 / 208 * 416]])
    with pytest.raises(SystemExit):
        cli.load_boxes(argparse.Namespace(dataset="voc", annopath=None, ids=None, input_size=416))
    assert cli.fmt([[1.234, 5.0]]) == "[[1.23, 5.00]]"
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            A.fit_anchors(AC.boxes("b257"), 3)
        with pytest.raises(RuntimeError):
            cli.main(["-d", "coco", "--annotations", str(tmp_path / "c.json"), "-na", "1"])
