"""VOC AP without a GPU: the NumPy restatement of the contract (tests/voc_ap_ref.py, the oracle of tests/test_voc_ap.py) against
the reference's own write_voc_results_file + voc_eval output (tests/golden/voc_ap.npz, made by tests/golden/gen_golden_voc_ap.py),
the XML reader, and the argument checks of the y355_apeval_* C ABI from a plain C program."""
import os
import subprocess

import numpy as np
import pytest

import voc_ap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a", "b", "c", "d")


def load_case(z, name):
    """-> (num_classes, ground_truth list, boxes, scores, cls, count) of a fixture case"""
    off, g = z[name + "/gt_off"], z[name + "/gt"].astype(np.float64)
    gt = [g[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return int(z[name + "/num_classes"]), gt, z[name + "/boxes"], z[name + "/scores"], z[name + "/cls"], z[name + "/count"]


@pytest.fixture(scope="module")
def golden_ap():
    with np.load(os.path.join(ROOT, "tests", "golden", "voc_ap.npz")) as z:
        return {k: z[k] for k in z.files}


def same(a, b):
    """bit for bit, NaN where the reference has NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_bit_for_bit(golden_ap, name):
    C, gt, boxes, scores, cls, count = load_case(golden_ap, name)
    for use07, key in ((True, "ap07"), (False, "ap_area")):
        got = R.evaluate(C, gt, boxes, scores, cls, count, 0.5, use07, True)
        assert same(got["ap"], golden_ap["%s/%s" % (name, key)]), (name, key, got["ap"], golden_ap["%s/%s" % (name, key)])
        for c in range(C):
            assert same(got["rec"][c], golden_ap["%s/rec/%d" % (name, c)]), (name, c)
            assert same(got["prec"][c], golden_ap["%s/prec/%d" % (name, c)]), (name, c)


def test_the_fixture_holds_the_edge_cases(golden_ap):
    """case d is what the issue lists: IoU exactly 0.5 / duplicate / NaN overlap -> FP, a difficult match -> neither, a class with
    detections and no box, a class with only difficult boxes (0.0 under VOC07, NaN under AREA), a class without detections (-1)"""
    C, gt, boxes, scores, cls, count = load_case(golden_ap, "d")
    got = R.evaluate(C, gt, boxes, scores, cls, count, 0.5, True, True)
    # class 0 in rank order: .99 difficult, .93 TP, .82 duplicate, .77 NaN, .71 TP, .61 IoU 0.5, .52 image without boxes
    assert got["flag"][0].tolist() == [0, 1, 2, 2, 1, 2, 2]
    assert got["prec"][0][0] == 0.0                                # tp + fp = 0 at rank 0: 0 / eps
    assert got["npos"].tolist() == [4, 0, 0, 2] and got["ndet"].tolist() == [7, 2, 3, 0]
    assert golden_ap["d/ap07"].tolist()[1:] == [0.0, 0.0, -1.0]
    area = golden_ap["d/ap_area"]
    assert np.isnan(area[1]) and np.isnan(area[2]) and area[3] == -1.0
    # the tied case really has ties inside a class
    C, gt, boxes, scores, cls, count = load_case(golden_ap, "c")
    img, pos, dcls, dsc, _ = R.flatten(boxes, scores, cls, count)
    assert any(len(np.unique(dsc[dcls == c])) < (dcls == c).sum() for c in range(C))


def test_quantisation_formulas_are_the_text_file_round_trip():
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.random(2000), [0.0005, 0.0015, 0.0625, 0.9995, 1.0]]).astype(np.float32)
    assert np.array_equal(R.quantize_scores(s), np.array([float("{:.3f}".format(v)) for v in s]))
    b = np.concatenate([rng.uniform(-50, 600, 2000), [0.05, 0.25, 10.75, -1.0]]).astype(np.float32)
    assert np.array_equal(R.quantize_coords(b), np.array([float("{:.1f}".format(v + 1)) for v in b]))


def test_voc_ground_truth_reads_voc_xml(tmp_path):
    from yolo355.utils.evaluator_batch import voc_ground_truth
    obj = ("<object><name>%s</name><pose>Left</pose><truncated>0</truncated>%s<bndbox><xmin>%d</xmin><ymin>%d</ymin>"
           "<xmax>%d</xmax><ymax>%d</ymax></bndbox></object>")
    files = {
        "000001": obj % ("dog", "<difficult>0</difficult>", 48, 240, 195, 371) + obj % ("person", "<difficult>1</difficult>", 8, 12, 352, 498),
        "000002": "",
        "000003": obj % ("zebra", "<difficult>0</difficult>", 1, 2, 3, 4) + obj % ("person", "", 5, 6, 70, 80),
    }
    for k, body in files.items():
        (tmp_path / (k + ".xml")).write_text("<annotation><filename>%s.jpg</filename>%s</annotation>" % (k, body))
    gt = voc_ground_truth(str(tmp_path / "%s.xml"), ["000001", "000002", "000003"], ["person", "dog"])
    assert [g.shape for g in gt] == [(2, 6), (0, 6), (1, 6)]
    assert gt[0].tolist() == [[1, 48, 240, 195, 371, 0], [0, 8, 12, 352, 498, 1]]
    assert gt[2].tolist() == [[0, 5, 6, 70, 80, 0]]                # a name outside the labelmap is skipped; no <difficult>: 0


def test_header_library_and_ffi_agree_on_the_apeval_symbols():
    from yolo355 import _ffi
    names = ["y355_apeval_" + n for n in ("create", "destroy", "set_gt", "add", "add_host", "reset", "compute", "curve")]
    declared = _ffi.declared_symbols()
    lib = _ffi.lib()
    for n in names:
        assert n in declared and n in _ffi._SIGS and hasattr(lib, n), n
    hdr = open(_ffi.HEADER_PATH).read()
    for name, val in (("AP_VOC07", 0), ("AP_AREA", 1), ("AP_Q_VOCFILE", 0), ("AP_Q_NONE", 1)):
        assert getattr(_ffi, name) == val and "#define Y355_%s %d\n" % (name, val) in hdr, name


def test_apeval_argument_checks_from_a_c_program(tmp_path):
    """tests/c_client/apeval_client.c: every y355_apeval_* entry point linked from C99, every argument check answered before any
    HIP call (so it passes without a GPU; with one, the checks that need a live handle run too)"""
    from yolo355 import _ffi
    exe = str(tmp_path / "apeval_client")
    libdir = os.path.dirname(_ffi.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c_client", "apeval_client.c"), "-o", exe, "-L", libdir, "-l:libyolo355.so",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith("ok apeval")


def test_apeval_needs_a_gpu_and_says_so():
    """no host fallback: without a GPU the constructor raises; with one it builds a handle"""
    import torch
    from yolo355.apeval import ApEval
    if torch.cuda.is_available():
        ApEval(2, [np.zeros((0, 6))], max_dets=8).close()
    else:
        with pytest.raises(RuntimeError, match="no GPU"):
            ApEval(2, [np.zeros((0, 6))])
