"""The entry points of libyolo355_loss.so and libyolo355_anchors.so, pinned to tests/golden/companion_abi_parent.json (recorded
by tests/golden/gen_golden_companion_abi.py at the commit named in the file): every recorded call still answers with the
recorded return code and its family's last-error text -- wherever the code behind it lives now.  The "records" need no GPU;
the "gpu_records" are replayed, in the recorded order, on one live handle per library.  And the three libraries' error texts
stay apart in a process that holds all of them in its global scope."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_companion_abi", os.path.join(GOLDEN, "gen_golden_companion_abi.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the generator's calls: one definition of a record

with open(os.path.join(GOLDEN, "companion_abi_parent.json")) as _f:
    DOC = json.load(_f)

LOSS = ("default_config", "create", "destroy", "num_anchors_total", "set_labels", "get_targets", "compute", "iou_score", "flat")
ANCHORS = ("chunk", "create", "destroy", "set_boxes", "set_boxes_dev", "num_boxes", "fit", "get_result", "assignments", "score")


def _compare(got, want):
    assert [r[0] for r in got] == [r[0] for r in want]          # the same calls, in the recorded order
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad


def test_the_snapshot_covers_every_entry_point():
    from yolo355 import anchors as A, loss as L
    for key in ("records", "gpu_records"):
        labels = [r[0] for r in DOC[key]]
        assert len(labels) == len(set(labels))
    names = {r[0].split("(")[0] for r in DOC["records"]}
    assert names == {"y355_loss_" + n for n in LOSS} | {"y355_anchors_" + n for n in ANCHORS}
    assert names | {"y355_loss_last_error", "y355_anchors_last_error"} == set(L._SIGS) | set(A._SIGS)      # every entry point of both headers
    assert sum(r[0].startswith("y355_loss_create(") for r in DOC["records"]) == 29 and sum(r[0].startswith("y355_anchors_create(") for r in DOC["records"]) == 8
    assert all(r[1] in (-1, 0, None) for r in DOC["records"] if r[0] != "y355_anchors_chunk()")
    live = {r[0].split("(")[0] for r in DOC["gpu_records"]}
    assert live == {"y355_loss_" + n for n in LOSS if n not in ("default_config", "destroy")} | \
        {"y355_anchors_" + n for n in ANCHORS if n not in ("chunk", "destroy")}
    texts = {r[2] for r in DOC["gpu_records"]}
    for t in ("y355_loss_get_targets: no labels set", "y355_loss_compute: labels were set for a batch of 1, not 2", "image 1 has 3 labels, max_labels_per_image is 2",
              "label 1: coordinate outside [0, 1]", "y355_anchors_fit: no boxes set", "y355_anchors_get_result: no fit made", "box 1: w must be finite and > 0",
              "n must be 1..max_boxes (1025)", "y355_loss_create: invalid device ordinal", "y355_anchors_create: invalid device ordinal"):
        assert t in texts, t
    assert {r[1] for r in DOC["gpu_records"]} == {-3, -2, -1, 0, 3, 8}         # ENOTREADY, EHIP, EINVAL, success, 3 boxes, 8 anchors


def test_answers_before_any_device_work():
    from yolo355 import anchors as A, loss as L
    _compare(G.run_cpu(L, A), DOC["records"])


@pytest.mark.gpu
def test_answers_of_live_handles():
    from yolo355 import anchors as A, loss as L
    _compare(G.run_gpu(L, A), DOC["gpu_records"])


_CHILD = r"""
import ctypes as C, sys
main, loss, anchors = (C.CDLL(p, mode=C.RTLD_GLOBAL) for p in sys.argv[1:4])      # the main library first: its symbols lead the global scope
errs = []
for lib, name in ((main, "y355_last_error"), (loss, "y355_loss_last_error"), (anchors, "y355_anchors_last_error")):
    getattr(lib, name).restype = C.c_char_p
    errs.append(getattr(lib, name))
text = lambda: [e().decode() for e in errs]
assert text() == ["", "", ""], text()
out = C.c_void_p()
assert loss.y355_loss_create(None, None) == -1
assert text() == ["", "y355_loss_create: null argument", ""], text()
assert anchors.y355_anchors_create(0, 10, 1, 4, None) == -1
assert text() == ["", "y355_loss_create: null argument", "y355_anchors_create: null out"], text()
assert main.y355_apeval_create(0, 3, 2, 8, None) == -1
assert text() == ["null argument", "y355_loss_create: null argument", "y355_anchors_create: null out"], text()
assert anchors.y355_anchors_create(-1, 10, 1, 4, C.byref(out)) == -1 and loss.y355_loss_default_config(None) == -1
assert text() == ["null argument", "y355_loss_default_config: null config", "device_id < 0"], text()
print("apart")
"""


def test_error_state_stays_per_library():
    """a fresh process with all three libraries in its global scope, one refused call each: every family's text is its own"""
    from yolo355 import _ffi, anchors as A, loss as L
    r = subprocess.run([sys.executable, "-c", _CHILD, _ffi.LIB_PATH, L.LIB_PATH, A.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "apart", r.stdout + r.stderr
