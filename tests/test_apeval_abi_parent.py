"""The y355_apeval_* entry points of libyolo355.so, pinned to tests/golden/apeval_abi_parent.json (recorded by
tests/golden/gen_golden_apeval_abi.py at the commit named in the file): every recorded call still answers with the recorded
return code and y355_last_error() text -- wherever the code behind it lives now.  The "records" need no GPU; the
"gpu_records" are replayed, in the recorded order, on one live handle of 3 classes, 2 images and max_dets 8."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_apeval_abi", os.path.join(GOLDEN, "gen_golden_apeval_abi.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the generator's calls: one definition of a record

with open(os.path.join(GOLDEN, "apeval_abi_parent.json")) as _f:
    DOC = json.load(_f)

ENTRY_POINTS = ("create", "destroy", "set_gt", "add", "add_host", "reset", "compute", "curve", "set_gt_coco", "compute_coco", "coco_matches")


def _compare(got, want):
    assert [r[0] for r in got] == [r[0] for r in want]          # the same calls, in the recorded order
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad


def test_the_snapshot_covers_every_entry_point():
    labels = [r[0] for r in DOC["records"]]
    assert len(labels) == len(set(labels)) == 18
    assert sum(lb.startswith("y355_apeval_create(") for lb in labels) == 8 and sum("null handle" in lb for lb in labels) == 9
    assert {lb.split("(")[0] for lb in labels} == {"y355_apeval_" + n for n in ENTRY_POINTS}
    live = [r[0] for r in DOC["gpu_records"]]
    assert len(live) == len(set(live)) == 68
    assert {lb.split("(")[0] for lb in live} == {"y355_apeval_" + n for n in ENTRY_POINTS[2:]}
    texts = {r[2] for r in DOC["gpu_records"]}
    assert "9 detections were added, the store holds max_dets = 8" in texts
    assert "1 detections carry a class index outside 0 .. 2" in texts
    assert sorted({r[1] for r in DOC["gpu_records"]}) == [-4, -3, -1, 0]        # ERANGE, ENOTREADY, EINVAL, success


def test_answers_before_any_device_work():
    from yolo355 import _ffi
    lib = _ffi.lib()
    _compare(G.run(lib, G.cpu_calls(G.Args())), DOC["records"])


@pytest.mark.gpu
def test_answers_of_a_live_handle():
    from yolo355 import _ffi
    lib = _ffi.lib()
    h = G.live_handle(lib)
    try:
        got = G.run(lib, G.gpu_calls(G.Args(), h))
    finally:
        lib.y355_apeval_destroy(h)
    _compare(got, DOC["gpu_records"])
