"""The Python API over the C ABI, pinned to tests/golden/python_api_parent.json (recorded by
tests/golden/gen_golden_python_api.py at the commit named in the file): every recorded name still resolves through the module
it was recorded in and has the recorded signature -- wherever the code behind it lives now.  No GPU."""
import importlib
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_golden_python_api", os.path.join(GOLDEN, "gen_golden_python_api.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                               # the generator's describe(): one definition of a record

with open(os.path.join(GOLDEN, "python_api_parent.json")) as _f:
    RECORDS = json.load(_f)["records"]


def _resolve(path):
    """(owner, raw attribute) of a dotted path: the longest importable prefix is the module, the rest attributes; a class
    attribute is taken raw from the MRO, so that a property or a static method is seen as such"""
    parts = path.split(".")
    for k in range(len(parts), 0, -1):
        try:
            obj = importlib.import_module(".".join(parts[:k]))
        except ImportError:
            continue
        for name in parts[k:-1]:
            obj = getattr(obj, name)
        last = parts[-1]
        if isinstance(obj, type):
            for klass in obj.__mro__:
                if last in vars(klass):
                    return obj, vars(klass)[last]
            raise AttributeError(path)
        return obj, getattr(obj, last)
    raise ImportError(path)


def test_the_snapshot_is_the_whole_api():
    assert len(RECORDS) == 203
    assert sum(p.startswith(("yolo355.engine.", "yolo355.netengine.")) for p in RECORDS) >= 148
    for must in ("yolo355.engine.Engine._buffers", "yolo355.engine.Engine._dev_input", "yolo355.engine.Engine._stream",
                 "yolo355.engine.Pipeline._h", "yolo355.netengine.Net._collect", "yolo355.engine.NUM_LAYERS",
                 "yolo355.engine.LAYER_NAMES", "yolo355.netengine.PRED_TAIL", "yolo355.engine.mfma_peak_i8",
                 "yolo355.engine.conv3x3_i8_fused", "yolo355.models.slim_yolo_v2.SlimYOLOv2_quantize_bnfuse.PIPELINE_CHUNK"):
        assert must in RECORDS, must


@pytest.mark.parametrize("path", sorted(p for p, v in RECORDS.items() if v != G.INSTANCE_MARK))
def test_name_resolves_with_its_signature(path):
    _, raw = _resolve(path)
    assert G.describe(raw) == RECORDS[path]


def test_instance_attributes_are_set_by_the_handle_base():
    """_h / _lib / _stream exist on a live handle only (tests/test_entry_points_agree.py looks at real ones); here: the
    classes that recorded them still get them from the one place that sets them"""
    from yolo355 import _handle
    for path, mark in RECORDS.items():
        if mark != G.INSTANCE_MARK:
            continue
        cls, attr = _resolve(path.rsplit(".", 1)[0])[1], path.rsplit(".", 1)[1]
        assert issubclass(cls, _handle.Handle), path
        if attr == "_stream":
            assert issubclass(cls, _handle.StreamBound), path
        else:
            obj = cls.__new__(cls)
            obj._own(None, 7, owned=False)
            assert getattr(obj, attr) == (7 if attr == "_h" else None)
            assert obj not in _handle._live
