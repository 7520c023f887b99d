"""Records tests/golden/python_api_parent.json: the Python API over the C ABI at one commit -- every public name of
yolo355.engine, yolo355.netengine and yolo355.apeval (their classes' public methods and properties included), the model
classes of yolo355.models.slim_yolo_v2, and the private names other code relies on (PRIVATE below).  A record is the dotted
path and str(inspect.signature(...)), "<property>", "<instance attribute>" (set in __init__: only a live handle has it), or a
constant's repr.  Run at the commit whose API is to be pinned -- the parent of a change that must not move it; no GPU needed:

    python tests/golden/gen_golden_python_api.py [output.json]

tests/test_python_api.py resolves every path through the module it was recorded in and compares."""
import importlib
import inspect
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

MODULES = ["yolo355.engine", "yolo355.netengine", "yolo355.apeval"]
MODEL_CLASSES = ["SlimYOLOv2_quantize_bnfuse", "_NetModel", "SlimYOLOv2"]          # of yolo355.models.slim_yolo_v2
# private names tests, bench.py or other modules of the package reach for
PRIVATE = {"Engine": ["_buffers", "_dev_input"], "Net": ["_buffers", "_collect"],
           "SlimYOLOv2_quantize_bnfuse": ["_tracker_states"], "_NetModel": ["_get_net"]}
INSTANCE = {"yolo355.engine.Engine": ["_h", "_lib", "_stream"], "yolo355.engine.Pipeline": ["_h", "_lib"],
            "yolo355.netengine.Net": ["_h"]}
INSTANCE_MARK, PROPERTY_MARK = "<instance attribute>", "<property>"


def describe(obj):
    if isinstance(obj, property):
        return PROPERTY_MARK
    if isinstance(obj, (staticmethod, classmethod)):
        obj = obj.__func__
    if callable(obj):
        return str(inspect.signature(obj))
    return repr(obj)


def own_members(cls):
    """name -> the raw class attribute, from the classes of the MRO that live in this package (nn.Module's are not ours)"""
    out = {}
    for k in reversed(cls.__mro__):
        if k.__module__.startswith("yolo355"):
            out.update(vars(k))
    return out


def class_records(path, cls):
    rec = {path: describe(cls)}
    for name, raw in own_members(cls).items():
        if name.startswith("_") and name not in PRIVATE.get(cls.__name__, ()):
            continue
        rec["%s.%s" % (path, name)] = describe(raw)
    for name in INSTANCE.get(path, ()):
        rec["%s.%s" % (path, name)] = INSTANCE_MARK
    return rec


def records():
    rec = {}
    for mname in MODULES:
        mod = importlib.import_module(mname)
        for name, obj in vars(mod).items():
            if name.startswith("_") or isinstance(obj, types.ModuleType):
                continue
            path = "%s.%s" % (mname, name)
            if inspect.isclass(obj):
                if obj.__module__.startswith("yolo355"):
                    rec.update(class_records(path, obj))
            elif callable(obj):
                if getattr(obj, "__module__", "").startswith("yolo355"):
                    rec[path] = describe(obj)
            else:
                rec[path] = repr(obj)
    mod = importlib.import_module("yolo355.models.slim_yolo_v2")
    for cname in MODEL_CLASSES:
        rec.update(class_records("yolo355.models.slim_yolo_v2.%s" % cname, getattr(mod, cname)))
    return rec


def main():
    commit = os.environ.get("Y355_GOLDEN_COMMIT")
    if not commit:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "python_api_parent.json")
    rec = records()
    with open(out, "w") as f:
        json.dump({"commit": commit, "records": rec}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "with", len(rec), "records")


if __name__ == "__main__":
    main()
