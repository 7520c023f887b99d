"""Records tests/golden/apeval_abi_parent.json: what the y355_apeval_* entry points of libyolo355.so answer at one commit --
(call, return code, y355_last_error() text), as tests/golden/gen_golden_c_abi.py records the two model families:
  * "records": calls that answer before any device work -- the rules of y355_apeval_create, every other entry point with a
    null handle, y355_apeval_destroy(NULL) (no return value: recorded as null);
  * "gpu_records" (--gpu, on a GPU): one live handle of 3 classes, 2 images and max_dets 8 walked through the rules of every
    entry point in the order they are checked, the two Y355_ERANGE texts of an overfull store and of a class out of range, and
    the "not ready" answers before a ground truth, before a compute and after a later add.  The calls change the handle, so
    their order is part of the record.
Run at the commit whose answers are to be pinned -- the parent of a change that must not move them:

    python tests/golden/gen_golden_apeval_abi.py [output.json]            # no GPU needed
    python tests/golden/gen_golden_apeval_abi.py --gpu [output.json]      # appends gpu_records to the file

tests/test_apeval_abi_parent.py replays cpu_calls() / gpu_calls() on the built library and compares."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

CLASSES, IMAGES, MAX_DETS = 3, 2, 8
T, R, A, M = 10, 101, 4, 3                       # COCOeval's default parameter sizes


class Args:
    """valid arguments of every entry point for the handle above; the arrays live as long as the object"""

    def __init__(self):
        f32, f64, i32, i64, u8 = C.c_float, C.c_double, C.c_int32, C.c_int64, C.c_uint8
        self.off, self.off_1, self.off_dec = (i32 * 3)(0, 1, 2), (i32 * 3)(1, 1, 2), (i32 * 3)(0, 2, 1)
        self.gt_box = (f32 * 8)(10, 10, 50, 50, 20, 20, 60, 60)
        self.gt_cls, self.gt_cls_3, self.gt_diff = (i32 * 2)(0, 1), (i32 * 2)(0, 3), (u8 * 2)(0, 0)
        self.co_box, self.co_area = (f64 * 8)(10, 10, 40, 40, 20, 20, 40, 40), (f64 * 2)(1600, 1600)
        self.rank_2, self.rank_dup = (i32 * 2)(0, 2), (i32 * 2)(0, 0)
        # detections of a batch of 2 images, max_det 8 (16 records; add_host reads all of them, the count says how many are real)
        self.boxes = (f32 * 64)(*([10, 10, 50, 50] * 16))
        self.scores = (f32 * 16)(*[0.9 - 0.05 * i for i in range(16)])
        self.cls, self.cls_7 = (i32 * 16)(*([0] * 8 + [1] * 8)), (i32 * 16)(*([7] * 16))
        self.count_2, self.count_9, self.count_1 = (i32 * 2)(1, 1), (i32 * 2)(8, 1), (i32 * 2)(1, 0)
        # outputs
        self.ap, self.npos, self.ndet, self.mean = (f64 * CLASSES)(), (i32 * CLASSES)(), (i64 * CLASSES)(), f64(0)
        self.rec, self.prec, self.flag, self.n = (f64 * 16)(), (f64 * 16)(), (u8 * 16)(), i64(0)
        self.iou = (f64 * T)(*[0.5 + 0.05 * t for t in range(T)])
        self.rthr = (f64 * R)(*[r / 100.0 for r in range(R)])
        self.area = (f64 * (2 * A))(0, 1e10, 0, 1024, 1024, 9216, 9216, 1e10)
        self.md, self.md_0, self.md_desc = (i32 * M)(1, 10, 100), (i32 * 1)(0), (i32 * 2)(10, 1)
        self.precision, self.recall, self.stats = (f64 * (T * R * CLASSES * A * M))(), (f64 * (T * CLASSES * A * M))(), (f64 * 12)()
        self.num_d, self.num_g = i64(0), i64(0)
        self.pos, self.dtm, self.dti, self.gtm = (i32 * 8)(), (i32 * (T * 8))(), (u8 * (T * 8))(), (u8 * (T * 8))()

    def set_gt(self, **kw):
        d = dict(off=self.off, box=self.gt_box, cls=self.gt_cls, diff=self.gt_diff)
        d.update(kw)
        return (d["off"], d["box"], d["cls"], d["diff"])

    def add(self, first=0, batch=2, max_det=8, boxes=True, cls=None, count=None):
        return (first, batch, max_det, self.boxes if boxes else None, self.scores, cls or self.cls, count or self.count_2)

    def compute(self, thr=0.5, metric=0, quantize=0, ap=True):
        return (thr, metric, quantize, self.ap if ap else None, self.npos, self.ndet, C.byref(self.mean))

    def curve(self, cls=0, cap=16, n=True):
        return (cls, cap, self.rec, self.prec, self.flag, C.byref(self.n) if n else None)

    def set_gt_coco(self, **kw):
        d = dict(off=self.off, box=self.co_box, area=self.co_area, cls=self.gt_cls, crowd=self.gt_diff, rank=None)
        d.update(kw)
        return (d["off"], d["box"], d["area"], d["cls"], d["crowd"], d["rank"])

    def compute_coco(self, t=T, r=R, a=A, m=M, iou=True, md=None, precision=True):
        return (self.iou if iou else None, t, self.rthr, r, self.area, a, md or self.md, m, self.precision if precision else None,
                self.recall, self.stats)

    def matches(self, image=0, cls=0, area=0, cap_d=8, cap_g=8, num=True):
        return (image, cls, area, cap_d, cap_g, C.byref(self.num_d) if num else None, C.byref(self.num_g), self.pos, self.dtm, self.dti,
                self.gtm)


def _call(name, tag, h, args):
    return ("y355_apeval_%s(%s)" % (name, tag), name, (h,) + tuple(args))


def cpu_calls(v):
    hout = C.c_void_p()
    create = lambda tag, *a: ("y355_apeval_create(%s)" % tag, "create", a)       # noqa: E731
    calls = [create("null out", 0, CLASSES, IMAGES, MAX_DETS, None), create("device_id -1", -1, CLASSES, IMAGES, MAX_DETS, C.byref(hout)),
             create("num_classes 0", 0, 0, IMAGES, MAX_DETS, C.byref(hout)), create("num_classes 257", 0, 257, IMAGES, MAX_DETS, C.byref(hout)),
             create("num_images 0", 0, CLASSES, 0, MAX_DETS, C.byref(hout)),
             create("num_images 2^24 + 1", 0, CLASSES, (1 << 24) + 1, MAX_DETS, C.byref(hout)),
             create("max_dets 0", 0, CLASSES, IMAGES, 0, C.byref(hout)),
             create("max_dets 2^27 + 1", 0, CLASSES, IMAGES, (1 << 27) + 1, C.byref(hout))]
    null = "null handle"
    calls += [_call("set_gt", null, None, v.set_gt()), _call("add", null, None, v.add() + (None,)), _call("add_host", null, None, v.add()),
              _call("reset", null, None, ()), _call("compute", null, None, v.compute()), _call("curve", null, None, v.curve()),
              _call("set_gt_coco", null, None, v.set_gt_coco()), _call("compute_coco", null, None, v.compute_coco()),
              _call("coco_matches", null, None, v.matches()), ("y355_apeval_destroy(NULL)", "destroy", (None,))]
    return calls


def gpu_calls(v, h):
    """on a live handle of CLASSES classes, IMAGES images and max_dets MAX_DETS, fresh from y355_apeval_create"""
    live = lambda name, tag, args: _call(name, "live, " + tag, h, args)       # noqa: E731
    calls = []
    gt_rules = [("null offsets", dict(off=None)), ("offsets[0] 1", dict(off=v.off_1)), ("decreasing offsets", dict(off=v.off_dec)),
                ("null arrays", dict(box=None)), ("class 3", dict(cls=v.gt_cls_3))]
    calls += [live("set_gt", tag, v.set_gt(**kw)) for tag, kw in gt_rules]
    calls += [live("compute", "no ground truth", v.compute()), live("compute", "null output", v.compute(ap=False)),
              live("compute", "metric 2", v.compute(metric=2)), live("compute", "quantize 2", v.compute(quantize=2)),
              live("compute", "NaN threshold", v.compute(thr=float("nan"))), live("set_gt", "ok", v.set_gt())]
    for name, tail in (("add", (None,)), ("add_host", ())):
        calls += [live(name, "null buffer", v.add(boxes=False) + tail), live(name, "batch 0", v.add(batch=0) + tail),
                  live(name, "first_image 1, batch 2", v.add(first=1) + tail), live(name, "max_det 0", v.add(max_det=0) + tail),
                  live(name, "max_det 2^20 + 1", v.add(max_det=(1 << 20) + 1) + tail)]
    calls += [live("curve", "before a compute", v.curve()), live("curve", "class 3", v.curve(cls=3)), live("curve", "capacity -1", v.curve(cap=-1)),
              live("curve", "null n", v.curve(n=False)), live("add_host", "2 detections", v.add()), live("compute", "ok", v.compute()),
              live("curve", "ok", v.curve()), live("add_host", "2 more", v.add()), live("curve", "after a later add", v.curve())]
    calls += [live("reset", "1", ()), live("add_host", "9 detections into 8", v.add(count=v.count_9)), live("compute", "store overfull", v.compute()),
              live("reset", "2", ()), live("add_host", "class 7", v.add(cls=v.cls_7, count=v.count_1)), live("compute", "class outside", v.compute()),
              live("reset", "3", ()), live("add_host", "2 detections again", v.add()), live("compute", "ok again", v.compute())]
    calls += [live("set_gt_coco", tag, v.set_gt_coco(**kw)) for tag, kw in gt_rules]
    calls += [live("set_gt_coco", "rank 2", v.set_gt_coco(rank=v.rank_2)), live("set_gt_coco", "duplicate rank", v.set_gt_coco(rank=v.rank_dup))]
    calls += [live("compute_coco", "no COCO ground truth", v.compute_coco()), live("compute_coco", "null parameter array", v.compute_coco(iou=False)),
              live("compute_coco", "null output", v.compute_coco(precision=False))]
    for key, bad in (("t", (0, 17)), ("r", (0, 1025)), ("a", (0, 9)), ("m", (0, 9))):
        calls += [live("compute_coco", "%s %d" % (key.upper(), x), v.compute_coco(**{key: x})) for x in bad]
    calls += [live("compute_coco", "max_dets {0}", v.compute_coco(m=1, md=v.md_0)),
              live("compute_coco", "max_dets {10, 1}", v.compute_coco(m=2, md=v.md_desc)), live("set_gt_coco", "ok", v.set_gt_coco())]
    calls += [live("coco_matches", "null count", v.matches(num=False)), live("coco_matches", "image 2", v.matches(image=2)),
              live("coco_matches", "class 3", v.matches(cls=3)), live("coco_matches", "capacity -1", v.matches(cap_d=-1)),
              live("coco_matches", "before a COCO compute", v.matches()), live("compute_coco", "ok", v.compute_coco()),
              live("coco_matches", "area index A", v.matches(area=A)), live("coco_matches", "ok", v.matches())]
    return calls


def run(lib, calls):
    out = []
    for label, name, args in calls:
        rc = getattr(lib, "y355_apeval_" + name)(*args)
        out.append([label, rc, lib.y355_last_error().decode() if rc else ""])
    return out


def live_handle(lib):
    h = C.c_void_p()
    rc = lib.y355_apeval_create(0, CLASSES, IMAGES, MAX_DETS, C.byref(h))
    assert rc == 0, lib.y355_last_error().decode()
    return h


def main():
    from yolo355 import _ffi
    args = [a for a in sys.argv[1:] if a != "--gpu"]
    out = args[0] if args else os.path.join(HERE, "apeval_abi_parent.json")
    lib = _ffi.lib()
    v = Args()
    if "--gpu" in sys.argv:
        with open(out) as f:
            doc = json.load(f)
        h = live_handle(lib)
        try:
            doc["gpu_records"] = run(lib, gpu_calls(v, h))
        finally:
            lib.y355_apeval_destroy(h)
    else:
        commit = os.environ.get("Y355_GOLDEN_COMMIT")
        if not commit:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        doc = {"commit": commit, "records": run(lib, cpu_calls(v))}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "with", len(doc["records"]), "records,", len(doc.get("gpu_records", [])), "gpu records")


if __name__ == "__main__":
    main()
