"""Records tests/golden/c_abi_parent.json: the C ABI of libyolo355.so at one commit, as its callers see it --
  * "symbols": the sorted y355_* symbols the library exports;
  * "records": (call, return code, y355_last_error() text) of calls that answer before any device work -- the rules of
    y355_create / y355_net_create and the entry points the two handle families pair, with a null handle and with null arrays;
  * "gpu_records" (--gpu, on a GPU): the same on a live handle of each family (SlimYOLOv2, 96 x 96, max_batch 2) -- batches out
    of range, unknown options and option values out of range, a non-positive std, tracker counts off by one, profile_get after
    an unprofiled forward.
Run at the commit whose ABI is to be pinned -- the parent of a change that must not move it:

    python tests/golden/gen_golden_c_abi.py [output.json]            # no GPU needed
    python tests/golden/gen_golden_c_abi.py --gpu [output.json]      # appends gpu_records to the file

tests/test_c_abi_parent.py replays cpu_calls() / gpu_calls() on the built library and compares."""
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

SIZE, BATCH, CLASSES = 96, 2, 2
NO_MESSAGE = ("max_candidates", "max_det", "num_anchors_total")      # getters: Y355_EINVAL for a null handle, no message


def symbols(lib_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("y355_")})


def _answer(lib, label, fn, *args):
    rc = fn(*args)
    if label.split("(")[0].replace("y355_net_", "").replace("y355_", "") in NO_MESSAGE:
        return [label, rc, None]
    return [label, rc, lib.y355_last_error().decode() if rc else ""]


def _config(ffi, net=False, **kw):
    from yolo355 import synth
    cfg = ffi.NetConfig() if net else ffi.Config()
    cfg.device_id, cfg.height, cfg.width, cfg.num_classes, cfg.num_anchors = 0, SIZE, SIZE, CLASSES, 5
    for i, (w, h) in enumerate(synth.ANCHOR_SIZE_MASK):
        cfg.anchors[2 * i], cfg.anchors[2 * i + 1] = w, h
    cfg.conf_thresh, cfg.nms_thresh, cfg.max_batch, cfg.max_det = 0.01, 0.5, BATCH, 0
    if net:
        cfg.arch, cfg.dtype = ffi.ARCH_SLIM_V2, ffi.DT_INT8
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _paired(ffi, lib, h, tag, batches=(1,), fams=("y355_", "y355_net_")):
    """(label, fn, args) of the entry points the two families pair on handle h (None: the null handle) with valid arrays, for
    every batch of `batches`"""
    f3 = (C.c_float * 3)(0.4, 0.4, 0.4)
    buf = (C.c_float * 4096)()
    ibuf = (C.c_int32 * 64)()
    i64 = (C.c_int64 * 2)()
    frames = (ffi.Frame * 4)()
    for f in frames:
        f.data_dev, f.height, f.width, f.row_bytes = C.addressof(buf), 2, 2, 0
    ov = C.c_int(0)
    ip, fp = C.cast(ibuf, C.POINTER(C.c_int32)), C.cast(buf, C.POINTER(C.c_float))
    out = []
    for fam in fams:
        net = fam == "y355_net_"
        g = lambda name: getattr(lib, fam + name)       # noqa: E731
        lab = lambda name, extra="": "%s%s(%s%s)" % (fam, name, tag, extra)      # noqa: E731
        out += [(lab("set_thresholds"), g("set_thresholds"), (h, 0.1, 0.5)),
                (lab("max_candidates"), g("max_candidates"), (h,)), (lab("max_det"), g("max_det"), (h,)),
                (lab("num_anchors_total"), g("num_anchors_total"), (h,)),
                (lab("overflow"), g("overflow"), (h, C.byref(ov))),
                (lab("set_normalization"), g("set_normalization"), (h, f3, f3)),
                (lab("sync"), g("sync"), (h,)), (lab("profile"), g("profile"), (h, 0))]
        for b in batches:
            bt = ", batch %d" % b
            out += [(lab("get_candidates", bt), g("get_candidates"), (h, b, buf, buf, ibuf)),
                    (lab("scale_boxes", bt), g("scale_boxes"), (h, buf, ibuf, buf, b)),
                    (lab("resize_frames", bt), g("resize_frames"), (h, frames, b, buf))]
            if net:
                out.append((lab("resize_u8", bt), g("resize_u8"), (h, buf, 2, 2, b, buf)))
            else:
                out.append((lab("forward_u8_resized", bt), g("forward_u8_resized"), (h, buf, 2, 2, b, 0, None, None, None, None, buf)))
        if h is None:                                    # (a live handle answers these with device work)
            out += [(lab("set_option"), g("set_option"), (h, 4 if not net else 3, 4096)),
                    (lab("profile_get"), g("profile_get"), (h, fp)),
                    (lab("counters"), lib.y355_net_counters, (h, i64)) if net else (lab("forward_counters"), lib.y355_forward_counters, (h, i64, i64)),
                    (lab("set_trackers"), g("set_trackers"), (h, fp, ip, 11) if net else (h, fp, ip)),
                    (lab("get_trackers"), g("get_trackers"), (h, fp, ip, 11) if net else (h, fp, ip))]
    return out


def cpu_calls(ffi, lib):
    calls = []
    hout = C.c_void_p()
    # ---- the two creates: null arguments, then every rule in the order it is checked
    for net in (False, True):
        name = "y355_net_create" if net else "y355_create"
        fn = getattr(lib, name)
        calls += [("%s(null cfg)" % name, fn, (None, C.byref(hout))), ("%s(null out)" % name, fn, (C.byref(_config(ffi, net)), None))]
        cases = [("height 0", dict(height=0)), ("height 100", dict(height=100)), ("width -16", dict(width=-16)), ("width 24", dict(width=24)),
                 ("anchors 0", dict(num_anchors=0)), ("anchors 17", dict(num_anchors=17)), ("classes 0", dict(num_classes=0)),
                 ("max_batch 0", dict(max_batch=0)), ("predc 16 x 25", dict(num_anchors=16, num_classes=20)),
                 ("81920 anchors", dict(height=2048, width=2048))]
        if net:
            cases += [("arch -1", dict(arch=-1)), ("arch 5", dict(arch=5)), ("dtype 2", dict(dtype=2)),
                      ("tiny, height 48", dict(arch=ffi.ARCH_TINY_V3, height=48)), ("tiny, width 16", dict(arch=ffi.ARCH_TINY_V3, width=16)),
                      ("tiny, anchors 9", dict(arch=ffi.ARCH_TINY_V3, num_anchors=9)),
                      ("yolo_v3, anchors 6", dict(arch=ffi.ARCH_YOLO_V3, num_anchors=6)),
                      ("yolo_v3, anchors 5", dict(arch=ffi.ARCH_YOLO_V3, num_anchors=5, num_classes=80)),
                      ("yolo_v3, 72828 anchors", dict(arch=ffi.ARCH_YOLO_V3, num_anchors=3, height=1088, width=1088))]
        for tag, kw in cases:
            calls.append(("%s(%s)" % (name, tag), fn, (C.byref(_config(ffi, net, **kw)), C.byref(hout))))
    # ---- the paired entry points: the null handle ...
    calls += _paired(ffi, lib, None, "null handle")
    # ... and null arrays, behind a handle that is never read (each of these checks its pointers in one condition)
    dummy = C.create_string_buffer(1 << 16)
    h = C.cast(dummy, C.c_void_p)
    for fam in ("y355_", "y355_net_"):
        net = fam == "y355_net_"
        g = lambda name: getattr(lib, fam + name)       # noqa: E731
        lab = lambda name: "%s%s(null arrays)" % (fam, name)      # noqa: E731
        calls += [(lab("overflow"), g("overflow"), (h, None)), (lab("get_candidates"), g("get_candidates"), (h, 1, None, None, None)),
                  (lab("set_normalization"), g("set_normalization"), (h, None, None)),
                  (lab("scale_boxes"), g("scale_boxes"), (h, None, None, None, 1)),
                  (lab("resize_frames"), g("resize_frames"), (h, None, 1, None)), (lab("profile_get"), g("profile_get"), (h, None)),
                  (lab("set_trackers"), g("set_trackers"), (h, None, None, 11) if net else (h, None, None)),
                  (lab("get_trackers"), g("get_trackers"), (h, None, None, 11) if net else (h, None, None))]
        if net:
            calls += [(lab("resize_u8"), g("resize_u8"), (h, None, 2, 2, 1, None)), (lab("counters"), g("counters"), (h, None))]
        else:
            calls.append((lab("forward_u8_resized"), g("forward_u8_resized"), (h, None, 2, 2, 1, 0, None, None, None, None, None)))
    st = (C.c_float(1.0), C.c_int32(1), C.c_int32(0))
    calls += [("y355_tracker_step(null)", lib.y355_tracker_step, (None, None, 1.0, 0, 0.1, None)),
              ("y355_tracker_step(max 0)", lib.y355_tracker_step, (C.byref(C.c_float(0.0)), C.byref(C.c_int32(0)), 0.0, 0, 0.1, C.byref(st[2]))),
              ("y355_tracker_step(max 1e-30)", lib.y355_tracker_step, (C.byref(C.c_float(0.0)), C.byref(C.c_int32(0)), 1e-30, 0, 0.1, C.byref(st[2]))),
              ("y355_tracker_step(ok)", lib.y355_tracker_step, (C.byref(st[0]), C.byref(st[1]), 2.0, 0, 0.1, C.byref(st[2])))]
    return calls


def gpu_calls(ffi, lib, eng_h, net_h, ntrk):
    """on a live y355_engine / y355_net (int8) that have run an unprofiled forward; the profile_get records come last (their
    failed HIP call stays the thread's last error until somebody reads it)"""
    calls = _paired(ffi, lib, eng_h, "live", (0, 3), ("y355_",)) + _paired(ffi, lib, net_h, "live", (0, 3), ("y355_net_",))
    buf = (C.c_float * 4096)()
    calls += [("y355_forward_u8_resized(live, frame 0 x 2)", lib.y355_forward_u8_resized, (eng_h, buf, 0, 2, 1, 0, None, None, None, None, buf)),
              ("y355_net_resize_u8(live, frame 2 x 16385)", lib.y355_net_resize_u8, (net_h, buf, 2, 16385, 1, buf))]
    for opt, val in [(99, 0), (ffi.OPT_FUSE_FRONT, 2), (ffi.OPT_FUSE_PAIRS, -1), (ffi.OPT_RING_WORKGROUPS, -1), (ffi.OPT_RING_WORKGROUPS, 4097),
                     (ffi.OPT_MAX_CANDIDATES, 100), (ffi.OPT_MAX_CANDIDATES, 5000), (ffi.OPT_HEAD_ROUTE, 2)]:
        calls.append(("y355_set_option(live, %d, %d)" % (opt, val), lib.y355_set_option, (eng_h, opt, val)))
    for opt, val in [(99, 0), (ffi.NET_OPT_WORKGROUPS, 257), (ffi.NET_OPT_WORKGROUPS, -1), (ffi.NET_OPT_THIN_RESIDENT, 2),
                     (ffi.NET_OPT_MAX_CANDIDATES, 100), (ffi.NET_OPT_MAX_CANDIDATES, 5000), (ffi.NET_OPT_HEAD_ROUTE, -1)]:
        calls.append(("y355_net_set_option(live, %d, %d)" % (opt, val), lib.y355_net_set_option, (net_h, opt, val)))
    mean, bad = (C.c_float * 3)(0.4, 0.4, 0.4), (C.c_float * 3)(0.2, 0.0, 0.2)
    calls += [("y355_set_normalization(live, std 0)", lib.y355_set_normalization, (eng_h, mean, bad)),
              ("y355_net_set_normalization(live, std 0)", lib.y355_net_set_normalization, (net_h, mean, bad))]
    scale, first = (C.c_float * (ntrk + 1))(*([1.0] * (ntrk + 1))), (C.c_int32 * (ntrk + 1))(*([1] * (ntrk + 1)))
    zero, huge = (C.c_float * ntrk)(*([0.0] * ntrk)), (C.c_float * ntrk)(*([1e30] * ntrk))
    for n in (ntrk - 1, ntrk + 1):
        calls += [("y355_net_set_trackers(live, n %+d)" % (n - ntrk), lib.y355_net_set_trackers, (net_h, scale, first, n)),
                  ("y355_net_get_trackers(live, n %+d)" % (n - ntrk), lib.y355_net_get_trackers, (net_h, scale, first, n))]
    calls += [("y355_net_set_trackers(live, scale 0)", lib.y355_net_set_trackers, (net_h, zero, first, ntrk)),
              ("y355_net_set_trackers(live, scale 1e30)", lib.y355_net_set_trackers, (net_h, huge, first, ntrk)),
              ("y355_profile_get(live, unprofiled)", lib.y355_profile_get, (eng_h, C.cast(buf, C.POINTER(C.c_float)))),
              ("y355_net_profile_get(live, unprofiled)", lib.y355_net_profile_get, (net_h, C.cast(buf, C.POINTER(C.c_float))))]
    return calls


def live_handles():
    """(Engine, Net) -- SlimYOLOv2 int8, 96 x 96, max_batch 2, synthetic weights, calibrated, one unprofiled forward run"""
    from oracle import yolo_oracle as O
    from yolo355 import prep, synth
    from yolo355.engine import Engine
    from yolo355.netengine import Net
    eng = Engine([SIZE, SIZE], CLASSES, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=BATCH)
    eng.load_quantized(O.quantize_layers(synth.make_weights(seed=2, num_classes=CLASSES, pred_gain=400.0, obj_bias=-4.0)))
    x = synth.make_images(3, BATCH, SIZE, SIZE, "blocks")
    eng.calibrate(x, [prep.RangeTracker() for _ in range(11)])
    eng.forward(x)
    net = Net("slim_yolo_v2", [SIZE, SIZE], CLASSES, synth.ANCHOR_SIZE_MASK, 0.01, 0.5, max_batch=BATCH, dtype="int8")
    for i, q in enumerate(prep.quantize_folded(folded_layers(synth.make_fp32_model("slim_yolo_v2", 5, CLASSES, 5)))):
        net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
    net.calibrate(x)
    net.forward(x)
    return eng, net


def folded_layers(layers, eps=1e-5):
    """[(W fp32, b fp32)] of synth.make_fp32_model's layers with their batch norm folded in"""
    import numpy as np
    out = []
    for L in layers:
        w, b = L["w"].astype(np.float64), L["b"].astype(np.float64)
        if L["bn"] is not None:
            g, be, mu, var = (a.astype(np.float64) for a in L["bn"])
            s = g / np.sqrt(var + eps)
            w, b = w * s[:, None, None, None], (b - mu) * s + be
        out.append((w.astype(np.float32), b.astype(np.float32)))
    return out


def drain_last_error(lib, eng):
    """y355_profile_get on events never recorded leaves HIP's per-thread last error set; the next launch that checks
    hipGetLastError (torch's included) would report it.  One checked launch on the engine's own output buffers takes it; a
    second one must be clean."""
    boxes, scores, _, count = eng._buffers(1)
    args = (eng._h, boxes.data_ptr(), count.data_ptr(), scores.data_ptr(), 1)         # (any floats serve as sizes here)
    lib.y355_scale_boxes(*args)
    assert lib.y355_scale_boxes(*args) == 0


def run(lib, calls):
    return [_answer(lib, label, fn, *args) for label, fn, args in calls]


def main():
    from yolo355 import _ffi
    args = [a for a in sys.argv[1:] if a != "--gpu"]
    out = args[0] if args else os.path.join(HERE, "c_abi_parent.json")
    lib = _ffi.lib()
    if "--gpu" in sys.argv:
        with open(out) as f:
            doc = json.load(f)
        eng, net = live_handles()
        doc["gpu_records"] = run(lib, gpu_calls(_ffi, lib, eng._h, net._h, net.num_trackers))
        drain_last_error(lib, eng)
        eng.close()
        net.close()
    else:
        commit = os.environ.get("Y355_GOLDEN_COMMIT")
        if not commit:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        doc = {"commit": commit, "symbols": symbols(_ffi.LIB_PATH), "records": run(lib, cpu_calls(_ffi, lib))}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "with", len(doc["symbols"]), "symbols,", len(doc["records"]), "records,", len(doc.get("gpu_records", [])), "gpu records")


if __name__ == "__main__":
    main()
