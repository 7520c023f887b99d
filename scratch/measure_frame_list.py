"""Measurements of profiles/r13_frame_list_notes.md: the ragged resize stage (y355_net_resize_frames) against the
same-size stage (y355_net_resize_u8), the stage on a VOC-like mix of sizes, forward_frame_list against single-frame
calls, and a caller whose frame size alternates.  HIP events on the net's stream, warm, medians.
    python scratch/measure_frame_list.py [repeats]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from cases import synth_state_dict                     # noqa: E402
from yolo355 import _ffi, synth                        # noqa: E402
from yolo355.models.tiny_yolo_v3 import YOLOv3tiny     # noqa: E402

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 31
SIZE, B = [416, 416], 64


def events(fn, rep):
    """GPU milliseconds of rep single calls of fn (one event pair each)"""
    out = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return np.array(out)


def wall(fn, rep):
    out = []
    for _ in range(rep):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return np.array(out)


def desc(v):
    return "median %.1f us (min %.1f, q1 %.1f, q3 %.1f, max %.1f)" % tuple(1e3 * x for x in (np.median(v), v.min(), np.percentile(v, 25),
                                                                                        np.percentile(v, 75), v.max()))


def main():
    m = YOLOv3tiny("cuda:0", input_size=SIZE, num_classes=3, trainable=False, conf_thresh=0.02, nms_thresh=0.5,
                   anchor_size=synth.TINY_MULTI_ANCHOR_SIZE)
    m.load_state_dict(synth_state_dict(m.state_dict(), 5, weight_gain=2.0))
    m.eval()
    m.forward_batch(torch.from_numpy(synth.make_images(21, B, SIZE[0], SIZE[1], "blocks")), quantization=True)
    net = m._get_net(B, int8=True)
    lib = _ffi.lib()
    # ---- 1. homogeneous batch: 64 frames of 480 x 640 -> 416 x 416
    block = torch.from_numpy(synth.make_frames_u8(7, B, 480, 640, "blocks")).cuda()
    out = torch.empty((B, SIZE[0], SIZE[1], 3), dtype=torch.uint8, device="cuda:0")
    out2 = torch.empty_like(out)
    arr = (_ffi.Frame * B)()
    for i in range(B):
        arr[i].data_dev, arr[i].height, arr[i].width, arr[i].row_bytes = block[i].data_ptr(), 480, 640, 0

    def parent():
        _ffi.check(lib.y355_net_resize_u8(net._h, block.data_ptr(), 480, 640, B, out.data_ptr()))

    def ragged():
        _ffi.check(lib.y355_net_resize_frames(net._h, arr, B, out2.data_ptr()))
    for _ in range(5):
        parent()
        ragged()
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    tp, tr = [], []
    for _ in range(REP):                                # interleaved
        tp.append(events(parent, 1)[0])
        tr.append(events(ragged, 1)[0])
    tp, tr = np.array(tp), np.array(tr)
    print("1. 64 x 480x640 -> 416x416, %d interleaved repeats" % REP)
    print("   y355_net_resize_u8     (same-size stage): " + desc(tp))
    print("   y355_net_resize_frames (ragged stage):    " + desc(tr))
    print("   spread of the same-size stage between its own repeats: max - min %.1f us, q3 - q1 %.1f us; ragged median - same-size median %+.1f us"
          % (1e3 * (tp.max() - tp.min()), 1e3 * (np.percentile(tp, 75) - np.percentile(tp, 25)), 1e3 * (np.median(tr) - np.median(tp))))
    # ---- 2. VOC-like mix: 64 frames of 20 distinct sizes around 500 x 375
    rng = np.random.default_rng(0)
    kinds = [(375, 500), (500, 375), (333, 500), (500, 333), (374, 500), (500, 334), (357, 500), (281, 500), (500, 400), (400, 500),
             (332, 500), (375, 499), (480, 640), (500, 486), (366, 500), (345, 500), (500, 302), (442, 500), (319, 480), (96, 131)]
    sizes = [kinds[i % len(kinds)] for i in range(B)]
    frames = [synth.make_frames_u8(100 + i, 1, h, w, "blocks")[0] for i, (h, w) in enumerate(sizes)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    arr2 = (_ffi.Frame * B)()
    for i, d in enumerate(dev):
        arr2[i].data_dev, arr2[i].height, arr2[i].width, arr2[i].row_bytes = d.data_ptr(), sizes[i][0], sizes[i][1], 0

    def mix():
        _ffi.check(lib.y355_net_resize_frames(net._h, arr2, B, out2.data_ptr()))
    for _ in range(5):
        mix()
    tm = events(mix, REP)
    nbytes = sum(h * w * 3 for h, w in sizes) + B * SIZE[0] * SIZE[1] * 3
    print("2. ragged stage on 64 frames of %d distinct sizes: %s; %.1f MB read + written -> %.1f GB/s"
          % (len(set(sizes)), desc(tm), nbytes / 1e6, nbytes / (np.median(tm) * 1e-3) / 1e9))
    # ---- 3. forward_frame_list against 64 single-frame forward_frames calls (host frames, wall clock with the collect)
    def one_list():
        return net.forward_frame_list(frames)

    def singles():
        return [net.forward_frames(f[None])[0] for f in frames]
    a, b = one_list(), singles()
    for u, v in zip(a, b):
        assert all(np.array_equal(s, t) for s, t in zip(u, v))
    rep3 = max(5, REP // 3)
    tl, ts = wall(one_list, rep3), wall(singles, rep3)
    print("3. YOLOv3tiny int8 416x416, the same 64 host frames, wall clock incl. upload and collect, %d repeats" % rep3)
    print("   forward_frame_list (one call):       median %.2f ms (min %.2f, max %.2f)" % (np.median(tl), tl.min(), tl.max()))
    print("   64 forward_frames calls (B = 1 each): median %.2f ms (min %.2f, max %.2f)" % (np.median(ts), ts.min(), ts.max()))
    # ---- 4. a caller whose frame size alternates: 32 frames of 480x640, then 32 of 375x500, ...
    fa = torch.from_numpy(synth.make_frames_u8(8, 32, 480, 640, "blocks")).cuda()
    fb = torch.from_numpy(synth.make_frames_u8(9, 32, 375, 500, "blocks")).cuda()
    la, lb = [fa[i] for i in range(32)], [fb[i] for i in range(32)]

    def alt_parent():
        for _ in range(4):
            net.forward_frames_device(fa)
            net.forward_frames_device(fb)

    def same_parent():
        for _ in range(8):
            net.forward_frames_device(fa)

    def alt_list():
        for _ in range(4):
            net.forward_frame_list_device(la)
            net.forward_frame_list_device(lb)
    for f in (alt_parent, same_parent, alt_list):
        f()
    t1, t2, t3 = wall(alt_parent, rep3), wall(same_parent, rep3), wall(alt_list, rep3)
    print("4. 8 forwards of 32 CUDA frames queued back to back, wall clock per forward, %d repeats" % rep3)
    print("   forward_frames_device, sizes alternating (a table rebuild and a stream synchronisation per call): median %.3f ms" % (np.median(t1) / 8))
    print("   forward_frames_device, one size throughout:                                                      median %.3f ms" % (np.median(t2) / 8))
    print("   forward_frame_list_device, sizes alternating:                                                    median %.3f ms" % (np.median(t3) / 8))


if __name__ == "__main__":
    main()
