"""Measurements of profiles/r14_engine_frame_list_notes.md: the ragged resize stage on a q_bf engine (y355_resize_frames) at
416 x 416 with max_batch 64 on the two lists of profiles/r13_frame_list_notes.md (64 frames of 480 x 640; 64 frames of 20
VOC-like sizes), and Pipeline.forward_frame_list on 1024 frames beside the same pipeline on uint8 frames already at the
network size (the ceiling without a resize).  HIP events on the engine's stream, warm, 31 repeats.
    python scratch/measure_engine_frame_list.py [repeats]
The same-run A/B of the notes alternated this loop call by call between the byte-gather kernel of the commit before and the
row-staged kernel, both selectable through y355_launch_resize_frames while the change was developed; the tree keeps one."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "yolo-compression-and-deployment-in-fpga_amd")):
    sys.path.insert(0, p)

from oracle import yolo_oracle as O                    # noqa: E402
from oracle.resize_oracle import resize_linear_u8      # noqa: E402
from yolo355 import _ffi, prep, synth                  # noqa: E402
from yolo355.engine import Engine, Pipeline            # noqa: E402

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 31
SIZE, B = [416, 416], 64
KINDS = [(375, 500), (500, 375), (333, 500), (500, 333), (374, 500), (500, 334), (357, 500), (281, 500), (500, 400), (400, 500),
         (332, 500), (375, 499), (480, 640), (500, 486), (366, 500), (345, 500), (500, 302), (442, 500), (319, 480), (96, 131)]


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def desc(v):
    v = np.asarray(v)
    return "median %.1f us (min %.1f, q1 %.1f, q3 %.1f, max %.1f)" % (np.median(v), v.min(), np.percentile(v, 25), np.percentile(v, 75), v.max())


def frame_array(tensors):
    arr = (_ffi.Frame * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i].data_dev, arr[i].height, arr[i].width, arr[i].row_bytes = t.data_ptr(), int(t.shape[0]), int(t.shape[1]), 0
    return arr


def main():
    lib = _ffi.lib()
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0))
    calib = synth.normalize_frames(resize_linear_u8(synth.make_frames_u8(77, 1, 300, 400, "blocks"), SIZE[0], SIZE[1]))
    eng = Engine(SIZE, 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.05, max_batch=B)
    eng.load_quantized(ql)
    eng.calibrate(calib, [prep.RangeTracker() for _ in range(11)])
    block = torch.from_numpy(synth.make_frames_u8(7, B, 480, 640, "blocks")).cuda()
    sizes = [KINDS[i % len(KINDS)] for i in range(B)]
    mix = [torch.from_numpy(synth.make_frames_u8(100 + i, 1, h, w, "blocks")[0]).cuda() for i, (h, w) in enumerate(sizes)]
    lists = {"64 x 480x640": [block[i] for i in range(B)], "64 frames of 20 VOC-like sizes": mix}
    out = torch.empty((B, SIZE[0], SIZE[1], 3), dtype=torch.uint8, device="cuda:0")
    print("the stage on a q_bf engine, %d x %d, max_batch %d, %d repeats" % (SIZE[0], SIZE[1], B, REP))
    for name, tensors in lists.items():
        arr = frame_array(tensors)
        nbytes = sum(int(t.numel()) for t in tensors) + B * SIZE[0] * SIZE[1] * 3

        def run():
            _ffi.check(lib.y355_resize_frames(eng._h, arr, B, out.data_ptr()))
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        ref = resize_linear_u8(tensors[-1].cpu().numpy(), SIZE[0], SIZE[1])
        print("  %s: last frame equals the oracle: %s" % (name, np.array_equal(out[B - 1].cpu().numpy(), ref)))
        t = [event_us(run) for _ in range(REP)]
        print("  %s: %s; %.1f MB -> %.0f GB/s" % (name, desc(t), nbytes / 1e6, nbytes / np.median(t) / 1e3))
    eng.close()
    # ---- the pipeline on 1024 VOC-like frames beside the same pipeline on uint8 frames at the network size (not gating)
    pipe = Pipeline(SIZE, 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.05, max_batch=B)
    pipe.load_quantized(ql)
    pipe.calibrate(calib, [prep.RangeTracker() for _ in range(11)])
    n = 1024
    frames = [mix[i % B] for i in range(n)]
    at_size = torch.from_numpy(np.stack([resize_linear_u8(mix[i].cpu().numpy(), SIZE[0], SIZE[1]) for i in range(B)])).cuda()
    at_size = at_size.repeat(n // B, 1, 1, 1).contiguous()
    a = pipe.forward_frame_list(frames)
    b = pipe.forward(at_size, frames=True)
    same = all(np.array_equal(s, t) for u, v in zip(a, b) for s, t in zip(u, v))
    print("pipeline, %d handles, %d CUDA frames: detections of the two routes identical: %s (%d detections)"
          % (pipe.handles, n, same, sum(len(d[1]) for d in a)))

    def wall(fn, rep=7):
        v = []
        for _ in range(rep):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append(time.perf_counter() - t0)
        return np.asarray(v)
    tl = wall(lambda: pipe.forward_frame_list(frames))
    ts = wall(lambda: pipe.forward(at_size, frames=True))
    for label, v in (("forward_frame_list (20 sizes, resize on the GPU)", tl), ("forward(frames=True) at the network size (ceiling)", ts)):
        print("  %-52s: median %.0f images/s (min %.0f, max %.0f), %d runs, wall clock with the collect"
              % (label, n / np.median(v), n / v.max(), n / v.min(), len(v)))
    pipe.close()


if __name__ == "__main__":
    main()
