"""Times the training augmentation (yolo355.augment) on a seeded synthetic batch: 64 frames of 500 x 375 (width x height) with
a few boxes each, to 416 x 416.

    python -m yolo355.tools.augment_bench [--frames 64 --reps 15 --seed 0 --rocprof]

Prints one JSON line; every time is the median of --reps synchronous calls (one warm-up first), the fastest and slowest beside it:
  draw_ms              draw() for the batch: the reference's random stream replayed on the host, sequential Python by
                       construction -- its own row, in no total but augment_frame_list's
  apply_ms             apply() with the frames already on the device (descriptors, launches, synchronise)
  frame_list_ms        the whole augment_frame_list from host frames: draw, pinned packing, one upload, apply
  host_numpy_ms        the NumPy restatement of the same pixels (tests/augment_ref.py, when the tests directory is there) on
                       this host, and whether its batch equals the kernel's bit for bit
  kernel_ms            --rocprof: the kernel's own time per batch from a separate `rocprofv3 --kernel-trace --stats` run of
                       `--kernel-only` in a fresh process (the sum over the batch's launches, averaged over the calls)
  compulsory_bytes     from the shapes: the output batch once plus every source frame once; bound_ms at --tbps (6.29: the
                       measured copy bandwidth of an MI355X), and the share of that bound the kernel and apply reach
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

SIZE = (416, 416)
FRAME_HW = (375, 500)


def synthetic(seed, n):
    """(frames uint8 [375,500,3], targets float64 [k,5] with 1..4 boxes)"""
    rs = np.random.RandomState(seed)
    frames, targets = [], []
    for _ in range(n):
        frames.append(rs.randint(0, 256, FRAME_HW + (3,)).astype(np.uint8))
        k = int(rs.randint(1, 5))
        c, half = rs.uniform(0.2, 0.8, (k, 2)), rs.uniform(0.05, 0.35, (k, 2))
        targets.append(np.hstack((np.clip(c - half, 0, 1), np.clip(c + half, 0, 1), rs.randint(0, 20, (k, 1)).astype(np.float64))))
    return frames, targets


def timed(fn, reps, sync=None):
    ts = []
    for _ in range(reps + 1):                                               # one warm-up
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]
    return 1e3 * statistics.median(ts), [1e3 * min(ts), 1e3 * max(ts)]


def kernel_time_ms(argv_tail, calls):
    """the separate rocprofv3 run: a fresh process, the program after `--`"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, "-m", "yolo355.tools.augment_bench",
               "--kernel-only"] + argv_tail
        pkg = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
        env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if r.returncode != 0:
            raise RuntimeError("rocprofv3 run failed: " + r.stderr[-2000:])
        total, launches = 0, 0
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                if "augment_kernel" in row["Name"]:
                    total += int(row["TotalDurationNs"])
                    launches += int(row["Calls"])
        if not launches:
            raise RuntimeError("no augment_kernel row in rocprofv3's kernel stats")
        return total / 1e6 / calls, launches // calls


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tbps", type=float, default=6.29, help="the bandwidth the bound is stated against, TB/s")
    ap.add_argument("--rocprof", action="store_true", help="add kernel_ms from a separate rocprofv3 run")
    ap.add_argument("--kernel-only", action="store_true", help="only --reps applies from device frames (what --rocprof profiles)")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy restatement")
    a = ap.parse_args(argv)
    import torch
    from yolo355 import augment as A
    frames, targets = synthetic(a.seed, a.frames)
    sizes = [f.shape[:2] for f in frames]
    params, _ = A.draw_list(sizes, targets, rng=np.random.RandomState(a.seed))
    dev = [torch.from_numpy(f).to("cuda:0") for f in frames]
    out = torch.empty((a.frames, 3) + SIZE, dtype=torch.float32, device="cuda:0")
    sync = torch.cuda.synchronize
    if a.kernel_only:
        for _ in range(a.reps):
            A.apply(dev, params, SIZE, out=out)
        sync()
        return None
    res = dict(frames=a.frames, frame_hw=list(FRAME_HW), size=list(SIZE), reps=a.reps, seed=a.seed, chunk=A.chunk())
    res["draw_ms"], res["draw_ms_min_max"] = timed(lambda: A.draw_list(sizes, targets, rng=np.random.RandomState(a.seed)), a.reps)
    res["apply_ms"], res["apply_ms_min_max"] = timed(lambda: A.apply(dev, params, SIZE, out=out), a.reps, sync)
    res["frame_list_ms"], res["frame_list_ms_min_max"] = timed(
        lambda: A.augment_frame_list(frames, targets, SIZE, rng=np.random.RandomState(a.seed), out=out), a.reps, sync)
    res["virtual_pixels"] = int(sum(p.vh * p.vw for p in params))
    nbytes = out.numel() * 4 + sum(f.size for f in frames)
    bound_ms = nbytes / (a.tbps * 1e12) * 1e3
    res.update(compulsory_bytes=int(nbytes), tbps=a.tbps, bound_ms=bound_ms, apply_share_of_bound=bound_ms / res["apply_ms"])
    tests = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "tests"))
    if not a.no_host and os.path.exists(os.path.join(tests, "augment_ref.py")):
        sys.path.insert(0, tests)
        import augment_ref as R
        t0 = time.perf_counter()
        ref = R.batch(frames, params, SIZE, A.MEAN, A.STD)
        res["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)              # once: it takes seconds
        got = A.apply(dev, params, SIZE).cpu().numpy()
        fin = np.isfinite(ref)
        res["equals_host_numpy"] = bool(np.array_equal(fin, np.isfinite(got)) and np.array_equal(got.view(np.uint32)[fin], ref.view(np.uint32)[fin]))
    if a.rocprof:
        tail = ["--frames", str(a.frames), "--reps", str(a.reps), "--seed", str(a.seed)]
        res["kernel_ms"], res["launches_per_batch"] = kernel_time_ms(tail, a.reps)
        res["kernel_share_of_bound"] = bound_ms / res["kernel_ms"]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
