"""TEST INFRASTRUCTURE -- the cases of tests/test_net_shared_gpu.py (y355_net handles that share the GPU, as bench.py's
measure_net runs them), what the table must reach restated on the CPU, and the small helpers of those tests.

A contention hazard needs workgroups of two handles resident on one CU at the same time, which needs launches with at least as
many work items as the device has compute units (CUS, 256 on an MI355X).  The stride-32 level has the fewest: tile 5 and ring I4
give 4 items per image on a 13 x 13 map (B = 64), ring I5 gives 2 (B = 128, bench.py's own batch for YOLOv3tiny).  work_items()
recomputes the counts from int8_tile_cases.G_TILES / RINGS and predict() the way run_op (csrc/net.hip) and the ring launchers
(csrc/convr.hip) count them: tiles_x * tiles_y * (cout_pad / bn) per image.

Two rows are here beyond the eight the issue behind this module lists: slim_i8_c2 and spp_i8.  With them the int8 rows reach
every (family, tile) a deployed net selects; without them tile 6 (SlimYOLOv2's prediction layer with 2 classes) and tile 10
(the 1 x 1 behind YOLOv3-SPP's pooling block) would run beside no second handle.
"""
import numpy as np

import int8_tile_cases as T
import net_calib_ref as R

CUS = 256
# (tag, arch, dtype, [H, W], B = max_batch, handles, P (period of the batch), rounds, row of int8_tile_cases or None)
CASES = [
    ("tiny_i8", "tiny_yolo_v3", "int8", [416, 448], 128, 3, 2, 40, "tiny_448_mb64"),
    ("slim_bf16", "slim_yolo_v2", "bf16", [416, 416], 64, 3, 2, 40, None),
    ("slim_i8", "slim_yolo_v2", "int8", [416, 448], 64, 3, 2, 40, "slim_448_mb64_c20"),
    ("slim_i8_c2", "slim_yolo_v2", "int8", [416, 448], 64, 3, 2, 40, "slim_448_mb64"),
    ("tiny_bf16", "tiny_yolo_v3", "bf16", [416, 416], 128, 3, 2, 40, None),
    ("v2_i8", "yolo_v2", "int8", [416, 416], 64, 2, 2, 12, "v2_416_mb64"),
    ("v2_bf16", "yolo_v2", "bf16", [416, 416], 64, 2, 2, 12, None),
    ("v3_i8", "yolo_v3", "int8", [416, 448], 64, 2, 1, 12, "v3_448_mb64"),
    ("v3_bf16", "yolo_v3", "bf16", [416, 416], 64, 2, 1, 12, None),
    ("spp_i8", "yolo_v3_spp", "int8", [416, 416], 64, 2, 1, 12, "spp_416_mb64"),
]
TAGS = [c[0] for c in CASES]
INT8_TAGS = [c[0] for c in CASES if c[2] == "int8"]
BF16_TAGS = [c[0] for c in CASES if c[2] == "bf16"]
SMALL = ("slim_yolo_v2", "tiny_yolo_v3")
DARKNET_FALLBACK = 48                       # test_int8_production_tiles._equivalent_max_batch: the same tiles in every layer
# the variants, each on the handles of a case
THROUGHPUT = ("tiny_i8", "slim_bf16", "v3_i8")          # Y355_NET_OPT_WORKGROUPS 128 and 192 (profiles/r04_notes.md), half the rounds
THROUGHPUT_WGS = (128, 192)
CALIBRATION = ("tiny_i8", "v2_i8")
FRAMES = ("tiny_i8", "slim_bf16")
FRAME_SIZE = (480, 640)


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def classes_of(tag):
    row = case(tag)[8]
    return T.case(row)[3]


def predict_row(tag, wide=(), fused_front=False, max_batch=None):
    """int8_tile_cases.predict of an int8 row on THIS table's max_batch (the selector's batch hint), or on the one given"""
    _, arch, _, size, B, _, _, _, row = case(tag)
    return T.predict(arch, size, B if max_batch is None else max_batch, T.predc_of(arch, classes_of(tag)), wide, fused_front)


def work_items(tag, wide=(), fused_front=False, max_batch=None):
    """[(items per image, family, tile or ring, layer)] of the RING and GENERIC8 layers of an int8 row's forward"""
    _, arch, _, size, B, _, _, _, row = case(tag)
    g = R.graph(arch)
    rings = {r[0]: r[1:] for r in T.RINGS}
    predc = T.predc_of(arch, classes_of(tag))
    convs = [o for o in g.ops if o["op"] == "conv"]
    out = []
    for o, e in zip(convs, predict_row(tag, wide, fused_front, max_batch)):
        if e["family"] not in (T.RING, T.GENERIC8):
            continue
        hi, wi = size[0] // g.div[o["i"]], size[1] // g.div[o["i"]]
        cp = T.cout_pad(predc if o["cout"] is None else o["cout"], e["stat"])       # (NLayer.cout_pad: padded to the generic tile's bn)
        if e["family"] == T.RING:
            _, bn, th, tw, _ = rings[e["tile"]]
            ho, wo = hi, wi
        else:
            _, bn, th, tw = T.G_TILES[e["tile"]][:4]
            ho, wo = ((hi + 1) // 2, (wi + 1) // 2) if o["s2"] else (hi, wi)
        assert cp % bn == 0, (tag, o["layer"])
        out.append((-(-ho // th) * -(-wo // tw) * (cp // bn), e["family"], e["tile"], o["layer"]))
    return out


def periodic(base, B):
    """B images: the P of `base` repeated B / P times (numpy or torch, first axis)"""
    P = base.shape[0]
    assert B % P == 0
    if isinstance(base, np.ndarray):
        return np.concatenate([base] * (B // P))
    return base.repeat(B // P, *([1] * (base.dim() - 1)))


def is_periodic(t, P):
    """every element b of the first axis equals element b mod P (torch tensor or numpy array), bytes compared"""
    import torch
    B = t.shape[0]
    if isinstance(t, np.ndarray):
        v = np.ascontiguousarray(t).view(np.uint8).reshape(B // P, P, -1)
        return bool((v == v[:1]).all())
    v = t.contiguous().view(torch.uint8).reshape(B // P, P, -1)
    return bool((v == v[:1]).all())


def same_bytes(a, b):
    """numpy arrays equal as bytes (an fp32 NaN equals itself, -0.0 differs from 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def differing(a, b):
    """how many values of two arrays of one shape differ as bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    n = a.dtype.itemsize
    return int((a.view(np.uint8).reshape(-1, n) != b.view(np.uint8).reshape(-1, n)).any(axis=1).sum())


def overlapped(spans):
    """spans: [(actor, start, end)] of one round's forwards, times on one clock.  True when two forwards of DIFFERENT actors
    were in flight at the same time (their intervals intersect in more than a point)"""
    for i, (a, s0, e0) in enumerate(spans):
        for b, s1, e1 in spans[i + 1:]:
            if a != b and max(s0, s1) < min(e0, e1):
                return True
    return False


def overlap_time(spans):
    """(time during which forwards of at least two different actors were in flight, time during which any was) of a round"""
    cuts = sorted({t for _, s, e in spans for t in (s, e)})
    both = busy = 0.0
    for lo, hi in zip(cuts, cuts[1:]):
        live = {a for a, s, e in spans if s <= lo and e >= hi}
        busy += (hi - lo) if live else 0.0
        both += (hi - lo) if len(live) > 1 else 0.0
    return both, busy
