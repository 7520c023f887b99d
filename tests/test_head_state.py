"""The host state of the detection head and of the frame stage (csrc/head_state.hip, csrc/resize.hip), seen through the
three callers that share it: Engine (y355_engine), Net (y355_net) and engine.head_f32 (y355_head_f32_ex).

A walk of the candidate capacity and the head route must leave max_det / max_candidates at the values the handles reported
before the state had one owner (the literals of WALK, recorded from that commit: the walks pass there as they stand) and must
never change what a fixed input with fewer than 4096 candidates gives.  A rejected set_normalization must leave the handle as it was."""
import numpy as np
import pytest

import head_large_cases as LC

# (setter, value) -> (max_det, max_candidates) afterwards, for a head with more than 8192 anchors per image and max_det unset
WALK = [(None, None, (4096, 4096)),
        ("cap", 8192, (8192, 8192)),
        ("route", 1, (8192, 8192)),
        ("cap", 4096, (4096, 4096)),
        ("route", 0, (4096, 4096))]
# the same for a head with N <= 4096 anchors (here N = 180): the capacity cannot leave 4096, max_det is N throughout
WALK_SMALL = [(None, None, (180, 4096)), ("route", 1, (180, 4096)), ("route", 0, (180, 4096))]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x[1]) == len(y[1]), (i, len(x[1]), len(y[1]))
        for k in range(3):
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (i, k)


def _pred_q(seed, B, A, C, Hs, Ws, n_on):
    """int8 prediction map [B, A (5 + C), Hs, Ws] at exponent 4: objectness -7.9 except on n_on anchors per image (3.75)"""
    rng = np.random.RandomState(seed)
    pq = rng.randint(-40, 41, size=(B, A * (5 + C), Hs, Ws)).astype(np.int8)
    obj = np.full((B, A * Hs * Ws), -127, np.int8)
    for b in range(B):
        obj[b, rng.permutation(A * Hs * Ws)[:n_on]] = 60
    pq[:, :A] = obj.reshape(B, A, Hs, Ws)
    return pq


def _walk(handle, run, walk):
    from yolo355._ffi import Y355Error
    first = None
    for what, value, (max_det, max_cand) in walk:
        if what == "cap":
            handle.set_max_candidates(value)
        elif what == "route":
            handle.set_head_route(value)
        print(what, value, "-> max_det", handle.max_det, "max_candidates", handle.max_candidates)
        assert (handle.max_det, handle.max_candidates) == (max_det, max_cand), (what, value)
        dets = run()
        assert all(0 < len(d[1]) < 4096 for d in dets)
        if first is None:
            first = dets
        _same(dets, first)
    n = handle.num_anchors_total
    for bad in (4095, n + 1):                       # a refused value changes nothing
        with pytest.raises(Y355Error, match="4096 .. min"):
            handle.set_max_candidates(bad)
        assert (handle.max_det, handle.max_candidates) == walk[-1][2]
    _same(run(), first)


@pytest.mark.gpu
@pytest.mark.parametrize("size,walk", [([96, 96], WALK_SMALL), ([512, 1024], WALK)], ids=["N180", "N10240"])
def test_capacity_and_route_walk_on_the_engine(size, walk):
    from yolo355 import synth
    from yolo355.engine import Engine
    C, B = 2, 2
    Hs, Ws = size[0] // 16, size[1] // 16
    pq = _pred_q(3, B, 5, C, Hs, Ws, min(300, Hs * Ws * 5 // 2))
    eng = Engine(size, C, synth.ANCHOR_SIZE_MASK, conf_thresh=0.05, nms_thresh=0.5, max_batch=B)
    try:
        assert eng.num_anchors_total == Hs * Ws * 5
        _walk(eng, lambda: eng.head_nms(pq, 4), walk)
    finally:
        eng.close()


@pytest.mark.gpu
def test_capacity_and_route_walk_on_a_net():
    """YOLOv3tiny, bf16, 640 x 1024: (40 x 64 + 20 x 32) x 3 = 9600 anchors per image"""
    import torch
    from cases import synth_state_dict
    from yolo355 import synth
    from yolo355.models.tiny_yolo_v3 import YOLOv3tiny
    size, C = [640, 1024], 3
    m = YOLOv3tiny("cuda:0", input_size=size, num_classes=C, trainable=False, conf_thresh=0.02, nms_thresh=0.5,
                   anchor_size=synth.TINY_MULTI_ANCHOR_SIZE)
    m.load_state_dict(synth_state_dict(m.state_dict(), 5, weight_gain=2.0))
    m.eval()
    x = torch.from_numpy(synth.normalize_frames(synth.make_frames_u8(21, 1, size[0], size[1], "blocks")))
    net = m._get_net(1, int8=False)
    try:
        assert net.num_anchors_total == 9600
        net.set_thresholds(0.0, 0.5)
        net.set_max_candidates(9600)
        net.forward(x, tap=True)
        conf = float(np.sort(net.candidates(1)[1].reshape(-1))[-500])       # about 500 candidates
        net.set_max_candidates(4096)
        net.set_thresholds(conf, 0.5)
        _walk(net, lambda: net.forward(x), WALK)
    finally:
        net.close()


@pytest.mark.gpu
def test_capacity_and_route_on_head_f32():
    """y355_head_f32_ex builds and drops its state per call: every capacity and route gives the first call's bytes, on a head
    of 10647 anchors (300 candidates per image) and on its 13 x 13 level alone (N = 507)"""
    from yolo355 import engine as E
    case = LC.h4_variant(300)
    A = case["A"]
    anchors = np.asarray(case["anchors"], np.float32).reshape(len(case["strides"]), A, 2)

    def head(levels, **kw):
        return E.head_f32([case["preds"][l] for l in levels], [case["strides"][l] for l in levels], anchors[levels], case["C"], case["size"],
                          1.0, case["conf"], 0.5, **kw)
    first = head([0, 1, 2])
    assert all(0 < len(d[1]) < 4096 for d in first)
    for cap, route in [(4096, 0), (8192, 0), (8192, 1), (4096, 1), (10647, 0), (4096, 0)]:
        _same(head([0, 1, 2], max_candidates=cap, route=route), first)
    got = head([0, 1, 2], max_candidates=8192, max_det=5)
    _same(got, [tuple(r[:5] for r in d) for d in first])
    small = head([2])
    assert any(len(d[1]) for d in small)
    _same(head([2], route=1), small)
    _same(head([2], max_candidates=4096, route=0), small)
    with pytest.raises(E._ffi.Y355Error, match="max_candidates"):
        head([2], max_candidates=8192)


@pytest.mark.gpu
def test_rejected_normalization_leaves_the_engine_untouched():
    """std_bgr = (0, 1, 1): the first channel checked in RGB order is fine, the last is not -- no channel may change"""
    from oracle import yolo_oracle as O
    from yolo355 import synth
    from yolo355._ffi import Y355Error
    from yolo355.engine import Engine
    from yolo355.prep import RangeTracker
    H = W = 96
    eng = Engine([H, W], 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=2)
    try:
        eng.load_quantized(O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0)))
        eng.calibrate(synth.make_images(1, 1, H, W, "blocks"), [RangeTracker() for _ in range(11)])
        frames = synth.make_frames_u8(4, 2, H, W, "blocks")
        before = eng.forward_frames(frames)
        assert any(len(d[1]) for d in before)
        with pytest.raises(Y355Error, match="std must be positive"):
            eng.set_normalization((0.9, 0.1, 0.5), (0.0, 1.0, 1.0))
        _same(eng.forward_frames(frames), before)
        eng.set_normalization((0.9, 0.1, 0.5), (0.5, 1.0, 1.0))          # (an accepted call does change the outputs' inputs)
        after = eng.forward_frames(frames)
        assert any(np.asarray(a[1]).tobytes() != np.asarray(b[1]).tobytes() for a, b in zip(after, before))
    finally:
        eng.close()
