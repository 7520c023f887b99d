"""ApEval.add is free of host synchronisation: the append is ordered behind the producer of the buffers by the stream alone --
also when that stream is torch's default stream, HIP's null stream, whose handle 0 the C ABI reads as "no producer"
(Y355_AP_NULL_STREAM names it).  Each test queues the producer, adds at once, and never waits before compute()."""
import numpy as np
import pytest

import voc_ap_ref as R
from test_voc_ap_ref import same

pytestmark = pytest.mark.gpu


def _check(ev, C, gt, boxes, scores, cls, count):
    aps, mean = ev.compute()
    ref = R.evaluate(C, gt, boxes, scores, cls, count)
    assert np.array_equal(ev.ndet, ref["ndet"]), (ev.ndet, ref["ndet"])
    assert same(aps, ref["ap"]) and mean == ref["mean"]
    for c in range(C):
        rec, prec, flag = ev.curve(c)
        assert np.array_equal(flag, ref["flag"][c]) and same(rec, ref["rec"][c]) and same(prec, ref["prec"][c]), c
    # the C ABI's own mean: the same sum in class order, at most C roundings of values <= 1 from np.mean's pairwise one
    assert abs(ev.mean_abi - mean) <= C * 2.0 ** -52


@pytest.mark.parametrize("where", ["default_stream", "side_stream", "raw_null_handle"])
def test_add_right_behind_a_producer_that_is_still_queued(where):
    """the buffers hold nothing (count 0, classes out of range) until a copy that is queued behind some tens of milliseconds of
    matrix products fills them; add() follows at once.  An append that ran ahead of the copy would count no detection."""
    import torch
    from yolo355.apeval import ApEval
    gt, boxes, scores, cls, count = R.synth_set(51, 40, 3, 25, 3)
    good = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (boxes, scores, cls, count)]
    bufs = [torch.full_like(good[0], float("nan")), torch.full_like(good[1], float("nan")), torch.full_like(good[2], 99),
            torch.zeros_like(good[3])]
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    ev = ApEval(3, gt, max_dets=int(count.sum()))
    try:
        stream = torch.cuda.Stream() if where == "side_stream" else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            for _ in range(40):
                a = (a @ a).clamp_(-1, 1)
            for b, g in zip(bufs, good):
                b.copy_(g, non_blocking=True)
            if where == "raw_null_handle":
                assert stream.cuda_stream == 0            # torch's default stream is the null stream
                ev.add(0, *bufs, after_stream=0)
            elif where == "side_stream":
                ev.add(0, *bufs, after_stream=stream)
            else:
                ev.add(0, *bufs)                          # torch's current stream
        _check(ev, 3, gt, boxes, scores, cls, count)
    finally:
        ev.close()


def test_add_the_outputs_of_engine_forward_device_without_a_wait():
    """the module docstring's usage: ev.add(first, *Engine.forward_device(x)), the engine launching on torch's default stream"""
    import torch
    from oracle import yolo_oracle as O
    from yolo355 import synth
    from yolo355.apeval import ApEval
    from yolo355.engine import Engine
    from yolo355.prep import RangeTracker
    H = W = 96
    B = 4
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0))
    eng = Engine([H, W], 2, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=B)
    eng.load_quantized(ql)
    eng.calibrate(synth.make_images(1, 1, H, W, "blocks"), [RangeTracker() for _ in range(11)])
    x = synth.make_images(3, B, H, W, "blocks")
    dets = eng.forward(x)                                 # the host's copy of the same forward: what the restatement scores
    md = eng.max_det
    boxes, scores, cls = np.zeros((B, md, 4), np.float32), np.zeros((B, md), np.float32), np.zeros((B, md), np.int32)
    count = np.array([len(d[1]) for d in dets], np.int32)
    assert count.sum() > 20
    for i, d in enumerate(dets):
        boxes[i, :count[i]], scores[i, :count[i]], cls[i, :count[i]] = d[0], d[1], d[2]
    rng = np.random.default_rng(4)
    gt = []
    for i in range(B):                                    # ground truth in the boxes' own (normalised) units, from half the detections
        k = np.flatnonzero(rng.random(count[i]) < 0.5)
        g = (boxes[i, k].astype(np.float64) + rng.normal(0, 0.01, (len(k), 4))).astype(np.float32)      # ApEval keeps float32 boxes
        gt.append(np.c_[cls[i, k], g.astype(np.float64), rng.random(len(k)) < 0.2])
    xd = torch.from_numpy(x).cuda()
    ev = ApEval(2, gt, max_dets=int(count.sum()))
    try:
        out = (torch.zeros((B, md, 4), device="cuda"), torch.zeros((B, md), device="cuda"),
               torch.zeros((B, md), dtype=torch.int32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
        eng.forward_device(xd, out=out)                   # still queued when add() is called: nothing waits in between
        ev.add(0, *out, batch=B)
        aps, mean = ev.compute(quantize=False)
        ref = R.evaluate(2, gt, boxes, scores, cls, count, quantize=False)
        assert np.array_equal(ev.ndet, ref["ndet"]) and same(aps, ref["ap"]) and mean == ref["mean"]
        assert (aps > 0).any()
    finally:
        ev.close()
        eng.close()
