"""Every entry point that ends in the shared result collector gives the same lists, bit for bit: Engine.forward /
forward_frames / forward_frame_list / forward_scaled and Pipeline.forward / forward_frame_list / submit_batch on the same
three 96x96 frames (the pipeline with max_batch 2: two tickets, the chunk path)."""
import numpy as np
import pytest

from oracle import yolo_oracle as O
from yolo355 import _handle, synth
from yolo355.prep import RangeTracker

pytestmark = pytest.mark.gpu

H = W = 96
WH = [[640, 480], [320, 240], [96, 96]]


@pytest.fixture(scope="module")
def rig():
    from yolo355.engine import Engine, Pipeline
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=2, pred_gain=400.0, obj_bias=-4.0))
    frames = synth.make_frames_u8(11, 3, H, W, "blocks")
    x = synth.normalize_frames(frames)
    eng = Engine([H, W], 2, synth.ANCHOR_SIZE_MASK, max_batch=3)
    eng.load_quantized(ql)
    sa = eng.calibrate(x[:1], [RangeTracker() for _ in range(11)])
    pipe = Pipeline([H, W], 2, synth.ANCHOR_SIZE_MASK, max_batch=2)
    pipe.load_quantized(ql)
    assert pipe.calibrate(x[:1], [RangeTracker() for _ in range(11)]) == sa
    yield eng, pipe, frames, x
    pipe.close()
    eng.close()


def _same(ref, got, what):
    assert len(got) == len(ref) == 3, what
    for i, (a, b) in enumerate(zip(ref, got)):
        for field, u, v in zip(("boxes", "scores", "cls"), a, b):
            assert u.dtype == v.dtype and np.array_equal(u, v), (what, i, field)


@pytest.mark.parametrize("find", [False, True])
def test_plain_entry_points_agree(rig, find):
    """find=True is clean on these weights: the guard path must give the same lists and not raise"""
    eng, pipe, frames, x = rig
    ref = eng.forward(x)
    assert any(len(s) for _, s, _ in ref), "no detection at all: the comparison would be vacuous"
    assert all(b.shape == (len(s), 4) and c.dtype == np.int64 and b.flags.owndata for b, s, c in ref)
    if find:
        _same(ref, eng.forward(x, find=True), "forward(find)")
    _same(ref, eng.forward_frames(frames, find=find), "forward_frames")
    _same(ref, eng.forward_frame_list(list(frames), find=find), "forward_frame_list")
    _same(ref, pipe.forward(x, find=find), "Pipeline.forward")
    _same(ref, pipe.forward_frame_list(list(frames), find=find), "Pipeline.forward_frame_list")


def test_scaled_entry_points_agree(rig):
    eng, pipe, frames, x = rig
    plain = eng.forward(x)
    ref = eng.forward_scaled(x, WH)
    assert any(len(s) for _, s, _ in ref)
    for (pb, ps, pc), (rb, rs, rc) in zip(plain, ref):                   # the rescale touches the boxes only
        assert rb.shape == pb.shape and np.array_equal(rs, ps) and np.array_equal(rc, pc)
    assert any(len(s) and not np.array_equal(rb, pb) for (pb, _, _), (rb, s, _) in zip(plain[:2], ref[:2]))
    _same(ref, eng.forward_scaled(frames, WH, frames=True), "forward_scaled(frames)")
    _same(ref, eng.forward_frame_list(list(frames), sizes_wh=WH), "forward_frame_list(sizes_wh)")
    _same(ref, pipe.forward(x, sizes_wh=WH), "Pipeline.forward(sizes_wh)")
    tickets, wh = pipe.submit_batch(x, WH)                # two tickets: a chunk of 2 and a chunk of 1
    assert len(tickets) == 2 and tuple(wh.shape) == (3, 2)
    _same(ref, [d for t in tickets for d in pipe.fetch(t)], "Pipeline.submit_batch")
    with pytest.raises(ValueError, match="sizes_wh has 2 rows for a batch of 3"):
        eng.forward_scaled(x, WH[:2])
    with pytest.raises(ValueError, match="sizes_wh has 2 rows for a batch of 3"):
        pipe.submit_batch(x, WH[:2])


def test_handles_carry_what_callers_reach_for(rig):
    """the instance attributes of tests/golden/python_api_parent.json, on live handles; owners are closed at exit, views not"""
    eng, pipe, _, _ = rig
    view = pipe.engine(0)
    assert eng._h is not None and eng._lib is pipe._lib and eng._stream is not None and pipe._h is not None
    assert view._stream is pipe.stream(0) and view._h.value == pipe._lib.y355_pipeline_engine(pipe._h, 0)
    assert eng in _handle._live and pipe in _handle._live and view not in _handle._live
    view.close()                                          # a view lets go of the handle without destroying it
    assert view._h is None and pipe.engine(0).counters() is not None
