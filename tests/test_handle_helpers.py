"""yolo355/_handle.py on the CPU: the result collector, the two raises, the handle base and the int8 weight marshalling that
Engine, Pipeline, Net, ConvOp and ApEval share."""
import numpy as np
import pytest
import torch

from yolo355 import _ffi, _handle as H

B, MD, COUNTS = 3, 5, [0, 5, 2]


def _outputs():
    """a forward's four outputs for B images, capacity MD; everything beyond an image's count is NaN (cls: a sentinel)"""
    rng = np.random.RandomState(7)
    boxes = rng.rand(B + 1, MD, 4).astype(np.float32)
    scores = rng.rand(B + 1, MD).astype(np.float32)
    cls = rng.randint(0, 20, (B + 1, MD)).astype(np.int32)
    count = np.array(COUNTS + [4], np.int32)              # one row more than B, as buffers sized for max_batch have
    for i, n in enumerate(COUNTS):
        boxes[i, n:], scores[i, n:], cls[i, n:] = np.nan, np.nan, -12345
    return boxes, scores, cls, count


def _parent_expression(boxes, scores, cls, n):
    return [(boxes[i, :n[i]].copy(), scores[i, :n[i]].copy(), cls[i, :n[i]].astype(np.int64)) for i in range(B)]


@pytest.mark.parametrize("as_torch", [False, True])
def test_split_dets_cuts_per_image_lists(as_torch):
    boxes, scores, cls, count = _outputs()
    want = _parent_expression(boxes[:B], scores[:B], cls[:B], count[:B])
    args = [torch.from_numpy(a) for a in (boxes, scores, cls, count)] if as_torch else [boxes, scores, cls, count]
    got = H.split_dets(*args, B)
    assert len(got) == B and [len(s) for _, s, _ in got] == COUNTS
    for (gb, gs, gc), (wb, ws, wc) in zip(got, want):
        assert np.array_equal(gb, wb) and np.array_equal(gs, ws) and np.array_equal(gc, wc)
        assert gb.shape[1:] == (4,) and gb.dtype == np.float32 and gs.dtype == np.float32 and gc.dtype == np.int64
        assert not np.isnan(gb).any() and not np.isnan(gs).any() and (gc >= 0).all()      # nothing beyond the count
        for a in (gb, gs, gc):
            assert a.flags.owndata and a.base is None
    got[1][0][:] = -1.0                                   # the lists are copies: the outputs stay as they were
    assert (boxes[1] >= 0).all()


def test_split_dets_takes_a_downloaded_count():
    """Engine / Net download the count first (that synchronises) and hand it on beside the device tensors"""
    boxes, scores, cls, count = _outputs()
    got = H.split_dets(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(cls), torch.from_numpy(count)[:B].cpu(), B)
    for (gb, gs, gc), (wb, ws, wc) in zip(got, _parent_expression(boxes, scores, cls, count)):
        assert np.array_equal(gb, wb) and np.array_equal(gs, ws) and np.array_equal(gc, wc)


def test_raise_if_guard(capsys):
    assert H.raise_if_guard(0) is None
    assert capsys.readouterr().out == ""
    with pytest.raises(AssertionError, match="3 positions") as e:
        H.raise_if_guard(3)
    assert "16-bit head-room (find=True)" in str(e.value)
    assert capsys.readouterr().out == "too high!!!\n"


def test_raise_overflow_names_max_candidates_only_above_the_default():
    with pytest.raises(_ffi.Y355Error) as e:
        H.raise_overflow(4096)
    assert "more than 4096 anchors" in str(e.value) and "or max_candidates" not in str(e.value)
    with pytest.raises(_ffi.Y355Error) as e:
        H.raise_overflow(8192)
    assert "more than 8192 anchors" in str(e.value) and "or max_candidates" in str(e.value)


class _StubLib:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def y355_stub_destroy(self, h):
        self.calls.append(h)
        if self.fail:
            raise OSError("the runtime is gone")


class _StubHandle(H.Handle):
    _destroy = "y355_stub_destroy"


def test_handle_close_destroys_once():
    lib, h = _StubLib(), _StubHandle()
    h.close()                                             # before _own (a constructor that raised): nothing to do
    h._own(lib, 41)
    assert h in H._live and (h._h, h._lib) == (41, lib)
    h.close()
    h.close()
    assert lib.calls == [41] and h._h is None


def test_handle_view_never_destroys():
    lib, h = _StubLib(), _StubHandle()
    h._own(lib, 42, owned=False)
    assert h not in H._live
    h.close()
    h.close()
    h.__del__()
    assert lib.calls == [] and h._h is None


def test_handle_del_swallows_and_exit_hook_closes(monkeypatch):
    import weakref
    monkeypatch.setattr(H, "_live", weakref.WeakSet())    # the hook below must not close other tests' handles
    lib, h = _StubLib(fail=True), _StubHandle()
    h._own(lib, 43)
    h.__del__()                                           # the destroy symbol raises: __del__ does not
    assert lib.calls == [43]
    lib2, h2 = _StubLib(), _StubHandle()
    h2._own(lib2, 44)
    H._close_all()                                        # what runs at interpreter exit: every live owning handle
    assert lib2.calls == [44] and h2._h is None


def test_every_handle_class_sits_on_the_base():
    from yolo355 import apeval, engine, netengine, ops
    for cls, sym in ((engine.Engine, "y355_destroy"), (engine.Pipeline, "y355_pipeline_destroy"), (ops.ConvOp, "y355_conv_op_destroy"),
                     (netengine.Net, "y355_net_destroy"), (apeval.ApEval, "y355_apeval_destroy")):
        assert issubclass(cls, H.Handle) and cls._destroy == sym and sym in _ffi.declared_symbols()
        assert "close" not in vars(cls) and "__del__" not in vars(cls)
    assert engine.ConvOp is ops.ConvOp
    for cls in (engine.Engine, netengine.Net):
        assert issubclass(cls, H.StreamBound) and "_call" not in vars(cls) and "_enter" not in vars(cls)


def test_i8_layer_checks_the_callers_array():
    ok = np.arange(-127, 128, dtype=np.int16).reshape(5, 51, 1, 1)
    qw, qb = H.i8_layer(ok, np.arange(5))
    assert qw.dtype == np.int8 and qb.dtype == np.int32 and qw.flags.c_contiguous and np.array_equal(qw, ok)
    for bad in (np.array([[[[128]]]], np.int16), np.array([[[[128.0]]]], np.float32), np.array([[[[-129]]]], np.int32)):
        with pytest.raises(ValueError, match="127"):
            H.i8_layer(bad, np.zeros(1))


def test_dev_input_checks_shape_and_batch():
    x = np.zeros((2, 3, 32, 48), np.float64)
    y = H.dev_input(x, [32, 48], "cpu", max_batch=2)
    assert y.dtype == torch.float32 and y.is_contiguous() and tuple(y.shape) == (2, 3, 32, 48)
    with pytest.raises(ValueError, match=r"expected \[B,3,32,48\]"):
        H.dev_input(np.zeros((2, 3, 48, 32), np.float32), [32, 48], "cpu")
    with pytest.raises(ValueError, match="batch 2 > max_batch 1"):
        H.dev_input(x, [32, 48], "cpu", max_batch=1)
    assert tuple(H.dev_input(x, [32, 48], "cpu").shape) == (2, 3, 32, 48)       # a pipeline takes any batch size


def test_sizes_wh_messages_stay():
    from yolo355 import framelist
    with pytest.raises(ValueError, match="sizes_wh has 2 rows for a batch of 3"):
        framelist.wh_tensor([[1, 2], [3, 4]], 3, "cpu")
    with pytest.raises(ValueError, match="sizes_wh has 2 rows for a list of 3"):
        framelist.sizes_wh_tensor([[1, 2], [3, 4]], [(4, 4)] * 3, "cpu")
    wh = framelist.sizes_wh_tensor("own", [(4, 6), (8, 2)], "cpu")
    assert wh.dtype == torch.float32 and wh.tolist() == [[6.0, 4.0], [2.0, 8.0]]
    assert framelist.sizes_wh_tensor(None, [(4, 4)], "cpu") is None


def test_cached_handle_rebuilds_and_reloads_only_when_needed():
    """models/slim_yolo_v2.py's one cached-handle helper: slot state (handle, key, version)"""
    from yolo355.models.slim_yolo_v2 import _cached

    class Stub:
        def __init__(self, max_batch):
            self.max_batch, self.closed, self.loads = max_batch, False, 0

        def close(self):
            self.closed = True

    def load(h):
        h.loads += 1
    slots, built = {}, []

    def get(key, batch, version):
        return _cached(slots, "s", key, batch, version, lambda: built.append(Stub(max(batch, 1))) or built[-1], load)
    a = get("k", 2, 1)
    assert slots["s"] == (a, "k", 1) and a.loads == 1
    assert get("k", 1, 1) is a and a.loads == 1           # fits, same weights: nothing happens
    assert get("k", 2, 2) is a and a.loads == 2           # new weights: reloaded in place
    b = get("k", 3, 2)                                    # a larger batch: the old handle is closed first, the new one loaded
    assert b is not a and a.closed and b.loads == 1 and not b.closed
    c = get("k2", 1, 2)                                   # another configuration
    assert c is not b and b.closed and slots["s"] == (c, "k2", 2) and len(built) == 3

    def bad_load(h):
        raise ValueError("weights are not dyadic")
    with pytest.raises(ValueError):
        _cached(slots, "t", "k", 1, 1, lambda: Stub(1), bad_load)
    assert slots["t"][1:] == ("k", None)                  # built and kept, marked unloaded: the next call loads again
