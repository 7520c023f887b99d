"""Lists of camera frames of mixed sizes on the int8 SlimYOLOv2 path: y355_forward_frames / y355_resize_frames on the engine,
y355_pipeline_submit_frames on the pipeline, Engine / Pipeline / SlimYOLOv2_quantize_bnfuse .forward_frame_list and the frame
evaluators on that model.  Element i of a list call must equal the single-frame call on frame i bit for bit: detections,
the ten feature maps, candidates, the saturation / guard counts.  The ragged stage (csrc/resize.hip) is checked against the
oracle resize; its kernel gathers bytes from global memory for every frame, whatever its size."""
import ctypes as C

import numpy as np
import pytest

from test_evaluator_frames import _RawSet, _VocSet, _transformed
from test_net_frame_list import _bad_lists, _frame_array, _noise
from test_net_frames import SIZE, _same_dets

NEW = ("y355_forward_frames", "y355_resize_frames", "y355_pipeline_submit_frames")
NC = 2
CONF = 0.05


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_ffi_declare_the_engine_frame_list_entry_points():
    from yolo355 import _ffi
    declared = _ffi.declared_symbols()
    for n in NEW:
        assert n in declared and n in _ffi._SIGS, n
    text = open(_ffi.HEADER_PATH).read()
    assert text.count("typedef struct y355_frame {") == 1 and "} y355_frame;" in text
    assert text.index("} y355_frame;") < text.index("int y355_forward_frames(")       # declared above its first use
    assert text.index("} y355_frame;") < text.index("const y355_frame *")
    f = _ffi.Frame
    assert [n for n, _ in f._fields_] == ["data_dev", "height", "width", "row_bytes"]
    assert (f.data_dev.offset, f.height.offset, f.width.offset, f.row_bytes.offset, C.sizeof(f)) == (0, 8, 12, 16, 24)


def test_engine_frame_list_entry_points_reject_null_arguments_without_hip():
    """a NULL handle or a NULL array is Y355_EINVAL with a message; no HIP call is made (there is no GPU here)"""
    from yolo355 import _ffi
    lib = _ffi.lib()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    arr = (_ffi.Frame * 1)()
    arr[0].data_dev, arr[0].height, arr[0].width = p.value, 4, 4
    t = C.c_longlong(-7)
    calls = [lambda h, f: lib.y355_forward_frames(h, f, 1, 0, p, p, p, p),
             lambda h, f: lib.y355_resize_frames(h, f, 1, p),
             lambda h, f: lib.y355_pipeline_submit_frames(h, f, 1, 0, None, p, p, p, p, C.byref(t))]
    for call in calls:
        for h, f in ((None, arr), (None, None), (p, None)):        # (a non-null handle is not touched before the array check)
            assert call(h, f) == _ffi.EINVAL
            assert lib.y355_last_error().decode()
    assert t.value == -7


def _qbf_model(device="cpu", calibrated=False):
    """SlimYOLOv2_quantize_bnfuse with the weights of test_round2.py::test_resize_stage_matches_oracle, power-of-two quantized"""
    import torch
    from yolo355 import prep, synth
    from yolo355.models.slim_yolo_v2 import SlimYOLOv2_quantize_bnfuse
    m = SlimYOLOv2_quantize_bnfuse(device, input_size=SIZE, num_classes=NC, trainable=False, conf_thresh=CONF, nms_thresh=0.5,
                                   anchor_size=synth.ANCHOR_SIZE_MASK)
    sd = m.state_dict()
    for name, w, b in synth.make_weights(seed=2, num_classes=NC, pred_gain=400.0, obj_bias=-4.0):
        k = "pred" if name == "pred" else name + ".convs.0"
        sd[k + ".weight"] = torch.from_numpy(w.copy())
        sd[k + ".bias"] = torch.from_numpy(b.copy())
    m.load_state_dict(sd, strict=False)
    prep.init_quantize_net(m, 8)
    prep.quantize_layers(8, retune=False)
    m.eval()
    if calibrated:
        m.forward_batch(torch.from_numpy(_calib_input()), quantization=True)
    return m


@pytest.mark.parametrize("bad", ["empty", "4d", "float", "channels", "nested", "zero_height"])
def test_model_validates_the_list_before_any_engine(bad):
    m = _qbf_model()
    for q in (True, False):
        with pytest.raises(ValueError):
            m.forward_frame_list(_bad_lists()[bad], quantization=q)
    assert m._engine is None and m._pipe is None and not m.__dict__.get("_f32")


def test_model_needs_calibrated_trackers_before_any_engine():
    m = _qbf_model()
    with pytest.raises(RuntimeError, match="calibrate the trackers"):
        m.forward_frame_list([np.zeros((8, 8, 3), np.uint8)], quantization=True)
    with pytest.raises(RuntimeError, match="calibrate the trackers"):
        m.forward_frame_list([np.zeros((8, 8, 3), np.uint8)] * (m.PIPELINE_CHUNK + 1), quantization=True)
    assert m._engine is None and m._pipe is None


# ---------------------------------------------------------------------------------------------------- GPU
_CACHE = {}


def _calib_input():
    """one oracle-resized frame, normalised: what every handle of this file is calibrated on"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import synth
    return synth.normalize_frames(resize_linear_u8(synth.make_frames_u8(77, 1, 300, 400, "blocks"), SIZE[0], SIZE[1]))


def _load(target):
    from oracle import yolo_oracle as O
    from yolo355 import prep, synth
    if "ql" not in _CACHE:
        _CACHE["ql"] = O.quantize_layers(synth.make_weights(seed=2, num_classes=NC, pred_gain=400.0, obj_bias=-4.0))
    target.load_quantized(_CACHE["ql"])
    return target.calibrate(_calib_input(), [prep.RangeTracker() for _ in range(11)])


def _engine(maxb=4):
    if ("eng", maxb) not in _CACHE:
        from yolo355 import synth
        from yolo355.engine import Engine
        eng = Engine(SIZE, NC, synth.ANCHOR_SIZE_MASK, conf_thresh=CONF, max_batch=maxb)
        _load(eng)
        _CACHE[("eng", maxb)] = eng
    return _CACHE[("eng", maxb)]


def _ref(frames):
    """the oracle-resized frames [n,H,W,3] of a list"""
    from oracle.resize_oracle import resize_linear_u8
    return np.stack([resize_linear_u8(f, SIZE[0], SIZE[1]) for f in frames])


def _scramble(eng):
    """fill every batch slot, rs_frames, the per-frame tables and the same-size route's table with other data"""
    import torch
    from yolo355 import _ffi, synth
    n = eng.max_batch
    eng.forward_frame_list_device([_noise(900 + i, 90 + 7 * i, 130 - 11 * i) for i in range(n)], _ffi.F_TAP)
    other = synth.make_frames_u8(99, n, 120, 160, "noise")
    eng.forward_frames_device(torch.from_numpy(other).cuda(), _ffi.F_TAP)
    eng.forward_device(torch.from_numpy(synth.normalize_frames(_ref(list(other)))).cuda(), _ffi.F_TAP)
    eng.counters()


def _three_frames(seed=0):
    from yolo355 import synth
    return [synth.make_frames_u8(31 + seed, 1, SIZE[0], SIZE[1], "blocks")[0], synth.make_frames_u8(32 + seed, 1, 149, 211, "blocks")[0],
            synth.make_frames_u8(33 + seed, 1, 480, 640, "blocks")[0]]


def _dets(out, B):
    ob, os_, oc, on = out
    n = on[:B].cpu().numpy()
    b, s, c = ob[:B].cpu().numpy(), os_[:B].cpu().numpy(), oc[:B].cpu().numpy()
    return [(b[i, :n[i]].copy(), s[i, :n[i]].copy(), c[i, :n[i]].astype(np.int64)) for i in range(B)]


def _maps(eng, B):
    """the ten feature maps of the last forward (None where a fused launch keeps the map on chip: Y355_ENOTREADY)"""
    from yolo355 import _ffi
    out = []
    for k in range(10):
        try:
            out.append(eng.get_feature(k, B))
        except _ffi.Y355Error as e:
            assert e.code == _ffi.ENOTREADY and k in (0, 2), (k, e)
            out.append(None)
    return out


def _check_list(eng, frames, flags, given=None):
    """the list call on a scrambled engine against forward_frames_device(frame[None]) per frame"""
    import torch
    from yolo355 import _ffi
    n, tap = len(frames), bool(flags & _ffi.F_TAP)
    _scramble(eng)
    got = _dets(eng.forward_frame_list_device(frames if given is None else given, flags), n)
    gmaps = _maps(eng, n) if tap else None
    gcand = eng.candidates(n) if tap else None
    gsat, gguard = eng.counters()
    sat = guard = 0
    for i, f in enumerate(frames):
        _scramble(eng)
        one = _dets(eng.forward_frames_device(torch.from_numpy(f[None]).cuda(), flags), 1)
        _same_dets(one, got[i:i + 1])
        if tap:
            for k, (a, b) in enumerate(zip(gmaps, _maps(eng, 1))):
                assert (a is None) == (b is None), k
                assert a is None or np.array_equal(a[i], b[0]), "frame %d feature map %d differs" % (i, k)
            for a, b in zip(gcand, eng.candidates(1)):
                assert np.array_equal(a[i], b[0]), "frame %d candidates differ" % i
        s1, g1 = eng.counters()
        sat, guard = sat + s1, guard + g1
    assert (gsat, gguard) == (sat, guard)
    assert sum(len(d[1]) for d in got) > 0
    return got, gsat


def _stage_sizes():
    """(h, w) of the stage test: the named list and the two-dimensional sweep (heights geometric from 1 to 4000 against widths
    from 4000 down to 1).  The stage's one kernel gathers bytes for every frame: it has no path that depends on the size."""
    named = [(1, 1), (1, 7), (7, 1), (37, 53), tuple(SIZE), (480, 640), (2, 16384), (16384, 2), (500, 375)]
    hs = [int(round(v)) for v in np.geomspace(1, 4000, 12)]
    return named, list(zip(hs, hs[::-1]))


@pytest.mark.gpu
def test_ragged_stage_equals_the_oracle():
    """Engine.resize_frame_list against oracle.resize_oracle.resize_linear_u8, bit for bit; the frames are packed with
    misaligned starts and another list has gone through the handle first"""
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import framelist
    eng = _engine(8)
    named, sweep = _stage_sizes()
    assert len(sweep) == 12 and sweep[0] == (1, 4000) and sweep[-1] == (4000, 1)
    k = 0
    for sizes in (named[:5], named[5:], sweep[:6], sweep[6:]):
        assert len(sizes) < eng.max_batch
        sizes = [(1, 1)] + list(sizes)                                     # three bytes in front: the starts behind it are misaligned
        frames = [_noise(40 + k + i, h, w) for i, (h, w) in enumerate(sizes)]
        k += len(sizes)
        _, offsets, _ = framelist.pack_frames(frames)
        assert any(o % 4 for o in offsets)
        eng.resize_frame_list([_noise(60 + i, 50 + i, 70 - i) for i in range(8)])       # other tables and pixels first
        got = eng.resize_frame_list(frames).cpu().numpy()
        for i, f in enumerate(frames):
            want = resize_linear_u8(f, SIZE[0], SIZE[1])
            assert np.array_equal(got[i], want), (sizes[i], int((got[i] != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "find", "tap", "tap_find", "tap_unfused"])
def test_list_forward_equals_single_calls(mode):
    """three frames (the network size, 149 x 211, 480 x 640) against three single-frame calls: detections, the feature maps
    and candidates under tap, the (saturated, guard) sums.  A guard run launches every layer on its own, so all ten maps
    exist; a fused tap run keeps conv1's and conv3_1's maps on chip in both routes; tap_unfused switches the fusions off."""
    from yolo355 import _ffi
    eng = _engine()
    flags = (_ffi.F_TAP if "tap" in mode else 0) | (_ffi.F_GUARD if "find" in mode else 0)
    try:
        if mode == "tap_unfused":
            eng.set_option(_ffi.OPT_FUSE_FRONT, 0)
            eng.set_option(_ffi.OPT_FUSE_PAIRS, 0)
        _check_list(eng, _three_frames(), flags)
        if mode in ("tap_find", "tap_unfused"):
            assert all(m is not None for m in _maps(eng, 1))
    finally:
        eng.set_option(_ffi.OPT_FUSE_FRONT, 1)
        eng.set_option(_ffi.OPT_FUSE_PAIRS, 1)
    if mode == "find":                                                  # the host-side method reads the guard count of its own call
        _same_dets(eng.forward_frame_list(_three_frames(), find=True), _dets(eng.forward_frame_list_device(_three_frames(), flags), 3))


@pytest.mark.gpu
def test_clamp_counts_add_up():
    """input exponent raised by 3: the list's saturation count (> 0) is the sum of the single calls' counts"""
    from yolo355 import _ffi
    eng = _engine()
    sa = eng.get_act_exponents()
    try:
        eng.set_act_exponents([sa[0] + 3] + sa[1:])
        for flags in (0, _ffi.F_TAP):
            _, sat = _check_list(eng, _three_frames(), flags)
            assert sat > 0
    finally:
        eng.set_act_exponents(sa)


@pytest.mark.gpu
def test_pitched_views_and_mixed_lists():
    import torch
    from yolo355 import _ffi
    eng = _engine()
    big = torch.from_numpy(_noise(70, 60, 70)).cuda()
    view = big[10:47, 5:58]
    assert not view.is_contiguous() and view.stride() == (210, 3, 1)
    crop = view.contiguous().cpu().numpy()
    a, b, c = _three_frames(3)
    frames = [a, crop, b, c]
    given = [a, view, torch.from_numpy(b).cuda(), torch.from_numpy(c)]          # numpy, pitched CUDA, CUDA, CPU torch
    want = eng.resize_frame_list(frames).cpu().numpy()
    assert np.array_equal(want, _ref(frames))
    assert np.array_equal(eng.resize_frame_list(given).cpu().numpy(), want)
    _check_list(eng, frames, _ffi.F_TAP, given=given)
    _scramble(eng)
    _same_dets(eng.forward_frame_list(frames), eng.forward_frame_list(given))


@pytest.mark.gpu
def test_alternating_sizes_keep_no_stale_state():
    """two lists alternated for four rounds with nothing but launches in between; one same-size call of a non-network size
    before the rounds and one in the middle (the table cached under rs_src_h / rs_src_w must survive the list calls)"""
    import torch
    from yolo355 import synth
    eng = _engine()
    md, MAXB = eng.max_det, eng.max_batch

    def bufs():
        return (torch.empty((MAXB, md, 4), dtype=torch.float32, device="cuda:0"), torch.empty((MAXB, md), dtype=torch.float32, device="cuda:0"),
                torch.empty((MAXB, md), dtype=torch.int32, device="cuda:0"), torch.zeros((MAXB,), dtype=torch.int32, device="cuda:0"))
    la = _three_frames(5)
    lb = [synth.make_frames_u8(80 + i, 1, h, w, "blocks")[0] for i, (h, w) in enumerate([(375, 500), (333, 77), (224, 321), (97, 640)])]
    same = torch.from_numpy(synth.make_frames_u8(85, 2, 240, 352, "blocks")).cuda()
    _scramble(eng)
    outs = [bufs() for _ in range(10)]
    eng.forward_frames_device(same, 0, outs[8])
    for r in range(4):
        eng.forward_frame_list_device(la, 0, outs[2 * r])
        if r == 2:
            eng.forward_frames_device(same, 0, outs[9])
        eng.forward_frame_list_device(lb, 0, outs[2 * r + 1])
    torch.cuda.synchronize()
    res = [_dets(o, 2 if k >= 8 else (3 if k % 2 == 0 else 4)) for k, o in enumerate(outs)]
    assert sum(len(d[1]) for d in res[0] + res[1]) > 0 and sum(len(d[1]) for d in res[8]) > 0
    for r in range(1, 4):
        _same_dets(res[0], res[2 * r])
        _same_dets(res[1], res[2 * r + 1])
    _same_dets(res[8], res[9])
    _same_dets(res[8], eng.forward_frames(_ref(list(same.cpu().numpy()))))
    _same_dets(res[0], eng.forward_frames(_ref(la)))
    _same_dets(res[1], eng.forward_frames(_ref(lb)))


def _mixed_frames(n, seed=200):
    from yolo355 import synth
    kinds = [(375, 500), tuple(SIZE), (149, 211), (480, 640), (500, 333), (97, 131), (300, 301)]
    return [synth.make_frames_u8(seed + i, 1, *kinds[i % len(kinds)], "blocks")[0] for i in range(n)]


def _pipeline():
    if "pipe" not in _CACHE:
        from yolo355 import synth
        from yolo355.engine import Pipeline
        pipe = Pipeline(SIZE, NC, synth.ANCHOR_SIZE_MASK, conf_thresh=CONF, max_batch=3, handles=2)
        _load(pipe)
        _CACHE["pipe"] = pipe
    return _CACHE["pipe"]


@pytest.mark.gpu
def test_pipeline_forward_frame_list():
    """21 mixed frames: seven chunks of 3 through a depth of 4, equal to the engine's list forwards chunk by chunk;
    sizes_wh="own" equals the host rescale by every frame's own (w, h)"""
    pipe, eng = _pipeline(), _engine()
    assert pipe.depth == 4 and pipe.max_batch == 3
    assert eng.get_act_exponents() == pipe.engine(0).get_act_exponents()
    frames = _mixed_frames(21)
    t0 = pipe.next_ticket
    got = pipe.forward_frame_list(frames)
    assert pipe.next_ticket == t0 + 7
    want = []
    for i0 in range(0, 21, 3):
        _scramble(eng)
        want.extend(eng.forward_frame_list(frames[i0:i0 + 3]))
    _same_dets(want, got)
    assert sum(len(d[1]) for d in got) > 0
    host = []
    for (b, s, c), f in zip(want, frames):
        b = b.copy()
        b *= np.array([[f.shape[1], f.shape[0], f.shape[1], f.shape[0]]])
        host.append((b, s, c))
    own = pipe.forward_frame_list(frames, sizes_wh="own")
    _same_dets(host, own)
    _same_dets(own, pipe.forward_frame_list(frames, sizes_wh=np.asarray([(f.shape[1], f.shape[0]) for f in frames], np.float32)))
    _same_dets(own[:3], eng.forward_frame_list(frames[:3], sizes_wh="own"))
    guarded = pipe.forward_frame_list(frames[:6], find=True)              # the guard flag, read per ticket
    _same_dets(eng.forward_frame_list(frames[:3], find=True) + eng.forward_frame_list(frames[3:6], find=True), guarded)
    with pytest.raises(ValueError):
        pipe.forward_frame_list(frames, sizes_wh="theirs")
    with pytest.raises(ValueError):
        pipe.submit_frame_list(frames[:4])                              # more than max_batch frames
    with pytest.raises(ValueError):
        eng.forward_frame_list(frames[:5])


@pytest.mark.gpu
def test_pipeline_submit_frame_list_tickets_errors_and_lifetime():
    import torch
    from yolo355 import _ffi
    pipe, eng = _pipeline(), _engine()
    lib = _ffi.lib()
    frames = _mixed_frames(3, seed=230)
    want = eng.forward_frame_list(frames)
    assert sum(len(d[1]) for d in want) > 0
    md = pipe.max_det
    mine = (torch.empty((3, md, 4), dtype=torch.float32, device="cuda:0"), torch.empty((3, md), dtype=torch.float32, device="cuda:0"),
            torch.empty((3, md), dtype=torch.int32, device="cuda:0"), torch.zeros((3,), dtype=torch.int32, device="cuda:0"))
    ta = pipe.submit_frame_list(frames, out=mine)                       # caller-owned outputs
    tb = pipe.submit_frame_list(frames)                                 # pipeline-owned outputs
    assert tb == ta + 1 and pipe.outputs(ta)[0] is mine[0] and pipe.outputs(tb)[0] is not mine[0]
    pipe.wait(ta)
    pipe.wait(tb, host=True)
    _same_dets(want, _dets(pipe.outputs(ta), 3))
    _same_dets(want, _dets(pipe.outputs(tb), 3))
    _same_dets(want, pipe.fetch(tb))
    pipe.release(tb)
    # a rejected list: Y355_EINVAL, no ticket issued; the next good submit is right
    fd = torch.from_numpy(frames[0]).cuda()
    h, w = frames[0].shape[:2]
    bad = _frame_array([(fd.data_ptr(), h, w, 0), (fd.data_ptr(), h, w, 3 * w - 1)])
    t = C.c_longlong(-7)
    ob, os_, oc, on = mine
    n0 = pipe.next_ticket
    cur = torch.cuda.current_stream().cuda_stream
    assert lib.y355_pipeline_submit_frames(pipe._h, bad, 2, _ffi.PIPE_AFTER_STREAM, cur, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(),
                                           on.data_ptr(), C.byref(t)) == _ffi.EINVAL
    assert "row_bytes" in lib.y355_last_error().decode() and t.value == -7
    tc = pipe.submit_frame_list(frames)
    assert tc == n0 == pipe.next_ticket - 1
    _same_dets(want, pipe.fetch(tc))
    # fresh CUDA frames, every Python reference dropped, the same sizes allocated and filled on the current stream
    cuda = [torch.from_numpy(f).cuda() for f in frames]
    td = pipe.submit_frame_list(cuda)
    del cuda
    junk = [torch.full(f.shape, 255, dtype=torch.uint8, device="cuda:0") for f in frames for _ in range(2)]
    _same_dets(want, pipe.fetch(td))
    del junk
    # a ticket is gone after `depth` further submits
    for _ in range(pipe.depth):
        last = pipe.submit_frame_list(frames)
    with pytest.raises(_ffi.Y355Error):
        pipe.fetch(td)
    assert lib.y355_pipeline_wait(pipe._h, td, 0, None) == _ffi.ENOTREADY
    _same_dets(want, pipe.fetch(last))
    pipe.sync()


@pytest.mark.gpu
def test_model_forward_frame_list_matches_forward_batch():
    import torch
    from yolo355 import synth
    m = _qbf_model("cuda:0", calibrated=True)
    frames = _mixed_frames(5, seed=260)

    def want(q):
        return [m.forward_batch(torch.from_numpy(synth.normalize_frames(_ref([f]))), quantization=q)[0] for f in frames]
    wq = want(True)
    assert sum(len(d[1]) for d in wq) > 0
    _same_dets(wq, m.forward_frame_list(frames, quantization=True))
    assert m._pipe is None
    _same_dets(wq, m.forward_frame_list(frames))                                       # quantization=True is the default
    try:
        m.PIPELINE_CHUNK = 2                                                             # five frames: the pipeline branch
        _same_dets(wq, m.forward_frame_list(frames, quantization=True))
        assert m._pipe is not None and m._pipe.max_batch == 2
    finally:
        del m.PIPELINE_CHUNK
    _same_dets(want(False), m.forward_frame_list(frames, quantization=False))
    host = [(b * np.array([[f.shape[1], f.shape[0], f.shape[1], f.shape[0]]], np.float32), s, c) for (b, s, c), f in zip(wq, frames)]
    _same_dets(host, m.forward_frame_list(frames, sizes_wh="own"))


@pytest.mark.gpu
def test_frame_evaluators_accept_the_int8_model():
    from yolo355.utils.evaluator_batch import coco_data_dict, coco_data_dict_frames, voc_all_boxes, voc_all_boxes_frames
    m = _qbf_model("cuda:0", calibrated=True)
    raw = _RawSet()

    def transform(img):                                    # HWC BGR float at the network size, as BaseTransform returns it
        return [np.ascontiguousarray(_transformed(img).transpose(1, 2, 0)[:, :, ::-1])]
    got = voc_all_boxes_frames(m, raw, NC, batch_size=3, quantization=True)
    want = voc_all_boxes(m, _VocSet(raw), NC, batch_size=3, quantization=True)
    n = 0
    for j in range(NC):
        for i in range(len(raw)):
            assert got[j][i].dtype == np.float32 and np.array_equal(got[j][i], want[j][i]), (j, i)
            n += len(got[j][i])
    assert n > 0
    ids, dd = coco_data_dict_frames(m, raw, batch_size=3, quantization=True)
    wids, wdd = coco_data_dict(m, raw, transform, batch_size=3, quantization=True)
    assert ids == wids == [1000 + 3 * i for i in range(len(raw))]
    assert len(dd) > 0 and dd == wdd


@pytest.mark.gpu
def test_errors_on_a_live_handle_leave_it_usable():
    import torch
    from oracle.resize_oracle import resize_linear_u8
    from yolo355 import _ffi
    eng, pipe = _engine(), _pipeline()
    lib = _ffi.lib()
    f = _noise(95, 37, 53)
    three = _three_frames(9)
    want = resize_linear_u8(f, SIZE[0], SIZE[1])
    want_dets = eng.forward_frame_list(three)
    fd = torch.from_numpy(f).cuda()
    out = torch.empty((eng.max_batch + 1, SIZE[0], SIZE[1], 3), dtype=torch.uint8, device="cuda:0")
    ob, os_, oc, on = eng._buffers(1)
    good = (fd.data_ptr(), 37, 53, 0)
    t = C.c_longlong(-7)
    bad = {"pitch": [(fd.data_ptr(), 37, 53, 3 * 53 - 1)], "null": [good, (None, 37, 53, 0)], "wide": [(fd.data_ptr(), 1, 16385, 0)],
           "batch": [good] * (eng.max_batch + 1)}
    outs = (ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), on.data_ptr())
    n0 = pipe.next_ticket
    for name, desc in bad.items():
        arr = _frame_array(desc)
        assert lib.y355_resize_frames(eng._h, arr, len(desc), out.data_ptr()) == _ffi.EINVAL, name
        assert lib.y355_last_error().decode()
        assert lib.y355_forward_frames(eng._h, arr, len(desc), 0, *outs) == _ffi.EINVAL, name
        assert lib.y355_pipeline_submit_frames(pipe._h, arr, len(desc), 0, None, *outs, C.byref(t)) == _ffi.EINVAL, name
        assert lib.y355_pipeline_submit_frames(pipe._h, arr, len(desc), 0, None, None, None, None, None, C.byref(t)) == _ffi.EINVAL, name
    arr = _frame_array([good])                                          # a null output
    assert lib.y355_resize_frames(eng._h, arr, 1, None) == _ffi.EINVAL
    assert lib.y355_forward_frames(eng._h, arr, 1, 0, None, *outs[1:]) == _ffi.EINVAL
    assert lib.y355_pipeline_submit_frames(pipe._h, arr, 1, 0, None, None, *outs[1:], C.byref(t)) == _ffi.EINVAL
    assert lib.y355_pipeline_submit_frames(pipe._h, arr, 1, 0, None, *outs, None) == _ffi.EINVAL
    assert t.value == -7 and pipe.next_ticket == n0
    assert np.array_equal(eng.resize_frame_list([f]).cpu().numpy()[0], want)
    assert np.array_equal(pipe.engine(0).resize_frame_list([f]).cpu().numpy()[0], want)
    _same_dets(want_dets, eng.forward_frame_list(three))
    _same_dets(want_dets, pipe.forward_frame_list(three))
    assert pipe.next_ticket == n0 + 1
