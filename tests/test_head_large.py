"""The detection head above 4096 candidates per image (csrc/nms_large.hip): engine.head_f32(max_candidates=, route=), the
Y355_OPT_MAX_CANDIDATES / Y355_OPT_HEAD_ROUTE options of Engine, Pipeline and Net, and the network sizes the 4096-anchor
limit used to refuse.  Inputs: tests/head_cases.py, tests/head_large_cases.py.

Against the fp32 oracle (inputs under head_cases.h_guards): counts and classes exact, boxes within 2e-5, scores within 2e-6,
as tests/test_head_adversarial.py::_run_h.  Against the oracle's NMS on the GPU's own decode (the candidate tap), and between
the two routes: exact equality, no tolerance -- both read the same floats.
"""
import re

import numpy as np
import pytest

import head_cases as HC
import head_large_cases as LC

THR = 0.5


# ------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n_on,C", [(4097, 20), (6000, 20), (10647, 20), (6000, 1)])
def test_generators_hold_the_guards(n_on, C):
    case, dec = LC.guarded(n_on, C)
    n = [int((dec[1][b] >= np.float32(case["conf"])).sum()) for b in range(2)]
    assert n == [n_on, n_on], n
    g = HC.h_guards(case, THR, dec)
    print("h4 n_on=%d C=%d guards %s" % (n_on, C, g))
    assert g["ok"], g
    ref = HC.h_reference(case, THR, dec)
    assert all(0 < len(r[1]) < n_on for r in ref), [len(r[1]) for r in ref]          # some suppression, not all


def test_h4_variant_is_h4_compaction():
    a, b = LC.h4_variant(4097, 20), HC.h4_compaction(4097)
    assert all(np.array_equal(x, y) for x, y in zip(a["preds"], b["preds"])) and a["anchors"] == b["anchors"]


def test_ffi_and_header_declare_the_new_symbols():
    from yolo355 import _ffi
    hdr = open(_ffi.HEADER_PATH).read()
    for name in ("y355_head_f32_ex", "y355_overflow", "y355_max_candidates", "y355_pipeline_ticket_overflow", "y355_net_max_candidates"):
        assert name in _ffi._SIGS and re.search(r"\b%s\(" % name, hdr), name
    for name, val in (("OPT_MAX_CANDIDATES", 4), ("OPT_HEAD_ROUTE", 5), ("NET_OPT_MAX_CANDIDATES", 3), ("NET_OPT_HEAD_ROUTE", 4),
                      ("HEAD_ROUTE_AUTO", 0), ("HEAD_ROUTE_LARGE", 1)):
        assert getattr(_ffi, name) == val
        assert re.search(r"#define Y355_%s %d\b" % (name, val), hdr), name
    lib = _ffi.lib()                                     # every table entry resolves in the library
    assert lib.y355_head_f32_ex is not None


def test_head_f32_ex_validates_before_any_gpu_work():
    import ctypes as C
    from yolo355 import _ffi
    lib = _ffi.lib()
    p = np.zeros((1, 6, 2, 2), np.float32)
    ptrs = (C.c_void_p * 1)(p.ctypes.data)
    hs, ws, st = (C.c_int * 1)(2), (C.c_int * 1)(2), (C.c_float * 1)(8.0)
    an = (C.c_float * 2)(1.0, 1.0)
    out = np.zeros(64, np.float32)
    o = out.ctypes.data

    def err():
        return lib.y355_last_error().decode()

    def call(cap, route, taps=(None, None, None)):
        return lib.y355_head_f32_ex(0, 1, ptrs, hs, ws, st, an, 1, 1, 16, 16, 1.0, 0.5, 0.5, 1, 4, cap, route, o, o, o, o, *taps)
    assert call(4095, 0) == _ffi.EINVAL and "max_candidates" in err()
    assert call(5000, 0) == _ffi.EINVAL                  # above the head's 4 anchors
    assert call(4096, 2) == _ffi.EINVAL and "route" in err()
    assert call(4096, 0, (o, None, None)) == _ffi.EINVAL


# ------------------------------------------------------------------------------------------------- GPU helpers
def _head(case, thr=THR, **kw):
    from yolo355 import engine as E
    nlev, A = len(case["strides"]), case["A"]
    return E.head_f32(case["preds"], case["strides"], np.asarray(case["anchors"], np.float32).reshape(nlev, A, 2), case["C"], case["size"],
                      1.0, case["conf"], thr, **kw)


def _close(got, want, max_det=None):
    for b, (g, w) in enumerate(zip(got, want)):
        w = [r[:max_det] for r in w[:3]] if max_det else w[:3]
        assert len(g[1]) == len(w[1]), (b, len(g[1]), len(w[1]))
        assert np.array_equal(g[2], w[2]), b
        db, ds = np.abs(g[0] - w[0]).max(), np.abs(g[1] - w[1]).max()
        print("image %d: %d detections, max box error %.3g, max score error %.3g" % (b, len(g[1]), db, ds))
        assert db < 2e-5 and ds < 2e-6, (b, db, ds)


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x[1]) == len(y[1]), (i, len(x[1]), len(y[1]))
        for k in range(3):
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (i, k)


def _tap_equal(dets, tap, conf, thr, C, min_suppressed=0):
    """detections == the oracle's NMS on the tapped decode, exactly; returns the oracle's lists"""
    refs = []
    for b, d in enumerate(dets):
        ref = HC.oracle_nms(tap[0][b], tap[1][b], tap[2][b], conf, thr, C)
        ncand = int((tap[1][b] >= np.float32(conf)).sum())
        assert ncand - len(ref[1]) >= min_suppressed, (b, ncand, len(ref[1]))
        assert len(d[1]) == len(ref[1]), (b, len(d[1]), len(ref[1]))
        assert np.array_equal(d[0], ref[0]) and np.array_equal(d[1], ref[1]) and np.array_equal(d[2], ref[2]), b
        assert np.array_equal(d[0], tap[0][b][ref[3]]) and np.array_equal(d[1], tap[1][b][ref[3]])       # the tapped floats themselves
        refs.append(ref)
    return refs


# ------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n_on,C", [(4097, 20), (6000, 20), (10647, 20), (6000, 1)])
def test_above_the_old_limit_against_the_oracle(n_on, C):
    """more than 4096 candidates per image, capacity = N: the fp32 oracle's detections"""
    case, dec = LC.guarded(n_on, C)
    assert HC.h_guards(case, THR, dec)["ok"]
    _close(_head(case, max_candidates=10647), HC.h_reference(case, THR, dec))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["e1_low_2", "e1_mid_2", "e1_high_2", "e1_low_5", "e1_mid_5", "e1_high_5", "e2", "e3_chain", "e3_clump",
                                  "e4_0.5", "e4_5e-5", "e4_1.0", "e5_empty_and_dense"])
def test_routes_agree_on_the_engine(name):
    """the adversarial E inputs: Y355_OPT_HEAD_ROUTE = LARGE gives the default route's bytes"""
    from yolo355 import _ffi
    from yolo355.engine import Engine
    thr = None
    if name.startswith("e1"):
        _, band, C = name.split("_")
        case = HC.e1_full_capacity(band, int(C))
    elif name == "e2":
        case = HC.e2_dense()
    elif name.startswith("e3"):
        case = HC.e3_chain(name == "e3_clump")
    elif name.startswith("e4"):
        case, thr = HC.e4_degenerate(), float(name.split("_")[1])
    else:
        case = HC.e5_empty_and_dense()
    eng = Engine(case["size"], case["C"], case["anchors"], conf_thresh=case["conf"], nms_thresh=case["thr"] if thr is None else thr,
                 max_batch=2)
    try:
        small = eng.head_nms(case["pq"], case["sa"])
        eng.set_option(_ffi.OPT_HEAD_ROUTE, _ffi.HEAD_ROUTE_LARGE)
        large = eng.head_nms(case["pq"], case["sa"])
        eng.set_head_route(_ffi.HEAD_ROUTE_AUTO)
        again = eng.head_nms(case["pq"], case["sa"])
    finally:
        eng.close()
    print(name, "detections", [len(d[1]) for d in small])
    _same(small, large)
    _same(small, again)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h1", "h5"])
def test_routes_agree_on_head_f32(name):
    case = HC.h1_three_levels(2) if name == "h1" else HC.h5_degenerate()
    for thr in HC.H1_THR:
        _same(_head(case, thr), _head(case, thr, route=1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three_levels_4410", "large_boxes_10647"])
def test_dense_above_the_limit_exact_on_the_tap(name):
    """every anchor a candidate, thousands of suppressions, classes that span several tiles of the large route"""
    case = LC.dense_three_levels() if name == "three_levels_4410" else LC.dense_10647()
    N = sum(p.shape[2] * p.shape[3] for p in case["preds"]) * case["A"]
    assert N == (4410 if name == "three_levels_4410" else 10647)
    dets, tap = _head(case, case["thr"], max_candidates=N, return_candidates=True)
    for b in range(2):
        cand = tap[1][b] >= np.float32(case["conf"])
        assert int(cand.sum()) == N                                                   # every anchor
        assert np.bincount(tap[2][b][cand]).max() > 1024                               # one class spans several tiles
    refs = _tap_equal(dets, tap, case["conf"], case["thr"], case["C"], min_suppressed=1000)
    print(name, "candidates", N, "kept", [len(r[1]) for r in refs], "largest class",
          [int(np.bincount(tap[2][b]).max()) for b in range(2)])


@pytest.mark.gpu
def test_capacity_boundary():
    from yolo355._ffi import Y355Error
    case, dec = LC.guarded(6000)
    _close(_head(case, max_candidates=6000), HC.h_reference(case, THR, dec))
    over = HC.h4_compaction(6001)
    with pytest.raises(Y355Error, match="6000"):
        _head(over, max_candidates=6000)


@pytest.mark.gpu
def test_max_det_above_4096():
    case, dec = LC.guarded(6000)
    got = _head(case, max_candidates=6000, max_det=5000)
    assert [len(g[1]) for g in got] == [5000, 5000]
    _close(got, HC.h_reference(case, THR, dec), max_det=5000)


@pytest.mark.gpu
def test_mixed_batch_takes_both_routes():
    """an empty image, one for the small route and one for the large route in one batch, capacity raised, route AUTO"""
    case = LC.mixed_batch()
    got = _head(case, max_candidates=6000)
    n = [len(g[1]) for g in got]
    assert n[0] == 0 and 100 < n[1] <= 300 and n[2] > 4096, n
    for b in range(3):
        _same([got[b]], _head(LC.one_image(case, b), max_candidates=6000))
    _same([got[1]], _head(LC.one_image(case, 1)))                                  # and the default capacity's result


# ---- sizes the 4096-anchor limit used to refuse
def _below_and_above(run, tap_of, set_conf, set_cap, N, C, thr=0.5):
    """run() -> detections; with the capacity raised to N and conf_thresh 0 every anchor is a candidate; at the default
    capacity a threshold that lets about a thousand through.  Both equal the oracle's NMS on the tapped decode."""
    set_cap(N)
    set_conf(0.0)
    dets = run()
    tap = tap_of()
    assert all(int((tap[1][b] >= 0).sum()) == N for b in range(len(dets)))
    _tap_equal(dets, tap, 0.0, thr, C)
    conf = float(np.sort(tap[1].reshape(-1))[-1000 * len(dets)])
    set_cap(4096)
    set_conf(conf)
    dets2 = run()
    tap2 = tap_of()
    assert all(np.array_equal(x, y) for x, y in zip(tap, tap2))
    assert all(0 < int((tap2[1][b] >= np.float32(conf)).sum()) <= 4096 for b in range(len(dets2)))
    _tap_equal(dets2, tap2, conf, thr, C)
    return dets, dets2, conf


@pytest.mark.gpu
def test_q_bf_engine_and_pipeline_at_256x832():
    """16 x 52 cells x 5 anchors = 4160 anchors per image"""
    import torch
    from oracle import yolo_oracle as O
    from yolo355 import synth
    from yolo355.engine import Engine, Pipeline
    from yolo355.prep import RangeTracker
    H, W, C, B = 256, 832, 2, 2
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=C, pred_gain=400.0, obj_bias=-4.0))
    eng = Engine([H, W], C, synth.ANCHOR_SIZE_MASK, conf_thresh=0.01, nms_thresh=0.5, max_batch=B)
    assert eng.num_anchors_total == 4160 and eng.max_det == 4096
    eng.load_quantized(ql)
    sa = eng.calibrate(synth.make_images(1, 1, H, W, "blocks"), [RangeTracker() for _ in range(11)])
    x = synth.make_images(3, B, H, W, "blocks")
    dets, dets2, conf = _below_and_above(lambda: eng.forward(x, tap=True), lambda: eng.candidates(B),
                                         lambda c: eng.set_thresholds(c, 0.5), eng.set_max_candidates, 4160, C)
    assert eng.max_det == 4096
    eng.close()
    pipe = Pipeline([H, W], C, synth.ANCHOR_SIZE_MASK, conf_thresh=0.0, nms_thresh=0.5, max_batch=B, handles=1, max_candidates=4160)
    assert pipe.max_det == 4160
    pipe.load_quantized(ql)
    pipe.set_act_exponents(sa)
    xd = torch.from_numpy(x).to("cuda:0")
    t = pipe.submit(xd)
    _same(pipe.fetch(t), dets)
    # the overflow belongs to the ticket whose forward dropped candidates: capacity 4096 with every anchor a candidate
    from yolo355._ffi import Y355Error
    pipe.set_max_candidates(4096)
    t1 = pipe.submit(xd)
    pipe.set_thresholds(conf, 0.5)
    t2 = pipe.submit(xd)
    assert not pipe.overflow(t2) and pipe.overflow(t1)
    _same(pipe.fetch(t2), dets2)
    with pytest.raises(Y355Error, match="4096"):
        pipe.fetch(t1)
    pipe.close()


@pytest.mark.gpu
def test_packed_records_hold_max_det_above_4096():
    """y355_pack_dets_capped / y355_unpack_dets / y355_packed_det_bytes at max_det = 5000: the kernel's records equal the torch
    packing byte for byte, and unpack to the arrays that went in (entries past count zeroed)"""
    import ctypes as C
    import torch
    from yolo355 import _ffi, shard
    md, n = 5000, 3
    g = torch.Generator().manual_seed(5)
    boxes = torch.rand((n, md, 4), generator=g).cuda()
    scores = torch.rand((n, md), generator=g).cuda()
    cls = torch.randint(0, 80, (n, md), generator=g, dtype=torch.int32).cuda()
    count = torch.tensor([5000, 4097, 0], dtype=torch.int32).cuda()
    rb = shard.record_bytes(md)
    assert _ffi.lib().y355_packed_det_bytes(md) == rb == 16 + 24 * md
    want = shard.pack_detections(boxes, scores, cls, count, records=4)
    got = shard.pack_detections_kernel(boxes, scores, cls, count, 4, torch.empty((4, rb), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    ob, os_, oc = torch.full_like(boxes, -1), torch.full_like(scores, -1), torch.full_like(cls, -1)
    on = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    slot = torch.tensor([0, 1, 2, -1], dtype=torch.int32).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(_ffi.lib().y355_unpack_dets(got.data_ptr(), slot.data_ptr(), 4, md, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(),
                                           on.data_ptr(), st))
    torch.cuda.synchronize()
    keep = torch.arange(md, device="cuda")[None, :] < count[:, None]
    assert torch.equal(on, count) and torch.equal(os_, scores * keep) and torch.equal(oc, cls * keep)
    assert torch.equal(ob, boxes * keep[:, :, None])


@pytest.mark.gpu
@pytest.mark.parametrize("arch,size,int8,N", [("tiny_yolo_v3", [512, 640], True, 4800), ("slim_yolo_v2", [256, 832], False, 4160)])
def test_nets_at_sizes_above_4096_anchors(arch, size, int8, N):
    import torch
    from cases import synth_state_dict
    from yolo355 import synth
    if arch == "tiny_yolo_v3":
        from yolo355.models.tiny_yolo_v3 import YOLOv3tiny as M
        anchors = synth.TINY_MULTI_ANCHOR_SIZE
    else:
        from yolo355.models.slim_yolo_v2 import SlimYOLOv2 as M
        anchors = synth.ANCHOR_SIZE
    C, B = 3, 1
    m = M("cuda:0", input_size=size, num_classes=C, trainable=False, conf_thresh=0.02, nms_thresh=0.5, anchor_size=anchors,
          max_candidates=N)
    m.load_state_dict(synth_state_dict(m.state_dict(), 5, weight_gain=2.0))
    m.eval()
    frames = synth.make_frames_u8(21, B, size[0], size[1], "blocks")
    x = torch.from_numpy(synth.normalize_frames(frames))
    if int8:
        m.forward_batch(x, quantization=True)
    net = m._get_net(B, int8=int8)
    assert net.num_anchors_total == N and net.max_candidates == N and net.max_det == N
    _below_and_above(lambda: net.forward(x, tap=True), lambda: net.candidates(B), lambda c: net.set_thresholds(c, 0.5),
                     net.set_max_candidates, N, C)
    assert net.max_det == 4096
    net.close()
