"""Calibration on the int8 y355_net graphs themselves (y355_net_calibrate): the restatement
tests/net_calib_ref.py against the reference's goldens and against the definition on the CPU, and the engine against the
restatement bit for bit on the GPU."""
import os
import re

import numpy as np
import pytest

import int8_wide_ref as W
import net_calib_ref as R
from cases import E2E
from oracle import net_int8_oracle as N
from oracle import yolo_oracle as O
from yolo355 import _ffi, prep, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NEW = ["y355_net_num_trackers", "y355_net_set_trackers", "y355_net_get_trackers", "y355_net_calibrate", "y355_net_calibrate_u8"]
CLASSES = 2
ANCH = {"slim_yolo_v2": synth.ANCHOR_SIZE_MASK, "tiny_yolo_v3": synth.TINY_MULTI_ANCHOR_SIZE, "yolo_v2": synth.ANCHOR_SIZE,
        "yolo_v3": synth.MULTI_ANCHOR_SIZE, "yolo_v3_spp": synth.MULTI_ANCHOR_SIZE}
NLEV = {"slim_yolo_v2": 1, "tiny_yolo_v3": 2, "yolo_v2": 1, "yolo_v3": 3, "yolo_v3_spp": 3}
SIZE = {"slim_yolo_v2": [64, 96], "tiny_yolo_v3": [96, 128], "yolo_v2": [96, 128], "yolo_v3": [64, 96], "yolo_v3_spp": [64, 96]}
GAIN = {"yolo_v3": 1.3, "yolo_v3_spp": 1.3}


def _predc(arch):
    return len(ANCH[arch]) // NLEV[arch] * (5 + CLASSES)


def _qlayers(arch, seed, channel_level=False, scale_layer=None):
    folded = R.make_folded(arch, seed, _predc(arch), GAIN.get(arch, 2.0))
    if scale_layer is not None:
        li, f = scale_layer
        folded[li] = (folded[li][0] * np.float32(f), folded[li][1] * np.float32(f))
    return prep.quantize_folded(folded, channel_level, None)


def _images(seed, B, size):
    return np.concatenate([synth.make_images(seed + i, 1, size[0], size[1]) for i in range(B)])


def _fresh(arch):
    return [R.Tracker() for _ in range(len(R.graph(arch).C) + 1)]


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_ffi_agree_on_the_new_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(_ffi.HEADER_PATH).read(), flags=re.S)
    lib = _ffi.lib()
    ctype = {"int": "c_int", "double": "c_double"}
    for name in NEW:
        assert name in _ffi.declared_symbols() and hasattr(lib, name)
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        res, sig = _ffi._SIGS[name]
        assert res is _ffi.C.c_int and len(sig) == len(args), (name, args)
        for a, t in zip(args, sig):
            if "*" in a:
                assert t is _ffi.C.c_void_p or hasattr(t, "contents"), (name, a)
            else:
                assert t.__name__ == ctype[a.split()[0]], (name, a)


def test_blend_is_the_upsample_rule_before_its_rounding():
    q = np.random.default_rng(5).integers(-127, 128, size=(2, 3, 5, 7))
    for d in (-2, 0, 1):
        want = N.upsample_int(q, 2.0 ** d)
        got = np.clip(np.rint(R.blend(q) * np.float32(2.0 ** d)), -127, 127).astype(np.int64)
        assert np.array_equal(got, want)


def test_slim_first_frozen_step_gives_the_references_exponents():
    """the general rule on the graph the reference has: the 11 exponents of its own calibration forward (e2e.npz c1)"""
    golden = np.load(os.path.join(GOLD, "e2e.npz"))
    wkw, anchors, pattern = E2E["c1"]
    meta = [int(v) for v in golden["c1/meta"]]
    H, Wd, C, calib_seed = meta[:4]
    ql = O.quantize_layers(synth.make_weights(**wkw, num_classes=C))
    xc = synth.make_images(calib_seed, 1, H, Wd, pattern)
    tr = _fresh("slim_yolo_v2")
    r = R.step("slim_yolo_v2", xc, ql, tr, True, predc=ql[-1]["q_w"].shape[0])
    assert [r["sa_in"]] + r["sa"] == [int(v) for v in golden["c1/sa"]]
    assert not r["late"]


def test_slim_ema_reproduces_the_references_trackers():
    r2 = np.load(os.path.join(GOLD, "r2.npz"))
    H, Wd, C, B = [int(v) for v in r2["ema/meta"][:4]]
    seeds = [int(v) for v in r2["ema/meta"][4:]]
    ql = O.quantize_layers(synth.make_weights(seed=2, num_classes=C))
    tr = _fresh("slim_yolo_v2")
    for it, s in enumerate(seeds):
        r = R.step("slim_yolo_v2", synth.make_images(s, B, H, Wd), ql, tr, False, predc=ql[-1]["q_w"].shape[0])
        assert [r["sa_in"]] + r["sa"] == [int(v) for v in r2["ema/prequant/sa"][it]], it
        sc = np.array([float(t.scale.item()) for t in tr], np.float32)
        assert np.allclose(sc, r2["ema/prequant/scale"][it], rtol=1e-6, atol=0), it


# the route layer's weights scaled so that the late producer's maximum gives another exponent than the first producer's
MULTI = [("tiny_yolo_v3", 4, 8, 64.0), ("yolo_v2", 23, 20, 64.0)]


@pytest.mark.parametrize("arch,buf,layer,factor", MULTI, ids=[m[0] for m in MULTI])
def test_multi_producer_rule_against_its_definition(arch, buf, layer, factor):
    size = [96, 128]
    ql = _qlayers(arch, 11, scale_layer=(layer, factor))
    tr = _fresh(arch)
    x = _images(300, 1, size)
    r = R.step(arch, x, ql, tr, True, predc=_predc(arch))
    assert buf in r["late"]
    # the fixture exercises the rule: the buffer's final exponent differs from the one its first producer gave it
    assert r["sa"][buf] != r["first_sa"][buf], (r["sa"][buf], r["first_sa"][buf])
    # direct evaluation of the definition: the pass ran on the provisional exponents -- recompute every producer's maximum
    # from the tensors of a forward under first_sa, and update a fresh tracker with the maximum over all of them
    g = R.graph(arch)
    f = R.forward_int(arch, x, ql, r["sa_in"], r["first_sa"], _predc(arch))
    for t in range(len(g.C)):
        assert np.array_equal(f["t"][t], r["t"][t]), t
    ms = []
    for o in g.ops:
        if o["o"] != buf or o["op"] == "spp":
            continue
        if o["op"] == "conv":
            u, fb = R.pre_requant(W.conv_int(f["t"][o["i"]][:, :o["cin"]], np.asarray(ql[o["layer"]]["q_w"]), 1), ql[o["layer"]],
                                  r["first_sa"][o["i"]], o["act"])
            ms.append(float(np.abs(u).max()) * 2.0 ** -fb)
        elif o["op"] == "up":
            ms.append(float(np.abs(R.blend(f["t"][o["i"]])).max()) * 2.0 ** -r["first_sa"][o["i"]])
        else:
            ms.append(float(np.abs(f["t"][o["i"]]).max()) * 2.0 ** -r["first_sa"][o["i"]])
    assert len(ms) == 2 and ms[1] > ms[0]
    assert float(r["max"][buf + 1]) == pytest.approx(max(ms), rel=1e-6)
    want = R.Tracker()
    assert want.update(np.float32(max(ms)), True) == r["sa"][buf] and want.bits == tr[buf + 1].bits
    first = R.Tracker()
    assert first.update(np.float32(ms[0]), True) == r["first_sa"][buf]
    # a pool that reads the buffer mirrors the final entry
    for o in g.ops:
        if o["op"] == "pool" and o["i"] == buf:
            assert r["sa"][o["o"]] == r["sa"][buf] and tr[o["o"] + 1].bits == tr[buf + 1].bits


# ---------------------------------------------------------------------------------------------------- GPU
def _net(arch, size, B, dtype="int8", ql=None, conf=0.05):
    from yolo355.netengine import Net
    net = Net(arch, size, CLASSES, ANCH[arch], conf_thresh=conf, nms_thresh=0.5, max_batch=B, dtype=dtype)
    for i, q in enumerate(ql or []):
        net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
    return net


def _same_state(net, tr, r):
    scale, first = net.trackers
    assert [int(v) for v in scale.view(np.uint32)] == [t.bits for t in tr]
    assert [int(v) for v in first] == [t.first_a for t in tr]
    sa_in, sa = net.get_act_exponents()
    assert (sa_in, sa) == (r["sa_in"], r["sa"])
    assert np.array_equal(net.last_calibration_max.view(np.uint32), r["max"].view(np.uint32)), \
        [(k, a, b) for k, (a, b) in enumerate(zip(net.last_calibration_max, r["max"])) if a != b]


@pytest.mark.gpu
@pytest.mark.parametrize("pc", [False, True], ids=["per_tensor", "per_channel"])
@pytest.mark.parametrize("arch", R.ARCHS)
def test_three_steps_equal_the_restatement_bit_for_bit(arch, pc):
    size, B = SIZE[arch], 2
    ql = _qlayers(arch, 21, channel_level=pc)
    net = _net(arch, size, B, ql=ql)
    tr = _fresh(arch)
    for k, (freeze, seed) in enumerate([(True, 500), (False, 510), (False, 520)]):
        x = _images(seed, B, size)
        got = net.calibrate(x, freeze=freeze)
        r = R.step(arch, x, ql, tr, freeze, predc=_predc(arch))
        assert got == (r["sa_in"], r["sa"]), k
        _same_state(net, tr, r)
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2"])
def test_step_on_frames_equals_the_step_on_the_normalised_tensor(arch):
    from oracle import resize_oracle
    size, B = SIZE[arch], 2
    ql = _qlayers(arch, 22)
    frames = synth.make_frames_u8(77, B, 75, 110, "blocks")
    x = synth.normalize_frames(resize_oracle.resize_linear_u8(frames, size[0], size[1]))
    a, b = _net(arch, size, B, ql=ql), _net(arch, size, B, ql=ql)
    assert a.calibrate_frames(frames, freeze=True) == b.calibrate(x, freeze=True)
    for u, v in zip(a.trackers, b.trackers):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(a.last_calibration_max.view(np.uint32), b.last_calibration_max.view(np.uint32))
    same = synth.make_frames_u8(78, B, size[0], size[1], "noise")
    assert a.calibrate_frames(same) == b.calibrate(synth.normalize_frames(same))
    assert np.array_equal(a.trackers[0].view(np.uint32), b.trackers[0].view(np.uint32))
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["tiny_yolo_v3", "yolo_v2", "yolo_v3_spp"])
def test_forward_after_calibration_runs_on_the_calibrated_exponents(arch):
    from test_int8_wide_models import _check_against_restatement
    from helpers import dets_match
    size, B = SIZE[arch], 2
    ql = _qlayers(arch, 23)
    net = _net(arch, size, B, ql=ql)
    x = _images(600, B, size)
    sa_in, sa = net.calibrate(x, freeze=True)
    ref_q = [dict(q_w=np.asarray(q["q_w"], np.int64), q_b=np.asarray(q["q_b"], np.int64), e_w=int(q["e_w"]), e_b=int(q["e_b"])) for q in ql]
    if arch == "tiny_yolo_v3":
        ref = N.tiny_detect(x, ref_q, sa_in, sa, size, ANCH[arch], CLASSES, conf_thresh=0.05)
        out = net.forward(x, tap=True)
        for t in range(net.num_tensors):
            got = np.rint(net.get_tensor(t, B).astype(np.float64) * 2.0 ** sa[t]).astype(np.int64)
            assert np.array_equal(got[:, :ref["t"][t].shape[1]], ref["t"][t]), t
        assert net.counters() == ref["sat"]
        cb, cs, cc = net.candidates(B)
        assert np.allclose(cb, ref["box"], atol=2e-5, rtol=0) and np.allclose(cs, ref["cls_scores"].max(axis=2), atol=2e-6, rtol=1e-5)
        for i in range(B):
            ok, msg = dets_match(ref["dets"][i][:3], out[i], all_scores=ref["cls_scores"][i].max(axis=1))
            assert ok, (i, msg)
    else:
        ref = W.forward_int(arch, x, ref_q, sa_in, sa, _predc(arch))
        out = _check_against_restatement(net, x, ref, arch, size, ANCH[arch], CLASSES, 0.05)
    # frames: the same handle, the same exponents
    frames = synth.make_frames_u8(79, B, size[0], size[1], "blocks")
    a, b = net.forward_frames(frames), net.forward(synth.normalize_frames(frames))
    for i in range(B):
        assert all(np.array_equal(u, v) for u, v in zip(a[i], b[i]))
    # calibration left no routing state behind: the production routes are back
    fresh = _net(arch, size, B, ql=ql)
    fresh.set_act_exponents(sa_in, sa)
    fresh.forward(x)
    net.forward(x)
    routes = [net.layer_route(i) for i in range(net.num_layers)]
    assert routes == [fresh.layer_route(i) for i in range(net.num_layers)]
    fam = {r & 0xff for r in routes}
    assert fam & {net.ROUTE_RING, net.ROUTE_POINTWISE, net.ROUTE_FRONT}, routes
    net.close()
    fresh.close()


@pytest.mark.gpu
def test_set_trackers_of_get_trackers_continues_the_same_calibration():
    arch, size, B = "yolo_v2", SIZE["yolo_v2"], 2
    ql = _qlayers(arch, 24)
    a, b = _net(arch, size, B, ql=ql), _net(arch, size, B, ql=ql)
    a.calibrate(_images(700, B, size), freeze=True)
    b.trackers = a.trackers
    assert b.get_act_exponents() == a.get_act_exponents()
    x = _images(710, B, size)
    assert a.calibrate(x) == b.calibrate(x)
    for u, v in zip(a.trackers, b.trackers):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    a.close()
    b.close()


@pytest.mark.gpu
def test_calibrated_model_survives_its_state_dict():
    import torch
    from test_int8_wide_models import _model
    size, B = [64, 96], 2
    m, _ = _model("yolo_v2", "myYOLOv2", size, 20, 4100, 2.0, device="cuda")
    keys = set(m.state_dict())
    x = torch.from_numpy(_images(800, B, size)).cuda()
    m.calibrate(x, freeze=True)
    m.calibrate(torch.from_numpy(_images(810, B, size)).cuda())
    assert set(m.state_dict()) == keys | {"act_tracker_scale", "act_tracker_first_a"}
    assert "f" not in m.__dict__.get("_nets", {})             # no bf16 net was ever built
    want = m.forward_batch(x, quantization=True)
    m2, _ = _model("yolo_v2", "myYOLOv2", size, 20, 4100, 2.0, device="cuda")
    m2.load_state_dict(m.state_dict())
    assert m2.act_exponents == m.act_exponents
    got = m2.forward_batch(x, quantization=True)
    assert "f" not in m2.__dict__.get("_nets", {})
    for i in range(B):
        assert all(np.array_equal(u, v) for u, v in zip(want[i], got[i]))


@pytest.mark.gpu
def test_error_paths_leave_the_handle_as_it_was():
    arch, size, B = "tiny_yolo_v3", SIZE["tiny_yolo_v3"], 1
    x = _images(900, B, size)
    bf = _net(arch, size, B, dtype="bf16")
    with pytest.raises(_ffi.Y355Error) as e:
        bf.calibrate(x)
    assert e.value.code == _ffi.EINVAL
    bf.close()
    ql = _qlayers(arch, 25)
    net = _net(arch, size, B)
    with pytest.raises(_ffi.Y355Error) as e:
        net.calibrate(x)
    assert e.value.code == _ffi.ENOTREADY
    for i, q in enumerate(ql):
        net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
    import torch
    xd = torch.from_numpy(x).cuda()
    lib = _ffi.lib()
    for n in (net.num_trackers - 1, net.num_trackers + 1):
        assert lib.y355_net_calibrate(net._h, xd.data_ptr(), B, 1, 0.1, None, None, None, n) == _ffi.EINVAL
    assert not net.trackers[1].any()                           # none of them touched the state
    net.calibrate(x, freeze=True)
    state, exps = net.trackers, net.get_act_exponents()
    # a step that fails half-way (a layer whose outputs are all zero has no scale: Y355_ERANGE at its tracker)
    z = ql[5]
    net.load_layer_i8(5, np.zeros_like(z["q_w"]), np.zeros_like(z["q_b"]), z["e_w"], z["e_b"])
    with pytest.raises(_ffi.Y355Error) as e:
        net.calibrate(_images(910, B, size), freeze=False)
    assert e.value.code == _ffi.ERANGE
    assert net.get_act_exponents() == exps
    for u, v in zip(net.trackers, state):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    net.close()


# relative L2 of the int8 maps against the reference's fp32 maps under SELF-calibrated exponents (one frozen first step on
# the golden input), held to the bounds tests/test_int8_wide_models.py asserts for exponents from the float activations
@pytest.mark.parametrize("case", range(3), ids=["yolo_v2_224", "yolo_v3_224", "yolo_v3_spp_224"])
def test_self_calibrated_maps_track_the_reference_fp32_maps(case):
    import test_int8_wide_models as M
    tag, arch, cls, size, classes, seed, gain = M.CASES[case]
    m, _ = M._model(arch, cls, size, classes, seed, gain)
    folded = N.fold_bn(W.layers_of(m))
    predc = m.anchor_number * (5 + classes)
    x = synth.make_images(seed + 1, 1, size[0], size[1])
    ql = N.quantize_folded(folded)
    r = R.step(arch, x, ql, _fresh(arch), True, predc=predc)
    f = W.forward_int(arch, x, ql, r["sa_in"], r["sa"], predc)
    gold = [M.WGOLD[tag + "_pred"]] if arch == "yolo_v2" else [M.WGOLD[tag + "_pred_%d" % k] for k in (1, 2, 3)]
    rel = [float(np.sqrt(((p.astype(np.float64) - g) ** 2).sum() / (g.astype(np.float64) ** 2).sum()))
           for p, g in zip(W.preds_float(f), gold)]
    print(tag, "self-calibrated relative L2", ["%.4f" % v for v in rel])
    assert max(rel) <= M.REL_L2[arch], rel


def test_self_calibrated_tiny_maps_track_the_reference_fp32_maps():
    """YOLOv3tiny on fp32.npz (tiny_b2, the case tests/test_fp32_models.py holds to 8e-2 with exponents from the float
    activations): the same bound under self-calibrated exponents, one frozen first step on the golden input"""
    from cases import FP32_CASES, fp32_setup
    from oracle import fp32_oracle as F
    case = [c for c in FP32_CASES if c[0] == "tiny_b2"][0]
    tag, arch, size, classes = case[:4]
    layers, anchors, A, x = fp32_setup(case)
    gold = np.load(os.path.join(GOLD, "fp32.npz"))
    ql = N.quantize_folded(N.fold_bn(layers))
    r = R.step(arch, x, ql, _fresh(arch), True, predc=A * (5 + classes))
    ri = N.tiny_detect(x, ql, r["sa_in"], r["sa"], size, anchors, classes)
    fr = F.detect(arch, layers, x, size, anchors, classes)
    mx = [np.abs(t).max() for t in fr["taps"]] + [np.abs(p).max() for p in fr["preds"]]
    rf = N.tiny_detect(x, ql, O.floor_log2_scale(np.abs(x).max())[0], [O.floor_log2_scale(m)[0] for m in mx], size, anchors, classes)

    def rel(preds):
        return [float(np.sqrt(((p.astype(np.float64) - gold["%s/%s" % (tag, n)]) ** 2).sum() /
                              (gold["%s/%s" % (tag, n)].astype(np.float64) ** 2).sum())) for p, n in zip(preds, ("pred_1", "pred_2"))]
    a, b = rel(ri["preds"]), rel(rf["preds"])
    print(tag, "relative L2 self-calibrated", ["%.4f" % v for v in a], "from the float activations", ["%.4f" % v for v in b])
    assert max(a) <= 8e-2, a


@pytest.mark.gpu
def test_prepare_net_package_runs_without_fp32_weights(tmp_path):
    import torch
    from test_int8_wide_models import _model
    from yolo355.netengine import Net
    from yolo355.tools import prepare_net
    size, B, classes = [96, 128], 2, 20
    m, anchors = _model("yolo_v2", "myYOLOv2", size, classes, 4100, 2.0, device="cuda")
    calib = _images(1000, 4 * B, size)
    net, package = prepare_net.prepare("yolo_v2", m.state_dict(), classes, anchors, size, calib, calib_batch=B,
                                       conf_thresh=m.conf_thresh, nms_thresh=m.nms_thresh)
    net.close()
    path = str(tmp_path / "yolo_v2_q.npz")
    np.savez_compressed(path, **package)
    for it in range(4):                                       # the same four batches on the model the package was made from
        m.calibrate(torch.from_numpy(calib[it * B:(it + 1) * B]).cuda(), freeze=False)
    pk = Net.from_package(path, max_batch=B)
    assert pk.get_act_exponents() == m.act_exponents
    assert np.array_equal(pk.trackers[0].view(np.uint32), m.act_tracker_scale.cpu().numpy().view(np.uint32))
    x = _images(1100, B, size)
    want, got = m.forward_batch(torch.from_numpy(x).cuda(), quantization=True), pk.forward(x)
    assert sum(len(d[1]) for d in want) > 0
    for i in range(B):
        assert all(np.array_equal(u, v) for u, v in zip(want[i], got[i]))
    frames = synth.make_frames_u8(81, B, 70, 100, "blocks")
    wf, gf = m.forward_frames(frames, quantization=True), pk.forward_frames(frames)
    for i in range(B):
        assert all(np.array_equal(u, v) for u, v in zip(wf[i], gf[i]))
    sa = pk.calibrate(x)                                       # the holder of the package alone calibrates on
    assert sa == m.calibrate(torch.from_numpy(x).cuda())
    pk.close()
