"""Per-channel power-of-two int8 weights of the y355_net families (y355_net_load_layer_i8_pc, prep.quantize_folded(
channel_level=True), the model classes' channel_level switch).

The integer rule: with one weight exponent e_w[c] per output channel and E = max_c e_w[c],
    F = max(sa_in + E, e_b),  shl[c] = F - sa_in - e_w[c],  t = acc * 2^shl[c] + q_b[c] * 2^(F - e_b)
and everything after t as for one exponent per layer.  A per-channel layer therefore equals the per-tensor layer with the
widened integer weights q_w[c] * 2^(E - e_w[c]) at exponent E, and the existing restatements (int8_wide_ref.py,
oracle/net_int8_oracle.py), which work in int64, are the oracle of the new path as they stand (int8_pc_ref.widen)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import int8_pc_ref as P
import int8_wide_ref as R
from cases import FP32_CASES, fp32_setup
from helpers import dets_match
from test_int8_wide_models import CASES, GPU_CASES, WGOLD, _check_against_restatement, _images, _model, _rne

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "quant_pc.npz"))


def _per_tensor(b):
    from oracle import yolo_oracle as O
    return O.quantize_tensor_pow2(b)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", P.QUANT_PC_CASES, ids=[c[0] for c in P.QUANT_PC_CASES])
def test_quantize_tensor_channel_level_equals_the_reference(case):
    """prep.quantize_tensor / quantize_tensor_b with channel_level=True against the reference's recorded output, bit for bit
    (q, log2(scale) and the scale's shape)"""
    import torch
    from yolo355 import prep
    tag, seed, shape, gain = case
    t = torch.from_numpy(P.quant_pc_input(seed, shape, gain))
    fn = prep.quantize_tensor_b if len(shape) == 1 else prep.quantize_tensor
    q, scale = fn(t, 8, channel_level=True)
    e = torch.log2(scale)
    assert tuple(e.shape) == GOLD[tag + "/e"].shape
    assert np.array_equal(e.numpy().astype(np.int32), GOLD[tag + "/e"])
    assert np.array_equal(q.numpy().astype(np.int32), GOLD[tag + "/q"])
    # the per-tensor forms are unchanged
    q0, s0 = fn(t, 8)
    assert s0.dim() == 0 and float(q0.abs().max()) <= 127


def test_quantize_folded_channel_level_equals_the_independent_version():
    """uncapped, capped at the default and at a given spread; an all-zero channel; a channel beyond max_spread"""
    from yolo355 import prep, synth
    folded = []
    for i, shape in enumerate([(8, 3, 3, 3), (16, 8, 1, 1), (12, 16, 3, 3)]):
        w = (synth.uniform_pm1(700 + i, shape) * 0.4).astype(np.float32)
        w *= (2.0 ** -(np.arange(shape[0]) % 5)).astype(np.float32)[:, None, None, None]
        b = (synth.uniform_pm1(800 + i, (shape[0],)) * 0.1).astype(np.float32)
        folded.append((w, b))
    folded[1][0][3] = 0.0                                 # an all-zero output channel
    folded[2][0][7] *= np.float32(2.0 ** -11)             # a channel far beyond any cap used below
    for ms in (None, 0, 3, 40):
        prod = prep.quantize_folded(folded, channel_level=True, max_spread=ms)
        want = P.quantize_folded_pc(folded, prep.DEFAULT_MAX_SPREAD if ms is None else ms, _per_tensor)
        for a, b in zip(prod, want):
            assert np.asarray(a["e_w"]).shape == (a["q_w"].shape[0],) and np.asarray(a["e_w"]).dtype == np.int32
            assert np.array_equal(a["e_w"], b["e_w"]) and a["e_b"] == b["e_b"]
            assert np.array_equal(a["q_w"], b["q_w"]) and np.array_equal(a["q_b"], b["q_b"])
            assert np.abs(a["q_w"]).max() <= 127
        assert prod[1]["e_w"][3] == prod[1]["e_w"].min() and not prod[1]["q_w"][3].any()
        cap = prep.DEFAULT_MAX_SPREAD if ms is None else ms
        assert prod[2]["e_w"][7] == prod[2]["e_w"].min() + min(cap, 15) or cap >= 15
        assert P.max_spread_of(prod) <= cap
    # spread 0 is the per-tensor recipe; the default call is unchanged
    for a, b in zip(prep.quantize_folded(folded, True, 0), prep.quantize_folded(folded)):
        assert (a["e_w"] == b["e_w"]).all() and np.array_equal(a["q_w"], b["q_w"])
        assert np.ndim(b["e_w"]) == 0


def test_widening_identity_on_exact_rationals():
    """the rule stated in this file's docstring, evaluated on exact rationals, equals the per-tensor restatement on the
    widened weights -- plain and with a residual, three activations"""
    rng = np.random.default_rng(23)
    for trial in range(6):
        cout, cin = 5, 4
        e_w = rng.integers(3, 12, size=cout)
        e_b = int(rng.integers(4, 16))
        L = dict(q_w=rng.integers(-127, 128, size=(cout, cin, 3, 3)), e_w=e_w.astype(np.int32),
                 q_b=rng.integers(-4000, 4000, size=cout).astype(np.int64), e_b=e_b)
        Lw = P.widen([L])[0]
        assert Lw["e_w"] == e_w.max() and np.abs(Lw["q_w"]).max() > 127
        q_in = rng.integers(-127, 128, size=(1, cin, 4, 5))
        acc_pc = R.conv_int(q_in, L["q_w"], 1)              # what the kernel accumulates: the int8 weights
        acc_w = R.conv_int(q_in, Lw["q_w"], 1)
        qr = rng.integers(-127, 128, size=acc_pc.shape)
        for act in (R.L100, R.L125, R.NONE):
            lk, m = R.ACT[act]
            for sa_in, s_r, s_out in [(4, 2, 3), (3, 9, 5), (6, 6, 2)]:
                E = int(e_w.max())
                Fb = max(sa_in + E, e_b)
                plain = R.requant(acc_w, Lw, sa_in, s_out, act)
                res = R.requant(acc_w, Lw, sa_in, s_out, act, qr, s_r)
                for idx in np.ndindex(acc_pc.shape):
                    c = idx[1]
                    shl = Fb - sa_in - int(e_w[c])
                    assert shl >= 0
                    t_int = int(acc_pc[idx]) * 2 ** shl + int(L["q_b"][c]) * 2 ** (Fb - e_b)
                    # the same value from the definition: acc / 2^(sa_in + e_w[c]) + q_b / 2^e_b
                    t = Fraction(int(acc_pc[idx]), 2 ** (sa_in + int(e_w[c]))) + Fraction(int(L["q_b"][c]), 2 ** e_b)
                    assert t * 2 ** Fb == t_int
                    tp = t if t >= 0 else t * Fraction(m, 2 ** lk)
                    assert plain[idx] == _rne(tp * Fraction(2) ** s_out), (trial, act, idx)
                    assert res[idx] == _rne((tp + Fraction(int(qr[idx]), 2 ** s_r)) * Fraction(2) ** s_out), (trial, act, idx)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_per_channel_maps_are_no_further_from_the_reference_fp32_maps(case):
    """the cases of test_restatement_tracks_the_reference_fp32_maps: relative L2 against models_wide.npz, map by map,
    per channel (uncapped) <= per tensor.  Measured: yolo_v2_224 0.0842 <= 0.0909; yolo_v3_224 0.0278 / 0.0354 / 0.0337 <=
    0.0300 / 0.0357 / 0.0365; yolo_v3_spp_224 0.0290 / 0.0347 / 0.0366 <= 0.0314 / 0.0354 / 0.0402."""
    from oracle import net_int8_oracle as N
    from yolo355 import synth
    tag, arch, cls, size, classes, seed, gain = case
    m, anchors = _model(arch, cls, size, classes, seed, gain)
    folded = N.fold_bn(R.layers_of(m))
    predc = m.anchor_number * (5 + classes)
    x = synth.make_images(seed + 1, 1, size[0], size[1])
    sa_in, sa, T = R.calibrate_f64(arch, x, folded, predc)
    gold = [WGOLD[tag + "_pred"]] if arch == "yolo_v2" else [WGOLD[tag + "_pred_%d" % k].astype(np.float64) for k in (1, 2, 3)]

    def rel(q):
        r = R.forward_int(arch, x, q, sa_in, sa, predc)
        return [float(np.sqrt(((p.astype(np.float64) - ref) ** 2).sum() / (ref.astype(np.float64) ** 2).sum()))
                for p, ref in zip(R.preds_float(r), gold)]
    pt = rel(N.quantize_folded(folded))
    pc = rel(P.widen(P.quantize_folded_pc(folded, None, _per_tensor)))
    print(tag, "relative L2 per tensor", ["%.4f" % v for v in pt], "per channel", ["%.4f" % v for v in pc])
    for a, b in zip(pc, pt):
        assert a <= b, (pc, pt)


def test_header_and_ffi_declare_the_per_channel_entry_points():
    from yolo355 import _ffi
    declared = _ffi.declared_symbols()
    for n in ("y355_net_load_layer_i8_pc", "y355_net_layer_route"):
        assert n in declared and n in _ffi._SIGS, n
    lib = _ffi.lib()
    buf = (C.c_int32 * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.y355_net_load_layer_i8_pc(None, 0, p, p, 1, 1, 3, p, 0) == _ffi.EINVAL
    assert lib.y355_net_layer_route(None, 0, buf) == _ffi.EINVAL
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yolo355.h")).read()
    for d in ("Y355_ROUTE_FIRST", "Y355_ROUTE_RING", "Y355_ROUTE_POINTWISE", "Y355_ROUTE_GENERIC8", "Y355_ROUTE_EPI64",
              "Y355_ROUTE_RESIDUAL", "Y355_ROUTE_PER_CHANNEL"):
        assert "#define " + d in hdr


# ---------------------------------------------------------------------------------------------------- GPU
ROUTES_SEEN = set()          # (family, epilogue 64, residual) of the per-channel layers the GPU tests of this file ran


def _note_routes(net, qlayers):
    from yolo355.netengine import Net
    fams = {}
    for i, L in enumerate(qlayers):
        r = net.layer_route(i)
        pc = np.ndim(L["e_w"]) and int(np.max(L["e_w"]) != np.min(L["e_w"]))
        assert bool(r & Net.ROUTE_PER_CHANNEL) == bool(pc), (i, hex(r))
        if pc:
            ROUTES_SEEN.add((r & 0xff, bool(r & Net.ROUTE_EPI64), bool(r & Net.ROUTE_RESIDUAL)))
        fams[i] = r
    return fams


def _spread_bn(m, k):
    """scale gamma and beta of every BatchNorm by 2^-(c mod k): the folded weights and biases of channel c scale by exactly
    that power of two"""
    import torch
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                s = 2.0 ** -(torch.arange(mod.num_features) % k).float()
                mod.weight.mul_(s.to(mod.weight.device))
                mod.bias.mul_(s.to(mod.bias.device))


DARK = [c for c in GPU_CASES if c[0] in ("yolo_v2_224x320", "yolo_v3_224", "yolo_v3_spp_224")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DARK, ids=[c[0] for c in DARK])
def test_per_channel_darknet_bit_exact(case):
    """the drop-in with channel_level = True on channels spread over 6 more bits, B = 2: every tensor of a tap forward, the
    clamp count, the candidates and the detections against the restatement on the widened weights; the plain forward and
    forward_frames give the same detections"""
    import torch
    from oracle import net_int8_oracle as N
    from yolo355 import prep, synth
    from yolo355.utils.modules import folded_f32
    tag, arch, cls, size, classes, seed, gain = case
    assert len(DARK) == 3
    B = 2
    m, anchors = _model(arch, cls, size, classes, seed, gain, device="cuda")
    _spread_bn(m, 7)
    m.channel_level, m.max_spread = True, 8
    predc = m.anchor_number * (5 + classes)
    x = _images(seed, B, size)
    first = m.forward_batch(torch.from_numpy(x).cuda(), quantization=True)
    exps = m.act_exponents
    net = m._get_net(B, int8=True)
    folded = N.fold_bn(R.layers_of(m))
    qpc = P.quantize_folded_pc(folded, 8, _per_tensor)
    assert P.max_spread_of(qpc) >= 6, "the fixture no longer spreads the channels: the shifts would not matter"
    for a, b in zip(prep.quantize_folded([folded_f32(c) for c in m._conv_modules()], True, 8), qpc):
        assert np.array_equal(a["e_w"], b["e_w"]) and np.array_equal(a["q_w"], b["q_w"]) and a["e_b"] == b["e_b"]
    ref = R.forward_int(arch, x, P.widen(qpc), exps[0], exps[1], predc)
    out = _check_against_restatement(net, x, ref, arch, size, anchors, classes, 0.05)
    _note_routes(net, qpc)
    for i in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(first[i], out[i]))
    out2 = net.forward(x)
    _note_routes(net, qpc)
    for i in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(out[i], out2[i]))
    if arch == "yolo_v3":                                     # one frames case: uint8 input through the same layers
        frames = synth.make_frames_u8(31, B, size[0], size[1], "blocks")
        xf = synth.normalize_frames(frames)
        want = m.forward_batch(torch.from_numpy(xf).cuda(), quantization=True)
        reff = R.forward_int(arch, xf, P.widen(qpc), exps[0], exps[1], predc)
        got = m.forward_frames(frames, quantization=True)
        assert net.counters() == reff["sat"]
        for i in range(B):
            assert all(np.array_equal(a, b) for a, b in zip(want[i], got[i]))
        nt = net.num_tensors
        for t in (nt - 1, nt - 3, nt - 5):
            gq = np.rint(net.get_tensor(t, B).astype(np.float64) * 2.0 ** reff["sa"][t]).astype(np.int64)
            assert np.array_equal(gq, reff["t"][t])


def _small_setup(case):
    """(bf16-calibrated exponents, int8 Net, per-channel layers spread over >= 6 bits, anchors, x) of a FP32_CASES row"""
    from oracle import net_int8_oracle as N
    from yolo355.netengine import Net
    tag, arch, size, classes = case[:4]
    layers, anchors, A, x = fp32_setup(case)
    folded = P.spread_channels(N.fold_bn(layers), 7)
    B = x.shape[0]
    fnet = Net(arch, size, classes, anchors, 0.01, 0.5, max_batch=B, device="cuda:0", dtype="bf16")
    for i, (w, b) in enumerate(folded):
        fnet.load_layer(i, w, b)
    sa_in, sa = fnet.calibration_exponents(x)
    fnet.close()
    qpc = P.quantize_folded_pc(folded, 8, _per_tensor)
    assert P.max_spread_of(qpc) >= 6
    net = Net(arch, size, classes, anchors, 0.01, 0.5, max_batch=B, device="cuda:0", dtype="int8")
    for i, q in enumerate(qpc):
        net.load_layer_i8(i, q["q_w"], q["q_b"], q["e_w"], q["e_b"])
    net.set_act_exponents(sa_in, sa)
    return net, qpc, (sa_in, sa), anchors, x


def _small_reference(case, qlayers, sa_in, sa, anchors, x):
    from oracle import fp32_oracle as F
    from oracle import net_int8_oracle as N
    from oracle import yolo_oracle as O
    tag, arch, size, classes = case[:4]
    if arch == "tiny_yolo_v3":
        return N.tiny_detect(x, qlayers, sa_in, sa, size, anchors, classes)
    r = P.slim_forward_int(x, qlayers, sa_in, sa)
    pred = r["t"][-1].astype(np.float32) * np.float32(2.0 ** -r["sa"][-1])
    box, sc = O.head_decode(pred, size, anchors, classes)
    r.update(box=np.asarray(box), cls_scores=np.asarray(sc),
             dets=[O.postprocess(box[i], sc[i], 0.01, 0.5, classes) for i in range(box.shape[0])])
    return r


def _check_small(net, ref, B):
    from yolo355.netengine import Net
    sa_eff = net.get_act_exponents()[1]
    assert sa_eff == ref["sa"]
    out = net.forward(net_x(net), tap=True)
    for t in range(net.num_tensors):
        got = np.rint(net.get_tensor(t, B).astype(np.float64) * 2.0 ** sa_eff[t]).astype(np.int64)
        assert np.array_equal(got, ref["t"][t]), "tensor %d differs in %d places" % (t, int((got != ref["t"][t]).sum()))
    assert net.counters() == ref["sat"]
    cb, cs, cc = net.candidates(B)
    assert np.allclose(cb, ref["box"], atol=2e-5, rtol=0)
    assert np.allclose(cs, ref["cls_scores"].max(axis=2), atol=2e-6, rtol=1e-5)
    for bi in range(B):
        ok, msg = dets_match(ref["dets"][bi][:3], out[bi], all_scores=cs[bi])
        assert ok, (bi, msg)
    assert (net.layer_route(0) & 0xff) == Net.ROUTE_FIRST
    tap_t = [net.get_tensor(t, B) for t in range(net.num_tensors)]
    # the plain forward: a per-channel first or second layer keeps the fused front end out (one shift per layer there), so the
    # two layers run one by one and conv1's map is written
    out2 = net.forward(net_x(net))
    assert (net.layer_route(0) & 0xff) == Net.ROUTE_FIRST and (net.layer_route(1) & 0xff) != Net.ROUTE_FRONT
    for t in range(net.num_tensors):
        assert np.array_equal(net.get_tensor(t, B), tap_t[t]), t
    assert net.counters() == ref["sat"]
    for bi in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(out[bi], out2[bi]))
    return out


def _first_layer_forms(case, net, qpc, sa_in0, sa, anchors):
    """the per-channel first layer (conv1.hip) on its 32-bit (gen32) and its 64-bit route, each from fp32 input and from uint8
    frames (forward_frames at the network size reads the frames in the first-layer kernel): every tensor equal between the
    two inputs, conv1's map equal to the restatement, the route as expected"""
    from yolo355 import synth
    from yolo355.netengine import Net
    tag, arch, size, classes = case[:4]
    B = 2
    frames = synth.make_frames_u8(41, B, size[0], size[1], "blocks")
    xf = synth.normalize_frames(frames)
    sa_in = min(sa_in0, int(np.floor(np.log2(127.0 / np.abs(xf).max()))))      # the frames' own range: no input clamps
    coarse = [dict(L) for L in qpc]
    coarse[0]["e_w"] = (qpc[0]["e_w"] - (np.arange(16) % 19)).astype(np.int32)
    fine = [dict(L) for L in qpc]                 # (the same integers at other scales: different but valid layers)
    fine[0]["e_w"] = (qpc[0]["e_w"].max() - (np.arange(16) % 2)).astype(np.int32)
    for q, want64 in ((fine, False), (coarse, True)):
        net.load_layer_i8(0, q[0]["q_w"], q[0]["q_b"], q[0]["e_w"], q[0]["e_b"])
        net.set_act_exponents(sa_in, sa)
        ref = _small_reference(case, P.widen(q), sa_in, sa, anchors, xf)
        for tap in (True, False):
            a = net.forward(xf, tap=tap)
            ta = [net.get_tensor(t, B) for t in range(net.num_tensors)]
            ca = net.counters()
            b = net.forward_frames(frames, tap=tap)
            tb = [net.get_tensor(t, B) for t in range(net.num_tensors)]
            r = net.layer_route(0)
            assert (r & 0xff) == Net.ROUTE_FIRST and r & Net.ROUTE_PER_CHANNEL and bool(r & Net.ROUTE_EPI64) == want64, hex(r)
            for t in range(net.num_tensors):
                assert np.array_equal(ta[t], tb[t]), t
            for t in range(net.num_tensors):
                got = np.rint(tb[t].astype(np.float64) * 2.0 ** ref["sa"][t]).astype(np.int64)
                assert np.array_equal(got, ref["t"][t]), t
            # (the clamp COUNT against the restatement is _check_small's: on these frames pooled layers clamp, where the engine
            # counts pooled outputs and oracle/net_int8_oracle.conv_layer counts positions before the pool -- for per-tensor
            # layers alike)
            assert ca == net.counters()
            for i in range(B):
                assert all(np.array_equal(u, v) for u, v in zip(a[i], b[i]))
        _note_routes(net, q)
    net.load_layer_i8(0, qpc[0]["q_w"], qpc[0]["q_b"], qpc[0]["e_w"], qpc[0]["e_b"])
    net.set_act_exponents(sa_in0, sa)


_X = {}


def net_x(net):
    return _X[id(net)]


SMALL = [c for c in FP32_CASES if c[0] in ("slim_b2", "tiny_b2")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_per_channel_slim_and_tiny_bit_exact(case):
    """SlimYOLOv2 and YOLOv3tiny, B = 2, channels spread over 6 more bits: tap and plain forwards against the integer oracle
    on the widened weights (the first layer runs on conv1.hip with per-lane shifts, the fused front end stays out)"""
    assert len(SMALL) == 2
    net, qpc, (sa_in, sa), anchors, x = _small_setup(case)
    _X[id(net)] = x
    ref = _small_reference(case, P.widen(qpc), sa_in, sa, anchors, x)
    _check_small(net, ref, x.shape[0])
    _note_routes(net, qpc)
    _first_layer_forms(case, net, qpc, sa_in, sa, anchors)
    # equal exponents through the per-channel entry point = the per-tensor load: same tensors, and the fused front end is back
    from oracle import net_int8_oracle as N
    from yolo355.netengine import Net
    layers = fp32_setup(case)[0]
    qpt = N.quantize_folded(P.spread_channels(N.fold_bn(layers), 7))
    B = x.shape[0]
    res = []
    for per_channel_call in (False, True):
        for i, q in enumerate(qpt):
            e = np.full(q["q_w"].shape[0], q["e_w"], np.int32) if per_channel_call else q["e_w"]
            net.load_layer_i8(i, q["q_w"], q["q_b"], e, q["e_b"])
        net.set_act_exponents(sa_in, sa)
        out = net.forward(x, tap=True)
        t = [net.get_tensor(k, B) for k in range(net.num_tensors)]
        c = net.counters()
        net.forward(x)
        res.append((out, t, c, [net.layer_route(i) for i in range(len(qpt))]))
    (o0, t0, c0, r0), (o1, t1, c1, r1) = res
    assert c0 == c1 and r0 == r1 and not any(r & Net.ROUTE_PER_CHANNEL for r in r1)
    for a, b in zip(t0, t1):
        assert np.array_equal(a, b)
    for i in range(B):
        assert all(np.array_equal(a, b) for a, b in zip(o0[i], o1[i]))
    ref0 = _small_reference(case, qpt, sa_in, sa, anchors, x)
    for k in range(net.num_tensors):
        assert np.array_equal(np.rint(t0[k].astype(np.float64) * 2.0 ** ref0["sa"][k]).astype(np.int64), ref0["t"][k]), k
    net.close()


@pytest.mark.gpu
def test_per_channel_wide_spread_takes_the_64_bit_epilogue_and_erange():
    """yolo_v3: exponents lowered by up to 16 bits per channel on a 3x3, a 1x1 and a residual layer (the same integers at
    another scale: a different but valid layer) put them on the 64-bit epilogue, bit-exact; 30 bits: shl[c] > 24 is
    Y355_ERANGE at the forward, and the net works again after a valid reload; a residual layer whose per-channel bound
    fails: Y355_ERANGE from set_act_exponents, exponents kept"""
    import torch
    from oracle import net_int8_oracle as N
    from yolo355 import _ffi
    from yolo355.netengine import Net
    tag, arch, cls, size, classes, seed, gain = CASES[1]
    B = 2
    m, anchors = _model(arch, cls, size, classes, seed, gain, device="cuda")
    m.channel_level, m.max_spread = True, 8
    predc = m.anchor_number * (5 + classes)
    x = _images(seed, B, size)
    m.forward_batch(torch.from_numpy(x).cuda(), quantization=True)
    net = m._get_net(B, int8=True)
    sa_in, sa = m.act_exponents
    qpc = P.quantize_folded_pc(N.fold_bn(R.layers_of(m)), 8, _per_tensor)
    g = R.GRAPHS[arch]()
    convs = [o for o in g.ops if o["op"] == "conv"]
    res_l = [o["layer"] for o in convs if o["res"] >= 0][2]
    k3 = [o["layer"] for o in convs if o["res"] < 0 and qpc[o["layer"]]["q_w"].shape[2] == 3 and qpc[o["layer"]]["q_w"].shape[0] >= 128][1]
    k1 = [o["layer"] for o in convs if o["res"] < 0 and qpc[o["layer"]]["q_w"].shape[2] == 1 and qpc[o["layer"]]["q_w"].shape[0] >= 128][1]
    q2 = [dict(L) for L in qpc]
    for li in (res_l, k3, k1):
        q2[li]["e_w"] = (qpc[li]["e_w"] - (np.arange(len(qpc[li]["e_w"])) % 17)).astype(np.int32)
        net.load_layer_i8(li, q2[li]["q_w"], q2[li]["q_b"], q2[li]["e_w"], q2[li]["e_b"])
    ref = R.forward_int(arch, x, P.widen(q2), sa_in, sa, predc)
    _check_against_restatement(net, x, ref, arch, size, anchors, classes, 0.05)
    _note_routes(net, q2)
    for li in (res_l, k3, k1):
        assert net.layer_route(li) & Net.ROUTE_EPI64, (li, hex(net.layer_route(li)))
    assert net.layer_route(res_l) & Net.ROUTE_RESIDUAL
    # shl[c] > 24
    bad = (qpc[k3]["e_w"] - 30 * (np.arange(len(qpc[k3]["e_w"])) % 2)).astype(np.int32)
    net.load_layer_i8(k3, q2[k3]["q_w"], q2[k3]["q_b"], bad, q2[k3]["e_b"])
    with pytest.raises(_ffi.Y355Error) as ei:
        net.forward(x)
    assert ei.value.code == _ffi.ERANGE
    net.load_layer_i8(k3, q2[k3]["q_w"], q2[k3]["q_b"], q2[k3]["e_w"], q2[k3]["e_b"])
    _check_against_restatement(net, x, ref, arch, size, anchors, classes, 0.05)
    # a residual layer: exponents that are accepted with equal weight exponents are refused when one channel is 24 bits
    # coarser (its accumulator shift is 24 bits larger): the bound is evaluated per channel.  The residual tensor's exponent
    # is raised step by step (t' is then shifted further left in the 64-bit sum) until the two loads part
    net.set_act_exponents(sa_in, sa)
    o = [o for o in convs if o["layer"] == res_l][0]
    e_eq = np.full_like(qpc[res_l]["e_w"], qpc[res_l]["e_w"].max())
    e_res = e_eq.copy()
    e_res[0] -= 24
    found = None
    for d in range(0, 60, 2):
        sa3 = list(sa)
        sa3[o["res"]] = min(sa[o["res"]] + d, 64)
        net.load_layer_i8(res_l, qpc[res_l]["q_w"], qpc[res_l]["q_b"], e_eq, qpc[res_l]["e_b"])
        try:
            net.set_act_exponents(sa_in, sa3)
        except _ffi.Y355Error:
            break                                             # refused per tensor too: no further d can tell them apart
        net.set_act_exponents(sa_in, sa)
        keep = net.get_act_exponents()
        net.load_layer_i8(res_l, qpc[res_l]["q_w"], qpc[res_l]["q_b"], e_res, qpc[res_l]["e_b"])
        try:
            net.set_act_exponents(sa_in, sa3)
        except _ffi.Y355Error as e:
            assert e.code == _ffi.ERANGE
            assert net.get_act_exponents() == keep
            found = d
            break
        net.set_act_exponents(sa_in, sa)
    assert found is not None, "no residual exponent separates the per-channel bound from the per-tensor one"
    # the 32-bit residual epilogue with per-channel shifts: small weights (sum |q_w| / 16) and a spread of one bit
    net.set_act_exponents(sa_in, sa)
    q3 = [dict(L) for L in qpc]
    for oo in convs:
        if oo["res"] >= 0:
            li = oo["layer"]
            q3[li]["q_w"] = np.asarray(qpc[li]["q_w"]) // 16
            q3[li]["e_w"] = (e_eq_of(qpc[li]) - (np.arange(len(qpc[li]["e_w"])) % 2)).astype(np.int32)
    for li, L in enumerate(q3):
        net.load_layer_i8(li, L["q_w"], L["q_b"], L["e_w"], L["e_b"])
    ref3 = R.forward_int(arch, x, P.widen(q3), sa_in, sa, predc)
    _check_against_restatement(net, x, ref3, arch, size, anchors, classes, 0.05)
    seen = _note_routes(net, q3)
    narrow_res = [li for li, r in seen.items() if r & Net.ROUTE_RESIDUAL and r & Net.ROUTE_PER_CHANNEL and not r & Net.ROUTE_EPI64]
    assert narrow_res, [hex(r) for r in seen.values()]
    assert all((seen[li] & 0xff) in (Net.ROUTE_GENERIC8, Net.ROUTE_GENERIC4) for li in narrow_res)


def e_eq_of(L):
    return np.full_like(L["e_w"], np.max(L["e_w"]))


@pytest.mark.gpu
def test_every_route_ran_a_per_channel_layer():
    """over the cases above (this test runs after them: file order): the ring kernel, the pointwise kernel, convg8_kernel
    with the 32-bit epilogue, with the 64-bit one, with a residual, and the first-layer kernel"""
    from yolo355.netengine import Net
    if not any(f == Net.ROUTE_FIRST for f, _, _ in ROUTES_SEEN):       # run alone (-k, --lf, another order): run the cases here
        for c in SMALL:
            test_per_channel_slim_and_tiny_bit_exact(c)
    if not any(f == Net.ROUTE_RING for f, _, _ in ROUTES_SEEN):
        for c in DARK:
            test_per_channel_darknet_bit_exact(c)
    if not any(e for _, e, _ in ROUTES_SEEN):
        test_per_channel_wide_spread_takes_the_64_bit_epilogue_and_erange()
    fam = {f for f, _, _ in ROUTES_SEEN}
    assert Net.ROUTE_RING in fam and Net.ROUTE_POINTWISE in fam and Net.ROUTE_FIRST in fam, ROUTES_SEEN
    assert (Net.ROUTE_GENERIC8, False, False) in ROUTES_SEEN, ROUTES_SEEN
    assert any(f == Net.ROUTE_GENERIC8 and e for f, e, r in ROUTES_SEEN), ROUTES_SEEN
    assert (Net.ROUTE_GENERIC8, True, True) in ROUTES_SEEN, ROUTES_SEEN
    assert any(f in (Net.ROUTE_GENERIC8, Net.ROUTE_GENERIC4) and r and not e for f, e, r in ROUTES_SEEN), ROUTES_SEEN
    assert (Net.ROUTE_FIRST, False, False) in ROUTES_SEEN and (Net.ROUTE_FIRST, True, False) in ROUTES_SEEN, ROUTES_SEEN
    assert Net.ROUTE_FRONT not in fam
